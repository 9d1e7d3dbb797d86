"""Reference of the red-black Gauss-Seidel smoother (tp_options.amg_gs_levels / amg_gs_sweeps) for the tests:
oracle.linalg.SemiAMG with the smoother of its top levels restated.

Level l of a scalar hierarchy is a GS level when  l < L  and it lies above the single-workgroup tail (more than 1024 cells: the
tail is the first level of <= 1024 cells and everything below).  A cell with level-local indices (i0, i1, i2) is red when
i0 + i1 + i2 is even.  Half-sweep of colour c:

    x_i <- x_i + (b_i - (A x)_i) / a0_i     for every cell i of colour c,   other cells unchanged     (no damping),

forward sweep F = red then black, backward sweep B = black then red.  A GS level is V(g, g) whatever nu says:
x = F^g(0);  r = b - A x;  x += P cycle(P^T r);  x = B^g(x).  A relaxation-only level (dom_tau) that is a GS level returns
B^g(F^g(0)).  Transfers, coarse operators, the schedule, the truncation decision and every other level are SemiAMG's.
Not a test module."""
import numpy as np

from oracle.linalg import SemiAMG, spmv_scalar

TAIL_CELLS = 1024
OPTIONS = ("amg_gs_levels", "amg_gs_sweeps")


def red_mask(shape):
    """True at the red cells of an array of shape (n2, n1, n0)."""
    return np.indices(shape).sum(axis=0) % 2 == 0


class GsSemiAMG(SemiAMG):
    def __init__(self, n, strength, gs_levels=0, gs_sweeps=1, **kw):
        super().__init__(n, strength, **kw)
        self.gs_levels, self.gs_sweeps = int(gs_levels), int(gs_sweeps)

    @classmethod
    def from_amg(cls, amg, gs_levels, gs_sweeps=1):
        """The same hierarchy parameters as `amg` (a SemiAMG that has not been set up) with Gauss-Seidel on top."""
        self = cls.__new__(cls)
        self.__dict__.update(amg.__dict__)
        self.gs_levels, self.gs_sweeps = int(gs_levels), int(gs_sweeps)
        return self

    def is_gs(self, lvl):
        return lvl < self.gs_levels and self.levels[lvl][0].size > TAIL_CELLS

    def n_gs_levels(self):
        return sum(self.is_gs(l) for l in range(len(self.levels)))

    def half(self, lvl, colour, b, x):
        """H_colour(b, x): colour 0 red, 1 black."""
        A = self.levels[lvl]
        m = red_mask(b.shape) if colour == 0 else ~red_mask(b.shape)
        return np.where(m, x + (b - spmv_scalar(A, x))/A[0], x)

    def forward(self, lvl, b, x):
        return self.half(lvl, 1, b, self.half(lvl, 0, b, x))

    def backward(self, lvl, b, x):
        return self.half(lvl, 0, b, self.half(lvl, 1, b, x))

    def vcycle(self, b, lvl=0):
        if not self.is_gs(lvl):
            return super().vcycle(b, lvl)
        g = self.gs_sweeps
        x = np.zeros_like(b)
        for _ in range(g):
            x = self.forward(lvl, b, x)
        if not (self.trunc is not None and lvl == self.trunc):
            r = b - spmv_scalar(self.levels[lvl], x)
            x = x + self.prolong(self.vcycle(self.restrict(r, lvl), lvl + 1), lvl, b.shape)
        for _ in range(g):
            x = self.backward(lvl, b, x)
        return x


def swap_into(pc, gs_levels, gs_sweeps=1):
    """Replace the scalar hierarchies of a TwoStagePC (before its setup) by GsSemiAMG with the same parameters."""
    pc.amg_p = GsSemiAMG.from_amg(pc.amg_p, gs_levels, gs_sweeps)
    if pc.amg_T is not None:
        pc.amg_T = GsSemiAMG.from_amg(pc.amg_T, gs_levels, gs_sweeps)
    return pc


def oracle_engine(spec, opts):
    """OracleEngine for `opts` with the two option keys stripped before the oracle sees them and its scalar hierarchies swapped."""
    from oracle.engine import OracleEngine
    o = dict(opts)
    L, g = int(o.pop(OPTIONS[0], 0)), int(o.pop(OPTIONS[1], 1))
    eng = OracleEngine(spec, o)
    swap_into(eng.pc, L, g)
    return eng
