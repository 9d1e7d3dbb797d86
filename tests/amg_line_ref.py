"""Reference of the line relaxation (tp_options.amg_line_levels) for the tests: oracle.linalg.SemiAMG with the
smoother of its top levels restated.

Level l of a scalar hierarchy is a LINE level when  l < L,  it lies above the single-workgroup tail (more than 1024 cells: the
tail is the first level of <= 1024 cells and everything below) and its n0 >= 2.  There every sweep is line-Jacobi along
internal axis 0 (the last array axis):

    x <- x + omega T^-1 (b - A x),    T = tridiag(A[1], A[0], A[2]) along axis 0, one system per line (i1, i2),

the residual taken with the full 7-point operator.  Set-up (Thomas):  d~_0 = a0_0,  m_i = a-_i / d~_{i-1},
d~_i = a0_i - m_i a+_{i-1};  stored m_i and 1/d~_i.  Solve:  y_i = r_i - m_i y_{i-1};  e_i = (y_i - a+_i e_{i+1}) (1/d~_i).
The first pre-sweep from the zero guess is x = omega T^-1 b; a relaxation-only level (dom_tau) that is a line level does its
two sweeps as line sweeps.  Transfers, cycle shape, coarse operators and the truncation decision are SemiAMG's.
Not a test module."""
import numpy as np

from oracle.linalg import SemiAMG, spmv_scalar

TAIL_CELLS = 1024
OPTION = "amg_line_levels"


class LineSemiAMG(SemiAMG):
    def __init__(self, n, strength, line_levels=0, **kw):
        super().__init__(n, strength, **kw)
        self.line_levels = int(line_levels)

    @classmethod
    def from_amg(cls, amg, line_levels):
        """The same hierarchy parameters as `amg` (a SemiAMG that has not been set up) with line relaxation on top."""
        self = cls.__new__(cls)
        self.__dict__.update(amg.__dict__)
        self.line_levels = int(line_levels)
        return self

    def is_line(self, lvl):
        A = self.levels[lvl]
        return lvl < self.line_levels and A[0].size > TAIL_CELLS and A.shape[-1] >= 2

    def n_line_levels(self):
        return sum(self.is_line(l) for l in range(len(self.levels)))

    def setup(self, A):
        super().setup(A)
        self.line = {}
        for lvl in range(len(self.levels)):
            if not self.is_line(lvl):
                continue
            Al = self.levels[lvl]
            n0 = Al.shape[-1]
            m, rd = np.zeros_like(Al[0]), np.zeros_like(Al[0])
            d = Al[0][..., 0].copy()
            rd[..., 0] = 1.0/d
            for i in range(1, n0):
                m[..., i] = Al[1][..., i]/d
                d = Al[0][..., i] - m[..., i]*Al[2][..., i - 1]
                rd[..., i] = 1.0/d
            self.line[lvl] = (m, rd, Al[2])
        return self

    def tsolve(self, lvl, r):
        m, rd, ap = self.line[lvl]
        n0 = r.shape[-1]
        y = np.empty_like(r)
        y[..., 0] = r[..., 0]
        for i in range(1, n0):
            y[..., i] = r[..., i] - m[..., i]*y[..., i - 1]
        e = np.empty_like(r)
        e[..., n0 - 1] = y[..., n0 - 1]*rd[..., n0 - 1]
        for i in range(n0 - 2, -1, -1):
            e[..., i] = (y[..., i] - ap[..., i]*e[..., i + 1])*rd[..., i]
        return e

    def _first(self, lvl, b):
        """the sweep from the zero guess"""
        return self.omega*self.tsolve(lvl, b) if self.is_line(lvl) else self.invd[lvl]*b

    def _smooth(self, lvl, b, x):
        if not self.is_line(lvl):
            return super()._smooth(lvl, b, x)
        return x + self.omega*self.tsolve(lvl, b - spmv_scalar(self.levels[lvl], x))

    def vcycle(self, b, lvl=0):                 # (SemiAMG.vcycle with its two `invd*b` lines replaced by _first)
        A = self.levels[lvl]
        if self.trunc is not None and lvl == self.trunc:
            return self._smooth(lvl, b, self._first(lvl, b))
        if lvl == len(self.levels) - 1:
            if self.coarse is None:
                return b/self.coarse_scalar
            return self.coarse.solve(b.reshape(-1)).reshape(b.shape)
        if lvl < self.full_levels:
            pre, post = self.nu, self.nu
        else:
            pre, post = self.coarse_pre, (self.tail_post if b.size <= 1024 else self.coarse_post)
            if self.mid_skip and b.size > 1024 and (lvl - self.full_levels) % 2 == 1:
                pre, post = 0, 0
        if pre == 0:
            x, r = np.zeros_like(b), b
        else:
            x = self._first(lvl, b)
            for _ in range(pre - 1):
                x = self._smooth(lvl, b, x)
            r = b - spmv_scalar(A, x)
        ec = self.vcycle(self.restrict(r, lvl), lvl + 1)
        x = x + self.prolong(ec, lvl, b.shape)
        for _ in range(post):
            x = self._smooth(lvl, b, x)
        return x


def swap_into(pc, line_levels):
    """Replace the scalar hierarchies of a TwoStagePC (before its setup) by LineSemiAMG with the same parameters."""
    pc.amg_p = LineSemiAMG.from_amg(pc.amg_p, line_levels)
    if pc.amg_T is not None:
        pc.amg_T = LineSemiAMG.from_amg(pc.amg_T, line_levels)
    return pc


def oracle_engine(spec, opts):
    """OracleEngine for `opts` with the option key stripped before the oracle sees it and its scalar hierarchies swapped."""
    from oracle.engine import OracleEngine
    o = dict(opts)
    L = int(o.pop(OPTION, 0))
    eng = OracleEngine(spec, o)
    swap_into(eng.pc, L)
    return eng
