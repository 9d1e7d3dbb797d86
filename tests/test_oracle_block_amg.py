"""Independent properties of oracle/linalg.py:BlockSemiAMG, the mirror of csrc/tp_amg_block.hip (pc_cptramg[_QI|_TI]).

The GPU tests compare the kernels with this class, and the class states "the build's own algorithm", so their agreement
says nothing about the algorithm.  Here the class is checked against things it does not share code with: the scalar SemiAMG
on a block-diagonal operator (the same arithmetic), its transfers written out as matrices, and the spectral radius of the
two-grid and multi-level error propagators assembled densely (672 x 672 on the 7 x 8 x 6 box).

Finding pinned by the strict xfails below: the transfers and the block-Jacobi smoother are sound (with the Galerkin coarse
operator P^T A P the two-grid cycle contracts, rho = 0.38), but the lumped non-Galerkin 7-point coarse formula, applied to
the coupling blocks (p,T) and (T,p), makes the cycle divergent (two-grid rho = 2.5 for QI, 1.5 for No; the default
multi-level V-cycle 13.7 for QI).  DESIGN.md 4.7."""
import numpy as np
import pytest

import cases
import oracle.linalg as la
from oracle.engine import OracleEngine

DT, SEED, AMP = 8640.0, 5, 0.3

LUMPED = ("known defect: the lumped non-Galerkin coarse formula applied to the coupling blocks (p,T)/(T,p) "
          "(BlockSemiAMG.bcoarsen, k_bamg_coarsen) makes the system V-cycle divergent; DESIGN.md 4.7")


def block_amg(dims, decoup, **amg_opts):
    """The oracle's system hierarchy, set up on the seeded state -> (engine, BlockSemiAMG, level-0 operator)."""
    spec, u0, *_ = cases.c4_spe10_3d(Nx=dims[0], Ny=dims[1], Nz=dims[2], nphase=2)
    o = OracleEngine(spec, dict(pc="cptramg", decoup=decoup, **amg_opts))
    o.set_old(u0)
    o.set_dt(DT)
    o.set_state(cases.perturbed_state(spec, seed=SEED, amp=AMP))
    o.pc.setup(o.jacobian())
    amg = o.pc.amg_pT
    return o, amg, amg.levels[0].copy()


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


# ---------------------------------------------------------------- block-diagonal operator: two scalar hierarchies
REDUCTION = [
    ("7x8x6_default", (7, 8, 6), dict()),
    ("12x20x10_v33_v12", (12, 20, 10), dict(amg_nu=3, amg_full_levels=1, amg_coarse_pre=1, amg_coarse_post=2)),
    ("11x21x13_v11_to_one_cell", (11, 21, 13), dict(amg_nu=1, amg_min_cells=1)),
]


@pytest.mark.parametrize("name,dims,amg_opts", REDUCTION, ids=[c[0] for c in REDUCTION])
def test_block_diagonal_operator_reduces_to_scalar_hierarchies(name, dims, amg_opts):
    """With the (p,T) and (T,p) blocks zeroed every formula of the system AMG (weights, coarse blocks, 2x2 inverse, dense
    solve) is the scalar one per unknown: component q of the system V-cycle IS the scalar V-cycle on A^{qq}."""
    o, amg, A = block_amg(dims, "QI", **amg_opts)
    A[:, 0, 1] = 0.0
    A[:, 1, 0] = 0.0
    amg.setup(A)
    opts = o.opts
    b = np.random.default_rng(3).standard_normal((2,) + A.shape[3:])
    y = amg.vcycle(b)
    st = [1.0, 1.0, 1.0]       # (replaced by the system hierarchy's schedule below)
    for q in range(2):
        sc = la.SemiAMG(amg.n, st, omega=opts["amg_omega"], min_cells=opts["amg_min_cells"], nu=opts["amg_nu"],
                        full_levels=opts["amg_full_levels"], coarse_pre=opts["amg_coarse_pre"], coarse_post=opts["amg_coarse_post"],
                        tail_post=opts["amg_tail_post"], mid_skip=opts["amg_mid_skip"], dom_tau=0.0)
        sc.sched = list(amg.sched)
        sc.setup(A[:, q, q])
        assert len(sc.levels) == len(amg.levels)
        d = rel2(y[q], sc.vcycle(b[q]))
        print("%s: unknown %d, system vs scalar V-cycle %.3e" % (name, q, d))
        assert d < 1e-12, (name, q, d)
    if "one_cell" in name:
        assert amg.levels[-1].shape[3:] == (1, 1, 1) and len(amg.levels) == 14


# ---------------------------------------------------------------- two levels on 7 x 8 x 6, written out as matrices
class TwoLevel:
    """7 x 8 x 6 with amg_min_cells = 200: levels of 336 and 168 cells.  Dense matrices in the field-major ordering of the
    vectors, index = q*ncell + cell."""

    def __init__(self, decoup):
        self.o, self.amg, A = block_amg((7, 8, 6), decoup, amg_min_cells=200)
        amg = self.amg
        assert len(amg.levels) == 2 and amg.sched == [2]
        self.fshape, self.cshape = A.shape[3:], amg.levels[1].shape[3:]
        self.nf, self.nc = int(np.prod(self.fshape)), int(np.prod(self.cshape))
        assert (self.nf, self.nc) == (336, 168)
        self.A = self.dense(A)
        self.Ac_lumped = self.dense(amg.levels[1])
        P = np.zeros((2*self.nf, 2*self.nc))
        for j in range(2*self.nc):
            e = np.zeros(2*self.nc)
            e[j] = 1.0
            P[:, j] = amg._each(amg.prolong, e.reshape((2,) + self.cshape), 0, self.fshape).reshape(-1)
        R = np.zeros((2*self.nc, 2*self.nf))
        for j in range(2*self.nf):
            e = np.zeros(2*self.nf)
            e[j] = 1.0
            R[:, j] = amg._each(amg.restrict, e.reshape((2,) + self.fshape), 0).reshape(-1)
        self.P, self.R = P, R
        # damped block-Jacobi from the 2x2 diagonal blocks of A itself
        n = self.nf
        Dinv = np.zeros((2*n, 2*n))
        for c in range(n):
            ix = np.array([c, n + c])
            Dinv[np.ix_(ix, ix)] = np.linalg.inv(self.A[np.ix_(ix, ix)])
        self.S = np.eye(2*n) - amg.omega*Dinv @ self.A

    @staticmethod
    def dense(A):
        ncell = int(np.prod(A.shape[3:]))
        perm = np.arange(2*ncell).reshape(ncell, 2).T.reshape(-1)        # field-major position -> cell-interleaved index
        return la.to_csr(A).toarray()[np.ix_(perm, perm)]

    def two_grid_rho(self, C):
        """rho(S^2 (I - P C^-1 P^T A) S^2): V(2,2) with an exact solve of the coarse matrix C."""
        n = self.A.shape[0]
        S2 = self.S @ self.S
        E = S2 @ (np.eye(n) - self.P @ np.linalg.solve(C, self.P.T @ self.A)) @ S2
        return float(np.abs(np.linalg.eigvals(E)).max())


@pytest.fixture(scope="module", params=["QI", "No"])
def two_level(request):
    return TwoLevel(request.param)


def test_restriction_is_the_transpose_of_prolongation(two_level):
    t = two_level
    assert np.array_equal(t.R, t.P.T)
    # C points (even index along the coarsening axis, internal axis 2 = array axis 0) are injected: identity rows
    cell_f = np.arange(t.nf).reshape(t.fshape)
    cell_c = np.arange(t.nc).reshape(t.cshape)
    cf = cell_f[::2].reshape(-1)
    cc = cell_c.reshape(-1)
    assert cf.size == cc.size == t.nc
    for q in range(2):
        rows = t.P[q*t.nf + cf]
        expect = np.zeros_like(rows)
        expect[np.arange(t.nc), q*t.nc + cc] = 1.0
        assert np.array_equal(rows, expect)
    # F points interpolate inside their own unknown, from at most two parents
    ff = cell_f[1::2].reshape(-1)
    for q in range(2):
        rows = t.P[q*t.nf + ff]
        assert np.count_nonzero(rows[:, (1 - q)*t.nc:(2 - q)*t.nc]) == 0
        assert (np.count_nonzero(rows, axis=1) <= 2).all()


def test_sound_parts_converge_with_the_galerkin_coarse_operator(two_level):
    """Same P, R = P^T and smoother, coarse matrix P^T A P: the two-grid V(2,2) cycle contracts."""
    t = two_level
    rho = t.two_grid_rho(t.P.T @ t.A @ t.P)
    print("two-grid V(2,2), Galerkin coarse operator, %s: rho = %.4f" % (t.o.opts["decoup"], rho))
    assert rho < 1.0, rho


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=LUMPED)
def test_two_grid_cycle_with_the_oracles_coarse_operator_converges(two_level):
    t = two_level
    G, n = t.P.T @ t.A @ t.P, t.nc
    dev = {(q, r): float(np.linalg.norm((t.Ac_lumped - G)[q*n:(q + 1)*n, r*n:(r + 1)*n])/np.linalg.norm(G[q*n:(q + 1)*n, r*n:(r + 1)*n]))
           for q in range(2) for r in range(2)}
    print("lumped vs Galerkin coarse operator, relative deviation per block, %s: %s" % (t.o.opts["decoup"], dev))
    rho = t.two_grid_rho(t.Ac_lumped)
    print("two-grid V(2,2), the oracle's lumped coarse operator, %s: rho = %.4f" % (t.o.opts["decoup"], rho))
    assert rho < 1.0, rho


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=LUMPED)
@pytest.mark.parametrize("decoup", ["QI", "No"])
def test_default_system_vcycle_converges(decoup):
    """rho(I - V A) of the default multi-level cycle V(2,2 | 0,1 | tail 2), V assembled column by column."""
    o, amg, A = block_amg((7, 8, 6), decoup)
    assert len(amg.levels) == 4
    Ad = TwoLevel.dense(A)
    n = Ad.shape[0]
    V = np.zeros((n, n))
    shape = (2,) + A.shape[3:]
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        V[:, j] = amg.vcycle(e.reshape(shape)).reshape(-1)
    ev = np.linalg.eigvals(V @ Ad)
    rho = float(np.abs(1.0 - ev).max())
    print("default system V-cycle, %s: rho(I - V A) = %.4g, eigenvalues of V A real part %.3g ... %.3g"
          % (decoup, rho, ev.real.min(), ev.real.max()))
    assert rho < 1.0, rho
