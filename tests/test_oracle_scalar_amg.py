"""Independent properties of oracle/linalg.py:SemiAMG, the mirror of csrc/tp_amg.hip (the pressure and S~ hierarchies of pc_cptr),
and the CPU side of tests/test_gpu_scalar_amg.py.

The GPU tests compare the kernels with this class, and the kernels were written from it, so their agreement says nothing about the
cycle-shape rules.  (a) Here the cycle is composed as ONE dense matrix per shape on the 7 x 8 x 6 box -- P from the interpolation
weights, R = P^T, the level matrices by to_csr, the smoother I - diag(omega/a_0) A -- and SemiAMG.vcycle must reproduce it column by
column; the rules for levels of more than 1024 cells, which that box cannot reach, are held by level tables written out by hand.
(b) For every case of the GPU table, with the oracle alone: the path predicate holds on the level tables, the truncation level is
the named one and no dominance ratio lies within 10 % of amg_dom_tau, a one-ulp perturbation of J, S~ and x moves the oracle's
V-cycles, stage 1 and apply by at most a tenth of the GPU tolerance, and the coarsest grid has at most 200 cells (the global-memory
Gauss-Jordan kernel is one workgroup doing n^3/256 dependent global updates per thread)."""
import numpy as np
import pytest

import cases
import oracle.linalg as la
from oracle.engine import OracleEngine

import test_gpu_scalar_amg as G
from test_gpu_scalar_amg import levels_of, shapes, layout, rel2


# ---------------------------------------------------------------- (a) the cycle as one dense matrix, 7 x 8 x 6
SMALL = dict(Nx=7, Ny=8, Nz=6, nphase=2)
MIN_CELLS = 40


def small_amg(which, **amg_opts):
    """The oracle's hierarchy `which` (0: pressure, 1: S~) on the 7 x 8 x 6 box at the usual seeded state, set up."""
    spec, u0, *_ = cases.c4_spe10_3d(**SMALL)
    o = OracleEngine(spec, dict(pc="cptr", amg_min_cells=MIN_CELLS, amg_dom_tau=0.0, **amg_opts))
    o.set_old(u0)
    o.set_dt(G.DT)
    o.set_state(cases.perturbed_state(spec, seed=G.SEED, amp=G.AMP))
    J, Sm = o.jacobian(want_schur=True)
    o.pc.setup(J, Sm)
    return o.pc.amg_p if which == 0 else o.pc.amg_T


def prolongation(A, a):
    """P (fine cells x coarse cells) of a level with operator A coarsened along internal axis a (array axis 2 - a): even cells are
    injected, an odd cell g takes w-(g) from the coarse cell below it and w+(g) from the one above, if there is one."""
    ax = 2 - a
    fshape = A.shape[1:]
    n = fshape[ax]
    cshape = tuple((m + 1)//2 if q == ax else m for q, m in enumerate(fshape))
    f = np.moveaxis(np.arange(int(np.prod(fshape))).reshape(fshape), ax, 0)
    c = np.moveaxis(np.arange(int(np.prod(cshape))).reshape(cshape), ax, 0)
    wm, wp = (np.moveaxis(w, ax, 0) for w in la.SemiAMG.weights(A, a))
    P = np.zeros((f.size, c.size))
    for i in range(n):
        if i % 2 == 0:
            P[f[i].ravel(), c[i//2].ravel()] = 1.0
        else:
            P[f[i].ravel(), c[(i - 1)//2].ravel()] = wm[i].ravel()
            if (i + 1)//2 < c.shape[0]:
                P[f[i].ravel(), c[(i + 1)//2].ravel()] = wp[i].ravel()
    return P


def cycle_matrix(amg, T, lvl=0):
    """b -> x of the cycle from level `lvl` down, composed from dense matrices by the level table T = [(cells, axis, pre, post)]:
        relaxation-only level      (I + S) D                                   [x1 = D b; x = x1 + D (b - A x1)]
        coarsest level             A^-1
        otherwise                  S^post (Q_pre + P M_c P^T (I - A Q_pre)) + Q_post,   Q_k = (I + S + ... + S^(k-1)) D
    with D = diag(omega/a_0), S = I - D A."""
    A = la.to_csr(amg.levels[lvl][:, None, None]).toarray()
    n = A.shape[0]
    I = np.eye(n)
    D = np.diag((amg.omega/amg.levels[lvl][0]).ravel())
    S = I - D @ A
    if amg.trunc is not None and lvl == amg.trunc:
        return (I + S) @ D
    if lvl == len(amg.levels) - 1:
        return np.linalg.inv(A)

    def Q(k):
        out, Sk = np.zeros((n, n)), I
        for _ in range(k):
            out = out + Sk @ D
            Sk = S @ Sk
        return out
    _, axis, pre, post = T[lvl]
    P = prolongation(amg.levels[lvl], axis)
    M = Q(pre) + P @ cycle_matrix(amg, T, lvl + 1) @ P.T @ (I - A @ Q(pre))
    return np.linalg.matrix_power(S, post) @ M + Q(post)


# id, options, truncation forced after the set-up, (pre, post) of the levels but the coarsest as a function of their number
DENSE_SHAPES = [
    ("v11", dict(amg_nu=1, amg_full_levels=99), None, lambda n: [(1, 1)]*n),
    ("v33", dict(amg_nu=3, amg_full_levels=99), None, lambda n: [(3, 3)]*n),
    ("v44", dict(amg_nu=4, amg_full_levels=99), None, lambda n: [(4, 4)]*n),
    ("every_level_v02", dict(amg_full_levels=0, amg_coarse_pre=0, amg_coarse_post=2, amg_tail_post=2), None, lambda n: [(0, 2)]*n),
    ("every_level_v12", dict(amg_full_levels=0, amg_coarse_pre=1, amg_coarse_post=2, amg_tail_post=2), None, lambda n: [(1, 2)]*n),
    ("every_level_v31", dict(amg_full_levels=0, amg_coarse_pre=3, amg_coarse_post=1, amg_tail_post=1), None, lambda n: [(3, 1)]*n),
    # (below 1025 cells mid_skip must change nothing)
    ("one_full_level_mid_skip", dict(amg_full_levels=1, amg_mid_skip=True), None, lambda n: [(2, 2)] + [(0, 2)]*(n - 1)),
    ("one_full_level_no_mid_skip", dict(amg_full_levels=1, amg_mid_skip=False), None, lambda n: [(2, 2)] + [(0, 2)]*(n - 1)),
    ("tail_post_3_coarse_post_1", dict(amg_full_levels=1, amg_coarse_pre=1, amg_coarse_post=1, amg_tail_post=3), None,
     lambda n: [(2, 2)] + [(1, 3)]*(n - 1)),
    ("truncated_at_0", dict(), 0, lambda n: [(2, 2)]*3 + [(0, 2)]*(n - 3)),
    ("truncated_at_1", dict(), 1, lambda n: [(2, 2)]*3 + [(0, 2)]*(n - 3)),
    ("truncated_at_2", dict(amg_nu=3), 2, lambda n: [(3, 3)]*3 + [(0, 2)]*(n - 3)),
]


@pytest.mark.parametrize("which", [0, 1], ids=["pressure", "schur"])
@pytest.mark.parametrize("sid,amg_opts,trunc,expect", DENSE_SHAPES, ids=[s[0] for s in DENSE_SHAPES])
def test_vcycle_is_the_composed_matrix(sid, amg_opts, trunc, expect, which):
    amg = small_amg(which, **amg_opts)
    T = levels_of(amg)
    assert len(T) == 5 and [lv[0] for lv in T][:2] == [336, 168] and T[-2][0] > MIN_CELLS >= T[-1][0], T
    assert shapes(T) == expect(len(T) - 1), (sid, T)
    assert amg.trunc is None
    amg.trunc = trunc
    M = cycle_matrix(amg, T)
    shape = amg.levels[0].shape[1:]
    n = M.shape[0]
    V = np.zeros((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        V[:, j] = amg.vcycle(e.reshape(shape)).reshape(-1)
    d = float(np.abs(V - M).max()/np.abs(M).max())
    print("%s, hierarchy %d: SemiAMG.vcycle against the composed matrix, largest difference / largest entry %.3e" % (sid, which, d))
    assert d < 1e-12, (sid, which, d)
    if trunc is not None and which == 0:
        # the forced level really ended the cycle: another matrix than the untruncated one (on the pressure operator, where the
        # coarse-grid correction matters; S~ is dominated by its diagonal and loses next to nothing)
        amg.trunc = None
        M0 = cycle_matrix(amg, T)
        assert np.abs(M0 - M).max()/np.abs(M0).max() > 1e-3


@pytest.mark.parametrize("which", [0, 1], ids=["pressure", "schur"])
def test_dense_pieces_are_the_oracles_own(which):
    """to_csr orders the cells as the vectors are laid out, P is SemiAMG.prolong, P^T is SemiAMG.restrict: per level."""
    amg = small_amg(which)
    rng = np.random.default_rng(3)
    for l, A in enumerate(amg.levels):
        v = rng.standard_normal(A.shape[1:])
        Ad = la.to_csr(A[:, None, None]).toarray()
        assert rel2(Ad @ v.ravel(), la.spmv_scalar(A, v).ravel()) < 1e-14
        if l < len(amg.levels) - 1:
            P = prolongation(A, amg.sched[l])
            vc = rng.standard_normal(amg.levels[l + 1].shape[1:])
            assert rel2(P @ vc.ravel(), amg.prolong(vc, l, v.shape).ravel()) < 1e-15
            assert rel2(P.T @ v.ravel(), amg.restrict(v, l).ravel()) < 1e-14


# the rules for levels of more than 1024 cells, on the 15 x 25 x 21 box: pressure 7875(2) 4095(2) 2205(0) 1155(1) | 616(2) 352(0)
# 192(1) 96(2) 48, written out by hand from the statement of the options
BIG_RULES = [
    ("default", dict(),
     [(2, 2)]*3 + [(0, 1)] + [(0, 2)]*4),                   # three full levels; 1155: first mid level, smoothed; tail_post below
    ("no_full_levels", dict(amg_full_levels=0),
     [(0, 1), (0, 0), (0, 1), (0, 0)] + [(0, 2)]*4),        # every second mid level is a pure transfer level
    ("one_full_level", dict(amg_full_levels=1),
     [(2, 2), (0, 1), (0, 0), (0, 1)] + [(0, 2)]*4),        # the alternation counts from the first mid level
    ("no_mid_skip_v12_tail_3", dict(amg_full_levels=0, amg_mid_skip=False, amg_coarse_pre=1, amg_coarse_post=2, amg_tail_post=3),
     [(1, 2)]*4 + [(1, 3)]*4),                              # coarse_post above 1024 cells, tail_post at and below
    ("all_full", dict(amg_full_levels=99, amg_nu=3, amg_coarse_pre=1, amg_coarse_post=1, amg_tail_post=1),
     [(3, 3)]*8),                                           # full levels ignore every other shape option, whatever their size
    ("two_full_levels_mid_skip", dict(amg_full_levels=2, amg_coarse_pre=2, amg_coarse_post=3, amg_tail_post=1),
     [(2, 2)]*2 + [(2, 3), (0, 0)] + [(2, 1)]*4),
]


@pytest.mark.parametrize("rid,amg_opts,expect", BIG_RULES, ids=[r[0] for r in BIG_RULES])
def test_shape_rules_above_1024_cells(rid, amg_opts, expect):
    builder, kw, opts, P, _ = G.TABLES["B15"]
    c = G.case(rid, builder, kw, dict(opts, **amg_opts), None)
    o = G.oracle_engine(c)[0]
    T = levels_of(o.pc.amg_p)
    assert layout(T) == P
    assert shapes(T) == expect, (rid, T)


# ---------------------------------------------------------------- (b) the case table of tests/test_gpu_scalar_amg.py
@pytest.mark.parametrize("name", sorted(G.TABLES))
def test_level_tables_of_the_boxes(name):
    builder, kw, opts, P, S = G.TABLES[name]
    o = G.oracle_engine(G.case(name, builder, kw, opts, None))[0]
    assert layout(levels_of(o.pc.amg_p)) == P
    assert layout(levels_of(o.pc.amg_T)) == S


def ratios(amg, opts):
    """Dominance ratio of every level truncation is decided on: the first min(full_levels, levels - 1, 8)."""
    n = min(amg.full_levels, len(amg.levels) - 1, 8)
    return [float((np.abs(A[1:]).sum(axis=0)/np.abs(A[0])).max()) for A in amg.levels[:n]]


def one_ulp(rng, a):
    return a*(1.0 + rng.integers(-1, 2, size=a.shape)*2.0**-52)


@pytest.mark.parametrize("cid", [c.id for c in G.CASES])
def test_case_conditions(cid):
    c = G.CASE[cid]
    o, spec, u0, u, J, Sm = G.oracle_engine(c)
    amgs = (o.pc.amg_p, o.pc.amg_T)
    P, S = (levels_of(a) for a in amgs)
    # path predicate
    assert c.path(P, S), (cid, P, S)
    # coarsest size, box size
    assert P[-1][0] <= 200 and S[-1][0] <= 200 and P[0][0] <= 9360
    # truncation level and margin
    tau = c.opts["amg_dom_tau"]
    trunc = tuple(G.trunc_of(a) for a in amgs)
    assert trunc == c.trunc, (cid, trunc)
    if tau > 0.0:
        for a in amgs:
            r = ratios(a, c.opts)
            print("%s: dominance ratios %s against tau = %g" % (cid, ["%.4f" % v for v in r], tau))
            assert all(abs(v - tau) >= 0.1*tau for v in r), (cid, r, tau)
        assert all(v > 0.9 for v in ratios(amgs[0], c.opts))          # the pressure operator: ratio 1, never truncated
    else:
        assert trunc == (-1, -1)
    # the tail facts the GPU test will ask for, where the table pins them by hand
    for vid, env in G.variants_of(c):
        for w, T in enumerate((P, S)):
            lt, dense, napply, nlaunch = G.tail_facts(T, c.opts, env, trunc[w])
            if (cid, vid, w) in G.PINNED:
                assert (lt, dense) == G.PINNED[(cid, vid, w)], (cid, vid, w, lt, dense)
            assert napply + nlaunch == (0 if 0 <= trunc[w] < lt else 1)
    # sensitivity: the oracle under a one-ulp perturbation of its inputs, against a tenth of the GPU tolerance
    x = np.random.default_rng(11).standard_normal(u.shape)
    base = G.oracle_four(o, x)
    rng = np.random.default_rng(7)
    o.pc.setup(one_ulp(rng, J), one_ulp(rng, Sm))
    assert tuple(G.trunc_of(a) for a in amgs) == trunc
    pert = G.oracle_four(o, one_ulp(rng, x))
    d = {k: rel2(pert[k], base[k]) for k in G.KEYS}
    print("%s: one-ulp sensitivity of the oracle: %s" % (cid, {k: "%.2e" % v for k, v in d.items()}))
    tol = G.TOL_SINGLE if c.opts.get("amg_single") else G.TOL
    assert max(d.values()) <= 0.1*tol, (cid, d)


def test_the_pinned_facts_name_real_runs():
    runs = {(c.id, vid) for c in G.CASES for vid, _ in G.variants_of(c)}
    assert all((cid, vid) in runs and w in (0, 1) for cid, vid, w in G.PINNED)
