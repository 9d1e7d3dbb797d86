"""Coarse correction + first post-sweep of the top AMG levels in one tiled launch (k_amg_prolong_jacobi_tile)
against the two launches k_amg_prolong_add -> k_amg_jacobi that TP_AMG_PJ_FUSE=0 keeps: the corrected iterate is the same
prolong_added, the sweep the same jacobi_update on the same operands in the same order, so every comparison between the two forms
is BITWISE (uint64 view).  The default form is also held against the numpy oracle's V-cycle at the AMG tests' bound (rel <= 1e-10
in the 2-norm), so that the two forms cannot be wrong together.

The switches are read once per process: tests/pj_fuse_env_check.py runs every case in one child process per setting, once for
the whole module, the children side by side.  Settings: the default, TP_AMG_PJ_FUSE=0, and both again with TP_AMG_INVD_LOAD=1.
Each case asserts from tp_amg_layout that its V(nu,nu) levels coarsen the axes and extents it claims.

Measured on MI355X, default form against the oracle (each test prints its figures): V-cycles 8.5e-17 ... 5.3e-13, the whole
pc_apply 1.7e-12 and 7.6e-16 (amg_nu = 1), two slabs 5.0e-16."""
import numpy as np
import pytest

import pj_fuse_env_check as K
from switches import run_children

pytestmark = pytest.mark.gpu

TOL = 1e-10
RUN = 256               # cells of a run: TP_BLOCK
SETTINGS = {"tile": {}, "two_launches": {"TP_AMG_PJ_FUSE": "0"},
            "tile_invd_load": {"TP_AMG_INVD_LOAD": "1"}, "two_launches_invd_load": {"TP_AMG_PJ_FUSE": "0", "TP_AMG_INVD_LOAD": "1"}}

# name -> per hierarchy (0 pressure, 1 S~): (coarsening axis, the level's extents) of the levels with pre-sweeps, from level 0 on
LEVELS = {
    "ax1_90x27x37": {0: [(1, (37, 27, 90)), (0, (37, 14, 90)), (1, (19, 14, 90))], 1: [(0, (37, 27, 90)), (0, (19, 27, 90)), (0, (10, 27, 90))]},
    "ax2_6x37x5": {0: [(2, (5, 6, 37)), (2, (5, 6, 19)), (1, (5, 6, 10))], 1: [(0, (5, 6, 37)), (0, (3, 6, 37)), (0, (2, 6, 37))]},
    "ax2_5x6x37": {0: [(2, (37, 5, 6)), (2, (37, 5, 3)), (1, (37, 5, 2))], 1: [(0, (37, 5, 6)), (0, (19, 5, 6)), (0, (10, 5, 6))]},
    "ax1_37x6x5": {0: [(1, (5, 6, 37)), (0, (5, 3, 37)), (1, (3, 3, 37))], 1: [(0, (5, 6, 37)), (0, (3, 6, 37)), (0, (2, 6, 37))]},
    "odd_13x11x9": {0: [(1, (9, 11, 13)), (0, (9, 6, 13)), (1, (5, 6, 13))], 1: [(0, (9, 11, 13)), (0, (5, 11, 13)), (0, (3, 11, 13))]},
    "fp32_operators": {0: [(2, (18, 20, 26)), (2, (18, 20, 13)), (1, (18, 20, 7))], 1: [(0, (18, 20, 26)), (0, (9, 20, 26)), (0, (5, 20, 26))]},
    "nu1": {0: [(2, (18, 20, 26)), (2, (18, 20, 13)), (1, (18, 20, 7))], 1: [(0, (18, 20, 26)), (0, (9, 20, 26)), (0, (5, 20, 26))]},
    "wide_130": {0: [(2, (130, 5, 6)), (0, (130, 5, 3)), (2, (65, 5, 3))], 1: [(0, (130, 5, 6)), (0, (65, 5, 6)), (0, (33, 5, 6))]},
    "wide_128": {0: [(2, (128, 5, 6)), (0, (128, 5, 3)), (2, (64, 5, 3))], 1: [(0, (128, 5, 6)), (0, (64, 5, 6)), (0, (32, 5, 6))]},
    "thin_2x37x2": {0: [(2, (2, 2, 37)), (1, (2, 2, 19)), (2, (2, 1, 19))], 1: [(0, (2, 2, 37)), (2, (1, 2, 37)), (1, (1, 2, 19))]},
    "thin_2x2x37": {0: [(2, (37, 2, 2)), (0, (37, 2, 1)), (1, (19, 2, 1))], 1: [(0, (37, 2, 2)), (0, (19, 2, 2)), (0, (10, 2, 2))]},
    "thin_37x2x2": {0: [(1, (2, 2, 37)), (2, (2, 1, 37)), (0, (2, 1, 19))], 1: [(0, (2, 2, 37)), (1, (1, 2, 37)), (2, (1, 1, 37))]},
}
# cycles that end above the tail (amg_dom_tau's default): per hierarchy the level that is relaxed only; the levels above it are fused
TRUNC = {"thin_2x37x2": (-1, 2)}
# Gauss-Seidel and line levels 0 and 1 keep their sequences; level 2 (axis 1, 18 x 20 x 7) is a Jacobi level and takes the tiled launch
SEQUENCES = ("gs_levels", "line_levels")


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return run_children("pj_fuse_env_check.py", SETTINGS, tmp_path_factory.mktemp("pj_fuse"), timeout=600)         # the children side by side


def oracle_of(name, kw, opts, dt=K.DT, amp=K.AMP):
    """The numpy oracle at the child's state, set up: (engine, x)."""
    if "amg_gs_levels" in opts:
        from amg_gs_ref import oracle_engine
    elif "amg_line_levels" in opts:
        from amg_line_ref import oracle_engine
    else:
        from oracle.engine import OracleEngine as oracle_engine
    spec, u0, u, x = K.inputs(kw, amp)
    o = oracle_engine(spec, opts)
    o.set_old(u0)
    o.set_dt(dt)
    o.set_state(u)
    J, Sm = o.jacobian(want_schur=True)
    o.pc.setup(J, Sm)
    return o, x


def check_forms(runs, key):
    """The default form's vector, equal bit for bit in every setting."""
    a = runs["tile"][key]
    assert np.isfinite(a).all() and np.abs(a).max() > 0, key
    for other in SETTINGS:
        assert same_bits(a, runs[other][key]), (key, other)
    return a


def levels_of(n, sched):
    """(axis, extents) of every level of a schedule on the box n."""
    n, out = list(n), []
    for a in sched:
        out.append((a, tuple(n)))
        n[a] = (n[a] + 1)//2
    return out


def check_cycles(runs, case, o, x, levels=None):
    for which, ref in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        lay = runs["tile"]["%s_layout%d" % (case, which)]
        assert lay[0] == 0 and list(lay[1:]) == list(ref.sched)
        if levels is not None:
            assert levels_of(ref.n, ref.sched)[:3] == levels[which], levels_of(ref.n, ref.sched)[:3]
        y = check_forms(runs, "%s_v%d" % (case, which))
        d = rel2(y, ref.vcycle(x[which]))
        print("%s hierarchy %d: tiled V-cycle vs oracle %.3e" % (case, which, d))
        assert d <= TOL, (case, which, d)


@pytest.mark.parametrize("case", list(LEVELS))
def test_vcycles(runs, case):
    """Pressure and S~ V-cycles: tiled launch = two launches, with either form of the inverse diagonal, bit for bit;
    the tiled launch against the oracle.  The levels with pre-sweeps coarsen the axes and have the extents the case is there for."""
    kw, opts, env, whole = K.CASES[case]
    o, x = oracle_of(case, kw, opts)
    print("%s: truncation levels %s" % (case, tuple(int(t) for t in runs["tile"][case + "_trunc"])))
    assert tuple(runs["tile"][case + "_trunc"]) == TRUNC.get(case, (-1, -1))        # (-1: a full cycle, every level corrected from below)
    check_cycles(runs, case, o, x, LEVELS[case])
    if whole:
        z = check_forms(runs, case + "_pc")
        d = rel2(z, o.pc.apply(x))
        print("%s: pc_apply vs oracle %.3e" % (case, d))
        assert d <= TOL, (case, d)


def test_every_axis_and_edge_is_covered():
    """Over the cases' fused levels: each coarsening axis with odd and even extents and extents of 2 and 3; planes of less than one
    run, of several runs and of no whole number of runs; lines of 37 cells, of one cell, of half a run (the halo fills its slots) and
    of more (several halo cells per thread); levels of one, two and many planes; the thinnest levels along each axis that is not
    coarsened."""
    lv = [(a, n) for case, per in LEVELS.items() for which, hier in per.items()
          for l, (a, n) in enumerate(hier) if not 0 <= TRUNC.get(case, (-1, -1))[which] <= l]
    for a in (0, 1, 2):
        assert {n[a] & 1 for b, n in lv if b == a} == {0, 1}, a
        assert {n[a] for b, n in lv if b == a} >= {2, 3}, a
        for other in {0, 1, 2} - {a}:                               # one cell wide along an axis the level does not coarsen
            assert any(b == a and n[other] == 1 for b, n in lv), (a, other)
    planes = {n[0]*n[1] for a, n in lv}
    assert min(planes) < RUN and any(p >= 2*RUN and p % RUN for p in planes), planes
    lines = {n[0] for a, n in lv}
    assert {1, 37} <= lines and any(2*n0 > RUN for n0 in lines) and any(2*n0 == RUN for n0 in lines), lines
    depth = {n[2] for a, n in lv}
    assert {1, 2, 3} <= depth and max(depth) >= 37, depth
    assert K.CASES["nu1"][1]["amg_nu"] == 1 and K.CASES["fp32_operators"][1]["amg_single"] is True
    assert all("amg_nu" not in K.CASES[c][1] for c in LEVELS if c != "nu1")          # the default of two sweeps everywhere else


@pytest.mark.parametrize("case", SEQUENCES)
def test_gs_and_line_levels_keep_their_sequences(runs, case):
    """amg_gs_levels = 2, amg_line_levels = 2: levels 0 and 1 run x += P ec and their own sweeps, whatever the switch says."""
    kw, opts, env, whole = K.CASES[case]
    o, x = oracle_of(case, kw, opts)
    assert tuple(runs["tile"][case + "_trunc"]) == (-1, -1)
    check_cycles(runs, case, o, x)


def test_truncated_cycles_are_unchanged(runs):
    """amg_dom_tau = 1e6: both cycles end at level 0 with relaxation only -- no correction, nothing to fuse."""
    case = "truncated"
    assert tuple(runs["tile"][case + "_trunc"]) == (0, 0)
    kw, opts, env, whole = K.CASES[case]
    o, x = oracle_of(case, kw, opts)
    check_cycles(runs, case, o, x)


def test_two_slabs(runs):
    """Two slabs, amg_gather_cells = 0: every level with two planes per slab is distributed and keeps the two launches around the
    corrected iterate's halo exchange."""
    name, kw, opts, env, dt, amp = K.SLABS
    assert opts["amg_gather_cells"] == 0
    lay = runs["tile"][name + "_layout0"]
    nd, axes = int(lay[0]), list(lay[1:])
    assert nd >= 2 and axes[0] == 2 and axes[1] == 0, (nd, axes)
    y = check_forms(runs, name + "_v0")
    o, x = oracle_of(name, kw, {k: v for k, v in opts.items() if k != "amg_gather_cells"}, dt, amp)
    assert axes == list(o.pc.amg_p.sched)
    d = rel2(y, o.pc.amg_p.vcycle(x[0]))
    print("%s: pressure V-cycle vs the one-slab oracle %.3e" % (name, d))
    assert d <= TOL, d
