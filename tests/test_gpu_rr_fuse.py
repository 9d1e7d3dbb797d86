"""Residual + restriction of the top AMG levels in one tiled launch (k_amg_resid_restrict_tile) against the two
launches k_amg_resid -> k_amg_restrict that TP_AMG_RR_FUSE=0 keeps: each fine residual is the same resid_at, the combination
is restrict_cell's with the same operands in the same order, so every comparison between the two forms is BITWISE.  The
default form is also held against the numpy oracle's V-cycle at the AMG tests' bound (rel <= 1e-10 in the 2-norm), so that the
two forms cannot be wrong together, and the same cases are held bitwise between TP_AMG_INVD_LOAD=1 and the default.

The switches are read once per process: tests/rr_fuse_env_check.py runs every case in one child process per setting, once for
the whole module.  Each case asserts from tp_amg_layout that its V(2,2) levels coarsen the axes it claims.

Measured on MI355X, default form against the oracle (each test prints its figures): V-cycles 8.5e-17 ... 1.8e-14, the whole
pc_apply 2.5e-14, two slabs 5.0e-16; fp32 operators 8.5e-17 and 1.2e-15 (the oracle rounds its stored operators to fp32 as well)."""
import numpy as np
import pytest

import cases
import rr_fuse_env_check as K
from switches import run_children

pytestmark = pytest.mark.gpu

TOL = 1e-10
SETTINGS = {"tile": {}, "two_launches": {"TP_AMG_RR_FUSE": "0"}, "invd_load": {"TP_AMG_INVD_LOAD": "1"}}

# name -> per hierarchy (0 pressure, 1 S~): (coarsening axis, fine extent along it) of the levels with pre-sweeps, from level 0 on
LEVELS = {
    "ax1_90x27x37": {0: [(1, 27), (0, 37), (1, 14)], 1: [(0, 37), (0, 19), (0, 10)]},
    "ax2_6x37x5": {0: [(2, 37), (2, 19), (1, 6)], 1: [(0, 5), (0, 3), (0, 2)]},
    "ax2_5x6x37": {0: [(2, 6), (2, 3), (1, 5)], 1: [(0, 37), (0, 19), (0, 10)]},
    "ax1_37x6x5": {0: [(1, 6), (0, 5), (1, 3)], 1: [(0, 5), (0, 3), (0, 2)]},
    "odd_13x11x9": {0: [(1, 11), (0, 9), (1, 6)], 1: [(0, 9), (0, 5), (0, 3)]},
    "fp32_operators": {0: [(2, 26), (2, 13), (1, 20)], 1: [(0, 18), (0, 9), (0, 5)]},
    "gs_levels": {0: [(2, 26), (2, 13), (1, 20)], 1: [(0, 18), (0, 9), (0, 5)]},
    "line_levels": {0: [(2, 26), (2, 13), (1, 20)], 1: [(0, 18), (0, 9), (0, 5)]},
}


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return run_children("rr_fuse_env_check.py", SETTINGS, tmp_path_factory.mktemp("rr_fuse"), timeout=600)         # the children side by side


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
    a = runs["tile"][key]
    assert np.isfinite(a).all() and np.abs(a).max() > 0, key
    assert same_bits(a, runs["two_launches"][key]), key
    assert same_bits(a, runs["invd_load"][key]), key
    return a


def extents(n, sched):
    """(axis, fine extent along it) of every level of a schedule on the box n."""
    n, out = list(n), []
    for a in sched:
        out.append((a, n[a]))
        n[a] = (n[a] + 1)//2
    return out


@pytest.mark.parametrize("case", list(LEVELS))
def test_vcycles(runs, case):
    """Pressure and S~ V-cycles: tiled launch = two launches = stored inverse diagonal, bit for bit; tiled launch against the
    oracle.  The V(2,2) levels coarsen the axes and extents the case is there for."""
    kw, opts, env, whole = K.CASES[case]
    o, x = oracle_of(case, kw, opts)
    assert tuple(runs["tile"][case + "_trunc"]) == (-1, -1)          # full cycles: every V(2,2) level restricts a residual
    for which, ref in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        lay = runs["tile"]["%s_layout%d" % (case, which)]
        assert lay[0] == 0 and list(lay[1:]) == list(ref.sched)
        assert extents(ref.n, ref.sched)[:3] == LEVELS[case][which], extents(ref.n, ref.sched)[:3]
        y = check_forms(runs, "%s_v%d" % (case, which))
        d = rel2(y, ref.vcycle(x[which]))
        print("%s hierarchy %d: tiled V-cycle vs oracle %.3e" % (case, which, d))
        assert d <= TOL, (case, which, d)
    if whole:
        z = check_forms(runs, case + "_pc")
        d = rel2(z, o.pc.apply(x))
        print("%s: pc_apply vs oracle %.3e" % (case, d))
        assert d <= TOL, (case, d)


def test_every_axis_and_edge_is_covered():
    """Over the cases: each axis on a V(2,2) level; along the coarsening axis odd and even extents and extents of 2 and 3, for
    the tiled axes (1, 2) and for axis 0; lines that are no multiple of a tile's run, levels of more than one tile each way."""
    seen = {(a, n) for per in LEVELS.values() for lv in per.values() for a, n in lv}
    for a in (0, 1, 2):
        assert {n & 1 for b, n in seen if b == a} == {0, 1}, a
        assert {n for b, n in seen if b == a} & {2, 3}, a
    assert (1, 27) in seen and (2, 37) in seen        # 14 and 19 coarse cells: more than the 12 or 7 one tile holds along the axis
    assert (0, 37) in seen                            # lines of 37 cells cut by runs of 254


def test_truncated_cycles_are_unchanged(runs):
    """amg_dom_tau = 1e6: both cycles end at level 0 with relaxation only -- no residual, nothing to fuse."""
    case = "truncated"
    assert tuple(runs["tile"][case + "_trunc"]) == (0, 0)
    kw, opts, env, whole = K.CASES[case]
    o, x = oracle_of(case, kw, opts)
    for which, ref in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        y = check_forms(runs, "%s_v%d" % (case, which))
        d = rel2(y, ref.vcycle(x[which]))
        print("%s hierarchy %d: V-cycle vs oracle %.3e" % (case, which, d))
        assert d <= TOL, (which, d)


def test_two_slabs(runs):
    """Two slabs, every level distributed: level 0 coarsens the slab axis and keeps the two launches around the residual's halo
    exchange, level 1 (axis 0) is distributed too and takes the tiled launch on each slab's owned cells."""
    name, kw, opts, env, dt, amp = K.SLABS
    lay = runs["tile"][name + "_layout0"]
    nd, axes = int(lay[0]), list(lay[1:])
    assert nd >= 2 and axes[0] == 2 and axes[1] == 0, (nd, axes)
    y = check_forms(runs, name + "_v0")
    o, x = oracle_of(name, kw, {k: v for k, v in opts.items() if k != "amg_gather_cells"}, dt, amp)
    assert axes == list(o.pc.amg_p.sched)
    d = rel2(y, o.pc.amg_p.vcycle(x[0]))
    print("%s: pressure V-cycle vs the one-slab oracle %.3e" % (name, d))
    assert d <= TOL, d
