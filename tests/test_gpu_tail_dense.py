"""The AMG tail (the levels of <= 1024 cells) applied as ONE precomputed dense operator T per set-up (TP_AMG_TAIL_DENSE,
DESIGN.md 4.5) against the multilevel tail kernel it replaces and against the oracle, which evaluates the tail level by level.

T b is another evaluation order of the same linear map, so the bound is the project's stage tolerance, rel <= 1e-10 in the
2-norm; whole solves: Krylov counts within +-1 of each other, solutions rel <= 1e-8.  The switch is read at every set-up, so
both forms run in one process."""

import numpy as np
import pytest

import cases
from switches import setup_env

pytestmark = pytest.mark.gpu

TOL = 1e-10


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def engines(builder, kw, opts, dt=8640.0, seed=5, amp=0.3):
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = builder(**kw)
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    set_operator(o, h, spec, u0, dt, seed, amp)
    return spec, u0, o, h


def set_operator(o, h, spec, u0, dt, seed, amp):
    """Both engines at the seeded state; the Jacobian assembled on the GPU, assembled and set up in the oracle."""
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    for e in (o, h):
        e.set_old(u0)
        e.set_dt(dt)
        e.set_state(u)
    schur = o.opts["pc"] in ("cptr", "fieldsplit_cd")
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    h.jacobian()
    o.pc.setup(J, Sm)
    return u


def vcycle(h, which, dense):
    """Set up with the switch at `dense`, one V-cycle of hierarchy `which` on vector x -> result, tail info."""
    with setup_env(TP_AMG_TAIL_DENSE="1" if dense else "0"):
        h.pc_setup()
    h.amg_vcycle(which, "x", which, "y", which)
    return h.vec_get("y")[which].copy(), h.amg_tail_info(which)


VCYCLE = [
    # 9360 -> ... -> 585 | 293 | 147 | 74 | 37: a tail of five levels below four big ones
    ("box3d_deep_tail", cases.c4_spe10_3d, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr"), 4),
    # the 60 x 220 layer of C2/C3: 13200 -> ... -> 825 | 413 | ...; its tail vectors (three planes per level) do not fit the LDS
    ("layer2d_60x220", cases.c3_spe10_2d, dict(Nx=60, Ny=220, nphase=2), dict(pc="cptr"), 2),
    # 819 cells: the whole cycle is the tail (tail_level == 0); no truncation levels, so T is exact there
    ("tail_is_level0", cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", amg_dom_tau=0.0), 2),
    ("box3d_fp32_operators", cases.c4_spe10_3d, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_single=True), 4),
]


@pytest.mark.parametrize("name,builder,kw,opts,min_tail", VCYCLE, ids=[c[0] for c in VCYCLE])
def test_dense_tail_against_multilevel_and_oracle(name, builder, kw, opts, min_tail):
    spec, u0, o, h = engines(builder, kw, opts)
    x = np.random.default_rng(11).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    yd, info_d = vcycle(h, 0, True)
    ym, info_m = vcycle(h, 0, False)
    nlev = h.amg_info(0)[0]
    assert info_d["dense"] and not info_m["dense"], (info_d, info_m)
    assert nlev - info_d["tail_level"] >= min_tail and info_d["n"] <= 1024, (nlev, info_d)
    if name == "tail_is_level0":
        assert info_d["tail_level"] == 0
    assert info_d["builds"] == 1 and info_d["dense_applies"] == 1 and info_d["tail_launches"] == 0, info_d
    assert info_m["builds"] == 1 and info_m["tail_launches"] == 1, info_m
    yo = o.pc.amg_p.vcycle(x[0])
    d_dm, d_do, d_mo = rel2(yd, ym), rel2(yd, yo), rel2(ym, yo)
    print("%s: dense vs multilevel %.3e, dense vs oracle %.3e, multilevel vs oracle %.3e" % (name, d_dm, d_do, d_mo))
    assert d_dm <= TOL, (name, d_dm)
    assert d_do <= TOL, (name, d_do, d_mo)
    h.close()


@pytest.mark.parametrize("name,builder,kw,opts,min_tail", [VCYCLE[0], VCYCLE[2]], ids=[VCYCLE[0][0], VCYCLE[2][0]])
def test_no_stale_operator(name, builder, kw, opts, min_tail):
    """A second set-up on another operator re-forms T: the cycle matches the multilevel tail on the NEW operator and is far
    from the first one's result.  Where the tail is the whole cycle (tail_is_level0), y1 IS what the first T would give, so
    that case checks the statement exactly; on the box y1 also carries the old upper levels, so it is the weaker check there
    (the formed-operator counter and the agreement with the multilevel tail on the new operator carry it)."""
    spec, u0, o, h = engines(builder, kw, opts)
    x = np.random.default_rng(12).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    y1, info1 = vcycle(h, 0, True)
    set_operator(o, h, spec, u0, dt=86400.0, seed=9, amp=0.2)
    y2, info2 = vcycle(h, 0, True)
    y2m, _ = vcycle(h, 0, False)
    assert info1["builds"] == 1 and info2["builds"] == 2 and info2["dense"], (info1, info2)
    d_new, d_old = rel2(y2, y2m), rel2(y2, y1)
    print("%s: second set-up, dense vs multilevel %.3e; against the first operator's result %.3e" % (name, d_new, d_old))
    assert d_new <= TOL, d_new
    assert rel2(y2, o.pc.amg_p.vcycle(x[0])) <= TOL
    assert d_old > 1e-3, d_old
    h.close()


def test_truncated_above_the_tail_forms_no_operator():
    """At a small dt the temperature hierarchy ends on level 0 with relaxation only: its cycles never reach the tail and no T
    is formed for it, set-up after set-up; once the operator stops being dominant (huge dt) the next cycle needs the tail
    and T is formed on the way there (amg_resolve_trunc)."""
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr"), dt=86.4, amp=0.05)
    x = np.random.default_rng(13).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    for _ in range(2):
        yd, info = vcycle(h, 1, True)
        assert h.amg_trunc(1)[0] == 0
        assert info["builds"] == 0 and info["dense_applies"] == 0 and info["tail_launches"] == 0, info
    assert h.amg_tail_info(0)["builds"] == 2          # the pressure hierarchy is never truncated
    ym, _ = vcycle(h, 1, False)
    assert rel2(yd, ym) <= TOL
    assert rel2(yd, o.pc.amg_T.vcycle(x[1])) <= TOL
    # the same hierarchy, no longer dominant: the last resolved shape was truncated, so the set-up forms nothing ...
    set_operator(o, h, spec, u0, dt=4.0e6, seed=5, amp=0.05)
    yd, info = vcycle(h, 1, True)
    assert h.amg_trunc(1)[0] == -1
    assert info["dense"] and info["builds"] == 1 and info["dense_applies"] == 1, info      # ... and the first cycle does
    ym, info_m = vcycle(h, 1, False)
    assert info_m["tail_launches"] == 1
    d = rel2(yd, ym)
    print("formed on the way to the first cycle: dense vs multilevel %.3e" % d)
    assert d <= TOL, d
    # and from now on in the set-up
    yd2, info = vcycle(h, 1, True)
    assert info["builds"] == 2 and rel2(yd2, ym) <= TOL
    h.close()


def test_truncation_inside_the_tail_keeps_the_multilevel_kernel():
    """819 cells: tail_level = 0 lies among the levels relaxation-only truncation is decided on, so the tail may end early
    (the temperature hierarchy does, on level 0) and T would not be the cycle: the multilevel kernel stays, with either
    setting of the switch."""
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr"), dt=86.4, amp=0.05)
    x = np.random.default_rng(14).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    for which, orc in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        yd, info = vcycle(h, which, True)
        assert not info["dense"] and info["tail_level"] == 0 and info["builds"] == 0 and info["dense_applies"] == 0, info
        assert info["tail_launches"] >= 1
        ym, _ = vcycle(h, which, False)
        assert rel2(yd, ym) <= TOL
        assert rel2(yd, orc.vcycle(x[which])) <= TOL
    assert h.amg_trunc(1)[0] == 0 and h.amg_trunc(0)[0] == -1
    h.close()


SOLVES = [
    ("c4_like", cases.c4_spe10_3d, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr")),
    ("c3_like", cases.c3_spe10_2d, dict(Nx=60, Ny=220, nphase=2), dict(pc="cptr")),
]


@pytest.mark.parametrize("name,builder,kw,opts", SOLVES, ids=[c[0] for c in SOLVES])
def test_whole_solves_with_both_tails(name, builder, kw, opts):
    spec, u0, o, h = engines(builder, kw, opts)
    h.residual()
    h.copy_residual_to("b")
    res = {}
    for dense in (True, False):
        with setup_env(TP_AMG_TAIL_DENSE="1" if dense else "0"):
            h.pc_setup()
        its, reason, rn = h.fgmres("b", "d")
        assert reason > 0, (name, dense, reason)
        assert h.amg_tail_info(0)["dense"] == dense
        res[dense] = (its, h.vec_get("d").copy())
    d = rel2(res[True][1], res[False][1])
    print("%s: FGMRES iterations dense %d, multilevel %d; solutions differ by %.3e" % (name, res[True][0], res[False][0], d))
    assert abs(res[True][0] - res[False][0]) <= 1, (res[True][0], res[False][0])
    assert d <= 1e-8, d
    h.close()


def test_captured_pc_apply_sees_the_new_operator():
    """pc_apply is captured into a graph per vector pair and REPLAYED after the next set-up: T is rewritten in place (same
    address), so the replay applies the new operator."""
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr"))
    x = np.random.default_rng(15).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    with setup_env(TP_AMG_TAIL_DENSE="1"):
        h.pc_setup()
        h.pc_apply("x", "y")                 # captured
        h.pc_apply("x", "y")                 # replayed
        y1 = h.vec_get("y").copy()
        captured = h.amg_tail_info(0)["dense_applies"]
        assert captured >= 1
        set_operator(o, h, spec, u0, dt=86400.0, seed=9, amp=0.2)
        h.pc_setup()
        h.pc_apply("x", "y")
        y2 = h.vec_get("y").copy()
        info = h.amg_tail_info(0)
    assert info["dense"] and info["builds"] == 2 and info["dense_applies"] == captured, info      # no new capture: a replay
    with setup_env(TP_AMG_TAIL_DENSE="0"):
        h.pc_setup()
        h.pc_apply("x", "y")
    y2m = h.vec_get("y").copy()
    d_new, d_old = rel2(y2, y2m), rel2(y2, y1)
    print("replayed graph after the second set-up: dense vs multilevel %.3e; against the first result %.3e" % (d_new, d_old))
    assert d_new <= TOL, d_new
    assert rel2(y2, o.pc.apply(x)) <= TOL
    assert d_old > 1e-3, d_old
    h.close()
