"""The opt-in Eisenstat-Walker inexact Newton on the GPU (tp_options.ksp_ew) against the numpy reference tests/ew_ref.py, which runs
the same chooser on the oracle's residual, Jacobian and linear solve.

Inputs (tests/ew_ref.py): the eight-step ramp on c4_spe10_3d(8, 10, 6) pc_cptr; the first two ramp steps on c3_spe10_2d(12, 16)
pc_cptr (one plane; eta rises above rtol0 once); a single-phase pc_cpr box; for `bt` input A of newton_ls_ref at snes_rtol 1e-10.

State tolerance: not fixed by hand.  On the CPU the reference runs the ramp three times per version -- fixed tolerance, Eisenstat-
Walker, and Eisenstat-Walker with every eta halved: three legitimate solves of the same nonlinear problems.  The larger final-
state difference per field is the floor (ew_ref.FLOOR1: p 6.4e-11, T 1.2e-13 in the relative 2-norm, S_o 7.3e-10 max abs), and the
GPU, whose Krylov solves differ from the oracle's by the summation order and +-1 iteration, gets 10 x the floor
(ew_ref.PARITY_TOL; profiles/ew_parity.txt; tests/test_ew_host.py re-measures it).  The eta of the run's own record are recomputed
with the reference's chooser to 1e-14 relative: the same libm pow on the same recorded numbers."""
import ctypes as C
import threading

import numpy as np
import pytest

import cases
import ew_ref as R
import newton_ls_ref as L
import switches

pytestmark = pytest.mark.gpu

_REF, _GPU = {}, {}
KSP_RTOL = R.RAMP_OPTS["ksp_rtol"]
KSP_ATOL = 1e-50


def box_case():
    return cases.c4_spe10_3d(7, 13, 9, nphase=1)


# name -> (case builder, engine options, time steps in days)
INPUTS = {"ramp": (R.ramp_case, R.RAMP_OPTS, R.RAMP_DT), "c3": (R.c3_case, R.C3_OPTS, R.RAMP_DT[:2]),
          "box": (box_case, dict(pc="cpr", ksp_rtol=KSP_RTOL), (0.01, 0.02))}


def reference(name, version):
    """The reference on a named input, computed once and shared (never modified): (per-step results, final state)."""
    key = (name, version)
    if key not in _REF:
        case, opts, dts = INPUTS[name]
        _REF[key] = R.ref_ramp(version, case=case, opts=opts, dts=dts)
    return _REF[key]


def split_monitor(seen):
    """The monitor's (its, rnorm) stream cut into one residual list per linear solve (its restarts at 1)."""
    solves = []
    for its, rn in seen:
        if its == 1:
            solves.append([])
        solves[-1].append(rn)
    return solves


def run_gpu(name, opts, monitor=False, engine=None, keep=False, **kw):
    """The time steps of a named input on the GPU: dict(steps = per step the solve's info with its Eisenstat-Walker history under
    "ew" and, with monitor, the residuals per linear solve under "mon"; u = final state; info = ew_info at the end)."""
    from thermalporous_amd.engine import HipEngine
    case, base, dts = INPUTS[name]
    spec, u0, *_ = case()
    h = engine or HipEngine(spec, {**base, **opts}, **kw)
    seen = []
    if monitor:
        h.set_ksp_monitor(lambda its, rn, fn: seen.append((its, rn)))

    def solve(e):
        del seen[:]
        r = dict(e.newton_solve())
        r["ew"] = e.ew_history()
        r["mon"] = split_monitor(seen)
        return r
    steps = R.run_ramp(h, u0, dts, solve)
    out = dict(steps=steps, u=h.get_state(), info=h.ew_info())
    if monitor:
        h.set_ksp_monitor(None)
    if keep:
        out["engine"] = h
    else:
        h.close()
    return out


def gpu(name, **opts):
    """run_gpu without a monitor on a fresh engine, computed once per (input, options) and shared (never modified)."""
    key = (name, tuple(sorted(opts.items())))
    if key not in _GPU:
        _GPU[key] = run_gpu(name, opts)
    return _GPU[key]


def check_formula(steps, version, params=None, ksp_rtol=KSP_RTOL, tag=""):
    """Check 1: every recorded eta is what the reference's chooser gives from the recorded norms.  Returns how often the safeguard
    raised eta."""
    raised = 0
    for i, s in enumerate(steps):
        e = s["ew"]
        assert e["n"] == len(e["rtol"]) == len(e["kits"]) >= 1 and sum(e["kits"]) == s["lits"], (tag, i)
        assert e["fnorm"][0] == s["fnorm0"], (tag, i)
        for k in range(e["n"]):
            last = (e["fnorm"][k - 1], e["lresid"][k - 1], e["rtol"][k - 1]) if k else (0.0, 0.0, 0.0)
            want, fl = R.next_rtol(version, k, e["fnorm"][k], *last, ksp_rtol, **{**R.DEFAULTS, **(params or {})})
            assert abs(e["rtol"][k] - want) <= 1e-14*want, (tag, i, k, e["rtol"][k], want)
            raised += bool(fl & R.SAFE_RAISED)
    return raised


def check_honoured(steps, tag="", monitored=False):
    """Check 2: a converged solve ends at or below max(eta ||F||, ksp_atol), and (monitored) was above it one iteration before."""
    for i, s in enumerate(steps):
        e = s["ew"]
        if monitored:
            assert [len(m) for m in s["mon"]] == e["kits"], (tag, i)
        for k in range(e["n"]):
            tol = max(e["rtol"][k]*e["fnorm"][k], KSP_ATOL)
            if e["kreason"][k] > 0:
                assert e["lresid"][k] <= tol, (tag, i, k, e["lresid"][k], tol)
            if monitored and e["kits"][k] >= 2:
                assert s["mon"][k][-2] > tol, (tag, i, k, s["mon"][k], tol)


def check_state(u, uref, tag=""):
    d = R.state_diff(u, uref)
    print(tag, "state vs reference:", ["%.3e" % x for x in d], "tolerance", ["%.3e" % x for x in R.PARITY_TOL[:len(d)]])
    assert all(d[f] <= R.PARITY_TOL[f] for f in range(len(d))), (tag, d)


def describe(tag, steps):
    print(tag, "reasons", [s["reason"] for s in steps], "Newton", [s["nits"] for s in steps], "Krylov", [s["lits"] for s in steps])
    for s in steps:
        print(tag, "  eta", ["%.3g" % v for v in s["ew"]["rtol"]], "kits", s["ew"]["kits"])


def same_history(a, b):
    return all(x["ew"]["kits"] == y["ew"]["kits"] and x["ew"]["kreason"] == y["ew"]["kreason"] and
               all(np.array_equal(x["ew"][q], y["ew"][q]) for q in ("rtol", "fnorm", "lresid")) and
               (x["nits"], x["lits"], x["reason"], x["fnorm"]) == (y["nits"], y["lits"], y["reason"], y["fnorm"]) for x, y in zip(a, b)) \
        and len(a) == len(b)


# ---- 1, 2: the formula and the tolerance, from the run's own record ----------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("name", ["c3", "box", "ramp"])
def test_formula_and_tolerance_from_the_record(name, version):
    plain = gpu(name, ksp_ew=version)
    steps = plain["steps"]
    describe("%s v%d" % (name, version), steps)
    assert len(steps) == len(INPUTS[name][2]) and all(s["reason"] > 0 for s in steps)
    raised = check_formula(steps, version, tag=name)
    check_honoured(steps, tag=name)
    assert plain["info"] == dict(version=version, newton_solves=len(steps), linear_solves=sum(s["ew"]["n"] for s in steps), safeguarded=raised)
    assert raised >= 1 and all(s["ew_rtol"] == list(s["ew"]["rtol"]) for s in steps)
    # under the monitor (no pipelining, no speculative application) the same run, bit for bit, and no solve ran one iteration long
    mon = run_gpu(name, dict(ksp_ew=version), monitor=True)
    assert same_history(mon["steps"], steps) and np.array_equal(mon["u"], plain["u"])
    check_honoured(mon["steps"], tag=name + " monitored", monitored=True)
    for s in mon["steps"]:
        for k, m in enumerate(s["mon"]):
            assert m[-1] == s["ew"]["lresid"][k]


def test_recorded_norms_are_the_residual_history():
    """c3, first step: a solve cut off after j iterations ends with ||F_j||, which the full solve recorded for its linear solve j."""
    from thermalporous_amd.engine import HipEngine
    full = gpu("c3", ksp_ew=2)["steps"][0]
    case, base, dts = INPUTS["c3"]
    spec, u0, *_ = case()
    for j in range(1, full["nits"]):
        h = HipEngine(spec, {**base, "ksp_ew": 2, "snes_max_it": j})
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(dts[0]*R.DAY)
        r = h.newton_solve()
        assert (r["reason"], r["nits"]) == (-5, j) and r["fnorm"] == full["ew"]["fnorm"][j]
        assert np.array_equal(h.ew_history()["rtol"], full["ew"]["rtol"][:j])
        h.close()
    assert full["fnorm"] < full["ew"]["fnorm"][-1]


# ---- 3: the degenerate setting is the fixed solver, bitwise ------------------------------------------------------------------------
@pytest.mark.parametrize("ksp", ["fgmres", "bcgs"])
def test_degenerate_setting_is_the_fixed_solver_bitwise(ksp):
    fixed = gpu("ramp", ksp=ksp)
    assert all(s["reason"] > 0 and s["ew"]["n"] == 0 and "ew_rtol" not in s for s in fixed["steps"]) and len(fixed["steps"]) == len(R.RAMP_DT)
    assert fixed["info"] == dict(version=0, newton_solves=0, linear_solves=0, safeguarded=0)
    for version in (1, 2):
        deg = gpu("ramp", ksp=ksp, ksp_ew=version, ew_rtol0=KSP_RTOL, ew_rtolmax=KSP_RTOL)
        assert all(v == KSP_RTOL for s in deg["steps"] for v in s["ew"]["rtol"])
        assert [(s["nits"], s["lits"], s["reason"], s["fnorm"]) for s in deg["steps"]] == \
               [(s["nits"], s["lits"], s["reason"], s["fnorm"]) for s in fixed["steps"]]
        assert np.array_equal(deg["u"], fixed["u"])


def test_key_absent_after_an_ew_run_is_a_run_that_never_saw_it():
    fixed = gpu("ramp")
    first = run_gpu("ramp", dict(ksp_ew=2), keep=True)
    h = first["engine"]
    assert same_history(first["steps"], gpu("ramp", ksp_ew=2)["steps"])
    h.set_options(ksp_ew=False)
    again = run_gpu("ramp", {}, engine=h)                  # the same context, the key absent
    fresh = run_gpu("ramp", {})                            # a fresh context in a process that ran the option
    for run in (again, fresh):
        assert all(s["ew"]["n"] == 0 for s in run["steps"])
        assert [(s["nits"], s["lits"], s["reason"], s["fnorm"]) for s in run["steps"]] == \
               [(s["nits"], s["lits"], s["reason"], s["fnorm"]) for s in fixed["steps"]]
        assert np.array_equal(run["u"], fixed["u"])


# ---- 4: against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_ramp_against_the_reference(version):
    rsteps, uref = reference("ramp", version)
    run = gpu("ramp", ksp_ew=version)
    steps = run["steps"]
    describe("ramp v%d" % version, steps)
    print("reference Newton", [s["nits"] for s in rsteps], "Krylov", [s["lits"] for s in rsteps])
    assert [s["reason"] for s in steps] == [s["reason"] for s in rsteps] == [3]*len(R.RAMP_DT)
    assert all(abs(a["nits"] - b["nits"]) <= 1 for a, b in zip(steps, rsteps))
    check_state(run["u"], uref, "ramp v%d" % version)
    fixed = gpu("ramp")["steps"]
    kew, kfixed = sum(s["lits"] for s in steps), sum(s["lits"] for s in fixed)
    print("Krylov iterations: Eisenstat-Walker %d, fixed tolerance %d" % (kew, kfixed))
    assert kew < kfixed


# ---- 5: combinations ---------------------------------------------------------------------------------------------------------------
COMBOS = [("bcgs", dict(ksp="bcgs")), ("basis_single", dict(ksp_basis_single=True)), ("ISI", dict(pc_order="ISI")),
          ("s1_fgmres", dict(s1_ksp="fgmres", s1_max_it=4, s1_rtol=1e-2)), ("reorth", dict(ksp_reorth="always"))]


@pytest.mark.parametrize("tag,extra", COMBOS, ids=[c[0] for c in COMBOS])
def test_combinations(tag, extra):
    _, uref = reference("ramp", 2)
    run = run_gpu("ramp", dict(ksp_ew=2, **extra), monitor=True)
    steps = run["steps"]
    describe(tag, steps)
    assert len(steps) == len(R.RAMP_DT) and all(s["reason"] > 0 for s in steps)
    check_formula(steps, 2, tag=tag)
    check_honoured(steps, tag=tag, monitored=True)
    check_state(run["u"], uref, tag)


def test_combination_with_backtracking():
    """Input A of newton_ls_ref at snes_rtol 1e-10 (ew_ref.BT_OPTS): four shortened steps; after an accepted step ||F_k+1|| is the
    accepted trial's norm."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, eng = L.cold_engine("c3", R.BT_OPTS, R.BT_DT)
    ref = R.newton_ew_ref(eng, version=2, linesearch="bt")
    h = HipEngine(spec, {**R.BT_OPTS, "ksp_ew": 2, "linesearch": "bt"})
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(R.BT_DT*R.DAY)
    seen = []
    h.set_ksp_monitor(lambda its, rn, fn: seen.append((its, rn)))
    s = dict(h.newton_solve())
    s["ew"], s["mon"] = h.ew_history(), split_monitor(seen)
    ls = h.ls_history()
    describe("bt", [s])
    print("bt trials", ls["trials"], "reference", ref["trials"], "Newton", ref["nits"], "eta", ["%.3g" % v for v in ref["ew"]["rtol"]])
    # (the trial counts are printed, not compared: at eta up to 0.9 one Krylov iteration more or less is another Newton direction)
    assert s["reason"] == ref["reason"] == 3 and ref["trials"] == R.BT_EXPECT_TRIALS and max(ls["trials"]) > 1
    check_formula([s], 2, ksp_rtol=R.BT_OPTS["ksp_rtol"], tag="bt")
    check_honoured([s], tag="bt", monitored=True)
    assert np.array_equal(s["ew"]["fnorm"][1:], ls["fnorm"][:-1])          # the accepted trials' norms, bit for bit
    check_state(h.get_state(), ref["u"], "bt")
    h.close()


# ---- 6: two slabs ------------------------------------------------------------------------------------------------------------------
# Two slabs cut the grid's 10 planes at plane 5, and stage 2 is block-Jacobi over tiles that start at each slab's origin: with the
# default tiles (8 x 4 columns on two slabs, 4 x 8 on one) the two runs would have different preconditioners, and under Eisenstat-
# Walker another preconditioner is another sequence of eta (measured: Newton counts 4 4 4 4 4 4 4 4 against 4 4 4 4 5 5 4 5).  With
# 8 x 5 tiles both runs have the same two blocks, so they differ by the order of the slabs' sums only.
SLAB_TILE = (1 << 30, 8, 5)


def test_two_slabs():
    from thermalporous_amd import engine as E
    one = gpu("ramp", ksp_ew=2, ilu_tile=SLAB_TILE)
    lib = E.load_library()
    nslabs = 2
    group = C.c_void_p()
    assert lib.tp_local_group_create(nslabs, C.byref(group)) == 0
    out, err = [None]*nslabs, []

    def worker(rank):
        try:
            out[rank] = run_gpu("ramp", dict(ksp_ew=2, ilu_tile=SLAB_TILE), rank=rank, nranks=nslabs, local_group=group)
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nslabs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    describe("two slabs", out[0]["steps"])
    assert same_history(out[0]["steps"], out[1]["steps"]) and out[0]["info"] == out[1]["info"]
    assert [s["nits"] for s in out[0]["steps"]] == [s["nits"] for s in one["steps"]]
    assert all(s["reason"] > 0 for s in out[0]["steps"])
    check_formula(out[0]["steps"], 2, tag="two slabs")
    check_honoured(out[0]["steps"], tag="two slabs")
    un = np.concatenate([out[0]["u"], out[1]["u"]], axis=1)
    assert [s["ew"]["kits"] for s in out[0]["steps"]] == [s["ew"]["kits"] for s in one["steps"]]
    check_state(un, one["u"], "two slabs against one")
    check_state(un, reference("ramp", 2)[1], "two slabs")


# ---- 7: environment paths ----------------------------------------------------------------------------------------------------------
def run_child(tmp_path_factory, env):
    """tests/ew_env_check.py in a fresh process with only `env` of the switches set (one run per setting, shared): its .npz as a dict."""
    return switches.run_child("ew_env_check.py", env, out=tmp_path_factory.mktemp("ew_env")/"out.npz", cache=True)


@pytest.mark.parametrize("env", [{"TP_FGMRES_PIPE": "0"}, {"TP_PIN": "0"}], ids=["pipe0", "pin0"])
def test_env_paths(tmp_path_factory, env):
    """Without the pipelined loop and without the pinned result buffer the history and the state under Eisenstat-Walker are those of
    the default paths, bit for bit (tests/ew_env_check.py; every setting runs in a fresh child process)."""
    base = run_child(tmp_path_factory, {})
    got = run_child(tmp_path_factory, env)
    assert sorted(got) == sorted(base) and len(base) == 12
    for k in base:
        assert np.array_equal(got[k], base[k]), k
    # ... and the default paths in a child are this process's run
    mine = gpu("ramp", ksp_ew=2)
    assert np.array_equal(base["fgmres.x"], mine["u"])
    assert np.array_equal(base["fgmres.rtol"], np.concatenate([s["ew"]["rtol"] for s in mine["steps"]]))
    assert (base["bcgs.counts"][:, 2] > 0).all() and (base["fgmres.counts"][:, 2] > 0).all()


# ---- 8: ew_info and a live engine --------------------------------------------------------------------------------------------------
def test_ew_info_and_set_options_on_a_live_engine():
    from thermalporous_amd.engine import HipEngine
    case, base, dts = INPUTS["c3"]
    spec, u0, *_ = case()
    h = HipEngine(spec, dict(base))
    assert h.ew_info() == dict(version=0, newton_solves=0, linear_solves=0, safeguarded=0) and h.ew_history()["n"] == 0

    def solve(version):
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(dts[0]*R.DAY)
        s = dict(h.newton_solve())
        s["ew"] = h.ew_history()
        return s
    s0 = solve(0)
    assert s0["reason"] > 0 and s0["ew"]["n"] == 0 and h.ew_info()["newton_solves"] == 0
    h.set_options(ksp_ew=2)                                 # takes effect at the next solve
    s2 = solve(2)
    r2 = check_formula([s2], 2, tag="live v2")
    assert s2["reason"] > 0 and h.ew_info() == dict(version=2, newton_solves=1, linear_solves=s2["ew"]["n"], safeguarded=r2)
    assert same_history([s2], gpu("c3", ksp_ew=2)["steps"][:1])
    h.set_options(ksp_ew=1, ew_rtol0=0.1)
    s1 = solve(1)
    r1 = check_formula([s1], 1, params=dict(rtol0=0.1), tag="live v1")
    assert s1["ew"]["rtol"][0] == 0.1
    assert h.ew_info() == dict(version=1, newton_solves=2, linear_solves=s2["ew"]["n"] + s1["ew"]["n"], safeguarded=r2 + r1)
    with pytest.raises(ValueError):
        h.set_options(ksp_ew=False)                         # ew_rtol0 would be ignored
    h.set_options(ksp_ew=False, ew_rtol0=0.3)
    s0b = solve(0)
    assert (s0b["nits"], s0b["lits"], s0b["fnorm"]) == (s0["nits"], s0["lits"], s0["fnorm"]) and s0b["ew"]["n"] == 0
    assert h.ew_info() == dict(version=0, newton_solves=2, linear_solves=s2["ew"]["n"] + s1["ew"]["n"], safeguarded=r2 + r1)
    h.close()


def test_library_refuses_bad_ew_options():
    """tp_set_options names the field it refuses (the Python checks are bypassed by packing the struct directly); the context
    stays usable.  tp_fgmres on its own keeps ksp_rtol under the option."""
    from thermalporous_amd import engine as E
    spec, u0, *_ = cases.c1_homogeneous(6, 1)
    h = E.HipEngine(spec, dict(pc="cpr"))
    for field, value, ver in (("ew_rtol0", 0.2, 0), ("ew_threshold", 0.5, 0), ("ew_alpha", 1.0, 2), ("ew_rtolmax", 1e-9, 1), ("ksp_ew", 3, 3),
                              ("ksp_ew", 4, 4)):
        t = E.HipEngine._make_options(h.opts)
        t.ksp_ew = ver
        setattr(t, field, value)
        assert h.lib.tp_set_options(h.ctx, C.byref(t)) != 0
        assert field.encode() in h.lib.tp_last_error(), (field, h.lib.tp_last_error())
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(R.DAY)
    fixed = h.newton_solve()
    h.set_options(ksp_ew=2)
    h.set_state(u0)
    ew = h.newton_solve()
    assert fixed["reason"] > 0 and ew["reason"] > 0 and ew["lits"] <= fixed["lits"]
    # a linear solve on its own: to ksp_rtol, whatever the option says
    h.set_state(u0)
    h.residual()
    h.jacobian()
    h.copy_residual_to("b")
    h.pc_setup()
    its, reason, rn = h.fgmres("b", "x")
    assert reason > 0 and rn <= h.opts["ksp_rtol"]*h.norm2("b")
    h.close()
