"""The opt-in BiCGStab outer solver on the GPU (tp_bcgs, tp_options.ksp_kind = 1) against the numpy reference tests/bcgs_ref.py
composed with the oracle's SpMV and two-stage preconditioner.

Tolerance of the linear-solve comparison (first min(its, 6) residual norms and the final x): not fixed by hand.  On the CPU
the reference runs twice on every input of bcgs_ref.PARITY, once with its sums taken in reversed order; the largest relative
deviation over those residual norms and the final x, over all cases, is the floor two legitimate summation orders differ by:
7.13e-6 (case c4_cptramg_QI; the other cases lie between 1e-16 and 2e-7).  The GPU sums in a third order, so 10 x that is
allowed: bcgs_ref.PARITY_TOL = 7.2e-5 (profiles/bcgs_parity.txt; tests/test_bcgs_host.py re-measures the floor).  Iteration
counts must agree to +-1; every input was chosen, from the reference alone, so that its residual history stays a factor 2
away from the tolerance at the steps around its stop (tests/test_bcgs_host.py checks all of them).
True residual: ||b - J x|| <= 2 tol with the oracle's SpMV.
tp_ksp_info counts recorded pc_apply programs; with TP_GRAPH=0 in the environment pc_apply is launched eagerly and nothing is
recorded, so the count the tests expect is PROGRAMS (2, or 0 under TP_GRAPH=0).  The switches the library reads once per process
(TP_PIN, TP_BCGS_WIDE, TP_GRAPH) are covered by child processes (test_env_switches, tests/bcgs_env_check.py)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bcgs_ref as R
import cases
import switches

pytestmark = pytest.mark.gpu

_REF = {}


def _off(name):
    """The library's own reading of a switch: set and atoi(value) == 0."""
    v = os.environ.get(name)
    if v is None:
        return False
    try:
        return int(v.strip() or 0) == 0
    except ValueError:
        return True


PROGRAMS = 0 if _off("TP_GRAPH") else 2                 # (p, p^) and (s, s^)


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def reference(shape, opts, dt, seed, b=None, key=None, **kw):
    """The oracle problem and the reference solve, computed once per input and shared (never modified)."""
    key = key or (shape, tuple(sorted(opts.items())), dt, seed)
    if key not in _REF:
        spec, u0, u, o, J, F = R.oracle_problem(shape, opts, seed=seed, dt=dt)
        rhs = F if b is None else b(o, J)
        info = {}
        x, its, reason, hist = R.solve_ref(o, J, rhs, info=info, **kw)
        _REF[key] = dict(spec=spec, u0=u0, u=u, J=J, b=rhs, x=x, its=its, reason=reason, hist=hist, info=info)
    return _REF[key]


def gpu_engine(ref, opts, dt, **kw):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(ref["spec"], opts, **kw)
    h.set_old(ref["u0"])
    h.set_dt(dt)
    h.set_state(ref["u"])
    h.jacobian()
    h.pc_setup()
    return h


def true_residual(ref, x, b=None):
    import oracle.linalg as la
    b = ref["b"] if b is None else b
    return np.linalg.norm((b - la.spmv_block(ref["J"], x)).ravel())


@pytest.mark.parametrize("name,shape,opts,dt,seed", R.PARITY, ids=[p[0] for p in R.PARITY])
def test_linear_solve_parity(name, shape, opts, dt, seed):
    ref = reference(shape, opts, dt, seed)
    h = gpu_engine(ref, opts, dt)
    mon = []
    h.set_ksp_monitor(lambda its, rn, fn: mon.append((its, rn, list(fn))))
    h.vec_set("b", ref["b"])
    its, reason, rn = h.bcgs("b", "d")
    h.set_ksp_monitor(None)
    x = h.vec_get("d")
    tol = R.RTOL*ref["hist"][0]
    n = min(its, ref["its"], 6)
    dev = [abs(mon[i][1] - ref["hist"][i + 1])/ref["hist"][i + 1] for i in range(n)]
    ex = rel2(x, ref["x"])
    tr = true_residual(ref, x)
    print("parity", name, "its", its, "ref", ref["its"], "max hist dev %.3e" % max(dev), "x rel2 %.3e" % ex, "true res/tol %.3f" % (tr/tol))
    assert reason == ref["reason"] == 2 and abs(its - ref["its"]) <= 1, (its, ref["its"], reason)
    assert [m[0] for m in mon] == list(range(1, its + 1)) and mon[-1][1] == rn          # once per iteration, with ||r||
    nb = ref["b"].shape[0]
    assert all(len(m[2]) == nb and np.isfinite(m[2]).all() for m in mon)
    # the monitor's per-field norms are those of the true residual: together they are ||b - J x_i||, which the recurrence tracks
    # (to 1e-10 ||b||: what the GPU's and the oracle's Jacobian may differ by, tests/test_gpu_parity.py)
    assert abs(np.sqrt(sum(v*v for v in mon[-1][2])) - tr) <= 1e-10*ref["hist"][0]
    assert max(dev) <= R.PARITY_TOL, dev
    assert ex <= R.PARITY_TOL, ex
    assert tr <= 2*tol, (tr, tol)
    info = h.ksp_info()
    assert info["pc_programs"] == PROGRAMS and info["bcgs_vectors"] == 7
    h.close()


def run_bcgs_slabs(ref, opts, dt, nslabs):
    """tp_bcgs on `nslabs` in-process slabs (threads sharing the GPU): [(its, reason, owned x)] per rank."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nslabs, C.byref(group)) == 0
    out, err = [None]*nslabs, []

    def worker(rank):
        try:
            h = gpu_engine(ref, opts, dt, rank=rank, nranks=nslabs, local_group=group)
            h.vec_set("b", ref["b"])
            its, reason, rn = h.bcgs("b", "d")
            out[rank] = (its, reason, h.vec_get("d"))
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nslabs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    alive = any(t.is_alive() for t in ts)
    assert not alive, "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    return out


@pytest.mark.parametrize("nslabs", [2, 3])
def test_slabs_match_one_slab(nslabs):
    name, shape, opts, dt, seed = R.PARITY[-1]
    assert name == "c4_cptr_planes"
    ref = reference(shape, opts, dt, seed)
    assert ref["spec"]["n"][2] == 13                    # 2 slabs: 7/6 planes, 3 slabs: the ragged 5/4/4
    h = gpu_engine(ref, opts, dt)
    h.vec_set("b", ref["b"])
    its1, reason1, _ = h.bcgs("b", "d")
    x1 = h.vec_get("d")
    h.close()
    out = run_bcgs_slabs(ref, opts, dt, nslabs)
    x = np.concatenate([o[2] for o in out], axis=1)
    assert x.shape == x1.shape
    print("slabs", nslabs, "its", [o[0] for o in out], "one slab", its1, "x rel2 %.3e" % rel2(x, x1))
    assert all(o[1] == reason1 == 2 for o in out)
    assert len({o[0] for o in out}) == 1 and abs(out[0][0] - its1) <= 1        # every rank forms the same latches
    assert rel2(x, x1) <= R.PARITY_TOL


def newton_pair(shape, opts, dt=86.4, **extra):
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()[shape]
    spec, u0, *_ = builder(**kw)
    res = []
    for ksp in ("fgmres", "bcgs"):
        h = HipEngine(spec, dict(opts, ksp=ksp, ksp_rtol=1e-8, snes_max_it=25, **extra))
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(dt)
        r = h.newton_solve()
        res.append((r, h.get_state(), h.ksp_info()))
        h.close()
    return res


@pytest.mark.parametrize("shape,opts,extra", [("c3", dict(pc="cptr", ilu_tile=R.T2D), {}), ("c4", dict(pc="cptr"), {}),
                                              ("c4", dict(pc="cpr"), dict(s1_ksp="richardson", s1_max_it=2))],
                         ids=["c3_cptr", "c4_cptr", "c4_cpr_richardson2"])
def test_newton_reaches_the_fgmres_state(shape, opts, extra):
    (rf, uf, kf), (rb, ub, kb) = newton_pair(shape, opts, **extra)
    print("newton", shape, opts, "fgmres", rf["nits"], rf["lits"], rf["vcycles"], "bcgs", rb["nits"], rb["lits"], rb["vcycles"])
    assert rf["reason"] > 0 and rb["reason"] > 0 and rb["lits"] > 0 and rb["ksp_reason"] == 2
    assert (kf["kind"], kb["kind"]) == (0, 1)
    # both loops stop on snes_rtol 1e-8 / snes_stol 1e-8 with linear solves to 1e-8: either state is within ~1e-8 (relative, per
    # field) of the root, times the few Newton steps taken; 1e-6 leaves two orders for that
    for f in range(uf.shape[0]):
        assert rel2(ub[f], uf[f]) < 1e-6, (f, rel2(ub[f], uf[f]))


def test_time_loop_with_fbcgs():
    from thermalporous_amd.twophase import TwoPhase
    spec, u0, p, g, c = cases.c3_spe10_2d(14, 19, 2)
    m = TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters="pc_cptr", filename=None, verbosity=False)
    sp = dict(m.solver_parameters)
    m.engine.close()
    m = TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters={**sp, "ksp_type": "fbcgs"}, filename=None, verbosity=False)
    assert m.engine_opts["ksp"] == "bcgs" and m.engine.ksp_info()["kind"] == 1
    m.solve()
    assert m.failed_solves == 0 and m.total_lits > 0
    assert m.engine.ksp_info()["bcgs_vectors"] == 7
    m.engine.close()


def test_limits_and_latches():
    name, shape, opts, dt, seed = R.PARITY[8]
    assert name == "c4_cptr"
    ref = reference(shape, opts, dt, seed)
    h = gpu_engine(ref, opts, dt)
    h.vec_set("b", ref["b"])
    # ksp_max_it
    h.set_options(ksp_max_it=2)
    its, reason, rn = h.bcgs("b", "d")
    assert (its, reason) == (2, -3) and abs(rn - ref["hist"][2]) <= R.PARITY_TOL*ref["hist"][2]
    h.set_options(ksp_max_it=200)
    # b = 0
    h.vec_set("z", np.zeros_like(ref["b"]))
    h.vec_set("d", np.ones_like(ref["b"]))
    assert h.bcgs("z", "d") == (0, 2, 0.0) and not h.vec_get("d").any()
    # NaN in b: -9, nothing else; the next solve on the same context is an ordinary one
    bn = ref["b"].copy()
    bn[1].flat[17] = np.nan
    h.vec_set("n", bn)
    its, reason, rn = h.bcgs("n", "d")
    assert (its, reason) == (0, -9)
    its, reason, rn = h.bcgs("b", "d")
    assert reason == 2 and abs(its - ref["its"]) <= 1
    assert rel2(h.vec_get("d"), ref["x"]) <= R.PARITY_TOL
    h.close()


def test_half_step_exit_takes_the_reference_count():
    shape, opts, dt, seed, rtol = R.HALF
    ref = reference(shape, opts, dt, seed, b=R.smooth_rhs, key="half", rtol=rtol)
    tol = rtol*ref["hist"][0]
    assert ref["reason"] == 2 and ref["info"]["half"] and R.clear_of_tolerance(ref["hist"], ref["info"]["snorm"], tol), ref["hist"]
    h = gpu_engine(ref, dict(opts, ksp_rtol=rtol), dt)
    h.vec_set("b", ref["b"])
    its, reason, rn = h.bcgs("b", "d")
    x = h.vec_get("d")
    print("half step: its", its, "ref", ref["its"], "x rel2 %.3e" % rel2(x, ref["x"]))
    assert (its, reason) == (ref["its"], 2)
    assert rel2(x, ref["x"]) <= R.PARITY_TOL and true_residual(ref, x) <= 2*tol
    h.close()


def test_workspace_and_switching_back():
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()["c4"]
    spec, u0, *_ = builder(**kw)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)

    def newton(h):
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(86.4)
        return h.newton_solve()
    h = HipEngine(spec, dict(opts, ksp="bcgs"))
    assert h.ksp_info() == dict(kind=1, bytes=0, bcgs_vectors=0, pc_programs=0)
    r = newton(h)
    assert r["reason"] > 0 and r["nits"] >= 2
    info = h.ksp_info()
    assert info["kind"] == 1 and info["bcgs_vectors"] == 7
    assert info["bytes"] == info["bcgs_vectors"]*h.b*h.ntot*8           # nothing for V and Z
    assert info["pc_programs"] == PROGRAMS                              # (p, p^) and (s, s^), however many set-ups ran
    # one explicit set-up and one solve: still the same two
    h.jacobian()
    h.pc_setup()
    h.copy_residual_to("b")
    h.bcgs("b", "d")
    assert h.ksp_info()["pc_programs"] == PROGRAMS
    h.set_options(ksp="fgmres")
    rh = newton(h)
    f = HipEngine(spec, opts)
    rf = newton(f)
    assert h.ksp_info()["kind"] == 0 and h.ksp_info()["bytes"] > info["bytes"]
    assert (rh["nits"], rh["lits"], rh["reason"]) == (rf["nits"], rf["lits"], rf["reason"])
    assert np.array_equal(h.get_state(), f.get_state())
    h.close()
    f.close()


def test_default_path_is_untouched():
    name, shape, opts, dt, seed = R.PARITY[8]
    ref = reference(shape, opts, dt, seed)
    h = gpu_engine(ref, opts, dt)
    assert h.ksp_info()["kind"] == 0
    h.vec_set("b", ref["b"])
    a = h.fgmres("b", "x1")
    x1 = h.vec_get("x1")
    assert h.ksp_info()["bcgs_vectors"] == 0
    its, reason, _ = h.bcgs("b", "d")
    assert reason == 2
    b = h.fgmres("b", "x1")
    assert a == b and np.array_equal(h.vec_get("x1"), x1)
    h.close()


# ---- switches read once per process ----------------------------------------------------------------------------------------
def run_child(tmp_path_factory, env):
    """tests/bcgs_env_check.py in a fresh process with only `env` of the switches set (one run per setting, shared): its .npz as a dict."""
    return switches.run_child("bcgs_env_check.py", env, out=tmp_path_factory.mktemp("bcgs_env")/"out.npz", cache=True)


@pytest.mark.parametrize("env", [{"TP_PIN": "0"}, {"TP_GRAPH": "0"}, {"TP_BCGS_WIDE": "0"}, {"TP_PIN": "0", "TP_BCGS_WIDE": "0"}],
                         ids=["pin0", "graph0", "wide0", "pin0_wide0"])
def test_env_switches(tmp_path_factory, env):
    """TP_PIN=0 (the host reads a copy of the state block instead of pinned memory) and TP_GRAPH=0 (eager pc_apply) change no
    arithmetic: iterations, norms and x are bitwise those of the default.  TP_BCGS_WIDE=0 moves 8-byte items where the default
    moves 16-byte ones, so a wave sums other entries: c3_cptr (even plane size, wide by default) agrees to the parity tolerance
    and +-1 iteration, c4_cptr (odd plane size, never wide) stays bitwise.  Both inputs are parity inputs, clear of the
    tolerance around their stop.  pc_apply programs: 2 recorded, none under TP_GRAPH=0."""
    base = run_child(tmp_path_factory, {})
    got = run_child(tmp_path_factory, env)
    names = sorted({k.split(".")[0] for k in base})
    assert names == ["c3_cptr", "c4_cptr"] and sorted(got) == sorted(base)
    for n in names:
        print("env", env, n, "its", int(got[n + ".its"]), "default", int(base[n + ".its"]), "x rel2 %.3e" % rel2(got[n + ".x"], base[n + ".x"]))
        assert int(base[n + ".reason"]) == int(got[n + ".reason"]) == 2 and int(base[n + ".programs"]) == 2
        assert int(got[n + ".programs"]) == (0 if "TP_GRAPH" in env else 2)
        if "TP_BCGS_WIDE" in env and n == "c3_cptr":
            assert abs(int(got[n + ".its"]) - int(base[n + ".its"])) <= 1
            assert rel2(got[n + ".x"], base[n + ".x"]) <= R.PARITY_TOL
            assert not np.array_equal(got[n + ".x"], base[n + ".x"])            # (the default did take the 16-byte path)
        else:
            assert int(got[n + ".its"]) == int(base[n + ".its"]) and float(got[n + ".rnorm"]) == float(base[n + ".rnorm"])
            assert np.array_equal(got[n + ".x"].view(np.uint64), base[n + ".x"].view(np.uint64))
