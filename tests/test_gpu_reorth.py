"""Gram-Schmidt refinement of the outer FGMRES on the GPU (tp_options.ksp_reorth, tp_vec_orth_step, tp_ksp_reorth_info;
DESIGN.md 4.6d) against the numpy reference tests/reorth_ref.py.

Step tests: the near-dependent inputs of reorth_ref (V orthonormal, w = V a + delta u) on a 2-D 7 x 9 two-phase grid (189
entries: fewer cells than one workgroup) and a 3-D 5 x 6 x 13 one (1170 entries: no multiple of a wave's 512, active tail lanes),
k in {1, 4, 5, 17} around the kernels' 4-vector load batches.  Tolerance of coefficients and final norm: reorth_ref.STEP_TOL =
10 x the deviation between two summation orders of the reference on these very inputs, per delta (tests/test_reorth_host.py
re-measures it; profiles/reorth_parity.txt).
Solver tests: the linear systems of tests/bcgs_ref.py; the first min(its, 6) residual norms, the final x and the Hessenberg
columns against reorth_ref.fgmres_ref within reorth_ref.FGMRES_TOL = 10 x the deviation between two summation orders of that
reference on those systems (4.32e-12, case c4_cpr; re-measured by tests/test_reorth_host.py), iteration counts +-1."""
import ctypes as C
import threading

import numpy as np
import pytest

import bcgs_ref as R
import cases
import reorth_ref as RR
import switches

pytestmark = pytest.mark.gpu

_REF = {}


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def grid_engine(shape, opts=None, **kw):
    from thermalporous_amd.engine import HipEngine
    builder, args = RR.SHAPES[shape]
    spec, u0, *_ = getattr(cases, builder)(**args)
    return HipEngine(spec, dict(opts or dict(pc="cpr")), **kw), spec, u0


# ---- 1. the step on its own ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(RR.SHAPES))
def test_step_parity(shape):
    h, spec, _ = grid_engine(shape)
    assert (h.b,) + tuple(spec["phi"].shape) == RR.VSHAPE[shape]
    steps = 0
    for k in RR.KS:
        pre = "k%d_" % k
        h.vec_batch(pre, k + 1)                       # basis = the first k vectors, w = one more vector of the batch
        wname = pre + str(k)
        fig = {}
        for delta in RR.DELTAS:
            V, w = RR.near_dependent(shape, k, delta)
            for i in range(k):
                h.vec_set(pre + str(i), V[i])
            for mode in RR.MODES:
                hr, nr, ranr, wr = RR.orth_step(V, w, mode)
                h.vec_set(wname, w)
                hg, ng, rang = h.orth_step(pre, k, wname, mode)
                steps += 1
                wg = h.vec_get(wname)
                dh = float(np.max(np.abs(hg - hr))/np.sqrt(np.sum(hr*hr)))
                dn = abs(ng - nr)/nr
                fig[(delta, mode)] = (RR.orth_figure(V, wg), RR.orth_figure(V, wr))
                print("step %s k %2d delta %g %-8s dh %.3e dn %.3e (tol %.3e) ran %s figure gpu %.3e ref %.3e"
                      % (shape, k, delta, mode, dh, dn, RR.STEP_TOL[delta], rang, *fig[(delta, mode)]))
                assert rang == ranr == (mode != "never")
                assert dh <= RR.STEP_TOL[delta] and dn <= RR.STEP_TOL[delta], (k, delta, mode, dh, dn)
                # the vector left on the device is the one the sums describe
                assert abs(RR.dot_forward(wg, wg) - ng) <= 1e-12*ng
            for mode in ("ifneeded", "always"):
                assert fig[(delta, mode)][0] <= 10*RR.TWO_PASS_FIGURE[delta], (k, delta, mode, fig[(delta, mode)])
        assert fig[(1e-8, "never")][0] >= RR.SEPARATION*fig[(1e-8, "always")][0], (k, fig)
    info = h.ksp_reorth_info()
    print("info", info)
    assert info == dict(mode="never", steps=steps, refined=steps*2//3, skipped=0)
    h.close()


def test_step_criterion_on_the_device():
    """The flag is the reference's decision: eta on either side of ||w'|| / ||w||, an exactly orthogonal w, w in span(V), w = 0,
    NaN in w.  A skipped second pass leaves the first pass's values bit for bit and counts as skipped."""
    shape, k, delta = "g3d", 5, 1e-4
    h, spec, _ = grid_engine(shape)
    V, w = RR.near_dependent(shape, k, delta)
    h.vec_batch("v", k + 1)
    for i in range(k):
        h.vec_set("v" + str(i), V[i])

    def step(w, mode, eta=RR.ETA):
        h.vec_set("v5", w)
        hg, ng, ran = h.orth_step("v", k, "v5", mode, eta)
        return hg, ng, ran, h.vec_get("v5")
    h0, n0, ran0, w0 = step(w, "never")
    # ||w'|| / ||w|| = 1e-4 / sqrt(1 + 1e-8): eta below it skips, above it refines
    for eta, want in ((1e-12, False), (0.5e-4, False), (2e-4, True), (RR.ETA, True)):
        hg, ng, ran, wg = step(w, "ifneeded", eta)
        assert ran == want == RR.orth_step(V, w, "ifneeded", eta)[2], eta
        if not want:
            assert np.array_equal(hg, h0) and ng == n0 and np.array_equal(wg, w0)
        else:
            assert not np.array_equal(wg, w0)
    assert h.ksp_reorth_info() == dict(mode="never", steps=5, refined=2, skipped=2)
    # exactly orthogonal (disjoint supports): h = 0, never refined; in span(V): refined, nothing divides; w = 0: not refined
    sup = [np.zeros_like(w) for _ in range(k)]
    for i in range(k):
        sup[i].flat[3 + 7*i] = 1.0
        h.vec_set("v" + str(i), sup[i])
    u = np.zeros_like(w)
    u.flat[600:640] = 1.0
    for eta in (1e-12, RR.ETA, 1.0 - 1e-12):
        hg, ng, ran, wg = step(u, "ifneeded", eta)
        assert not ran and not hg.any() and ng == 40.0 and np.array_equal(wg, u)
    hg, ng, ran, wg = step(3.0*sup[1], "ifneeded")
    assert ran and ng == 0.0 and list(hg) == [0.0, 3.0, 0.0, 0.0, 0.0] and not wg.any()
    hg, ng, ran, wg = step(np.zeros_like(w), "ifneeded")
    assert not ran and ng == 0.0
    # NaN: no refinement, the NaN reaches the host as in the one-pass step; "always" refines regardless
    wn = w.copy()
    wn.flat[11] = np.nan
    hg, ng, ran, wg = step(wn, "ifneeded")
    h1, n1, ran1, w1 = step(wn, "never")
    assert not ran and np.isnan(ng) and np.array_equal(hg, h1, equal_nan=True) and np.array_equal(wg, w1, equal_nan=True)
    assert np.isnan(n1)
    assert step(wn, "always")[2]
    h.close()


# ---- 2. a criterion that never fires is the one-pass solver, bit for bit ---------------------------------------------------
def newton(h, u0, dt=86.4):
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(dt)
    return h.newton_solve()


@pytest.mark.parametrize("monitor", [False, True], ids=["pipelined", "monitor"])
def test_ifneeded_that_never_fires_is_bitwise_never(monitor):
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()["c4"]
    spec, u0, *_ = builder(**kw)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    res = []
    for extra in ({}, dict(ksp_reorth="ifneeded", ksp_reorth_eta=1e-12)):
        h = HipEngine(spec, dict(opts, **extra))
        mon = []
        if monitor:                       # (the monitor takes the loop off its pipelined path)
            h.set_ksp_monitor(lambda its, rn, fn: mon.append((its, rn)))
        r = newton(h, u0)
        res.append((r, h.get_state(), h.ksp_reorth_info(), mon))
        h.close()
    (r0, x0, i0, m0), (r1, x1, i1, m1) = res
    print("never", r0["nits"], r0["lits"], i0, "ifneeded 1e-12", r1["nits"], r1["lits"], i1)
    assert r0["reason"] > 0 and r0["lits"] > 0
    assert (r0["nits"], r0["lits"], r0["reason"]) == (r1["nits"], r1["lits"], r1["reason"])
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64)) and m0 == m1
    assert i0 == dict(mode="never", steps=r0["lits"], refined=0, skipped=0)
    assert i1 == dict(mode="ifneeded", steps=r1["lits"], refined=0, skipped=r1["lits"])


# ---- 3. the solver against the reference ------------------------------------------------------------------------------------
def reference(name, mode):
    """The oracle problem (shared between the modes, never modified) and the reference solve of one mode."""
    name_, shape, opts, dt, seed = next(p for p in R.PARITY if p[0] == name)
    if name not in _REF:
        spec, u0, u, o, J, F = R.oracle_problem(shape, opts, seed=seed, dt=dt)
        _REF[name] = dict(spec=spec, u0=u0, u=u, o=o, J=J, b=F, opts=opts, dt=dt)
    ref = _REF[name]
    if mode not in ref:
        info = {}
        x, its, reason, hist = RR.solve_ref(ref["o"], ref["J"], ref["b"], mode, info=info)
        ref[mode] = dict(x=x, its=its, reason=reason, hist=hist, info=info)
    return ref, ref[mode]


def gpu_engine(ref, opts, **kw):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(ref["spec"], opts, **kw)
    h.set_old(ref["u0"])
    h.set_dt(ref["dt"])
    h.set_state(ref["u"])
    h.jacobian()
    h.pc_setup()
    return h


@pytest.mark.parametrize("name", [p[0] for p in R.PARITY])
def test_fgmres_parity(name):
    for mode in ("always", "ifneeded"):
        ref, rs = reference(name, mode)
        h = gpu_engine(ref, dict(ref["opts"], ksp_reorth=mode))
        mon = []
        h.set_ksp_monitor(lambda its, rn, fn: mon.append(rn))
        h.vec_set("b", ref["b"])
        its, reason, rn = h.fgmres("b", "x")
        h.set_ksp_monitor(None)
        x = h.vec_get("x")
        info = h.ksp_reorth_info()
        n = min(its, rs["its"])
        dev = max(abs(mon[i] - rs["hist"][i + 1])/rs["hist"][i + 1] for i in range(min(n, 6)))
        fired = sum(rs["info"]["fired"])
        near = sum(0.99 < m < 1.01 for m in rs["info"]["margin"])       # criteria within rounding of eta
        print("fgmres", name, mode, "its", its, "ref", rs["its"], "hist dev %.3e" % dev, "x rel2 %.3e" % rel2(x, rs["x"]),
              "second passes", info["refined"], "ref", fired, "near eta", near)
        assert reason == rs["reason"] == 2 and abs(its - rs["its"]) <= 1
        assert dev <= RR.FGMRES_TOL and rel2(x, rs["x"]) <= RR.FGMRES_TOL
        assert info["mode"] == mode and info["steps"] == its and info["refined"] + info["skipped"] == its
        assert abs(info["refined"] - fired) <= near + abs(its - rs["its"])
        if mode == "always":
            assert info["refined"] == its
        # the same solve again without the monitor (the pipelined loop): the same iterates
        its2, reason2, rn2 = h.fgmres("b", "x2")
        assert (its2, reason2, rn2) == (its, reason, rn) and np.array_equal(h.vec_get("x2"), x)
        h.close()


def test_hessenberg_columns_are_h_plus_c():
    """Arnoldi driven from here over the exported kernels (tp_pc_apply, tp_spmv, tp_vec_orth_step with "always"): column j of the
    Hessenberg matrix, as the host of tp_fgmres reads it, is the reference's h + c and final ||w||."""
    ref, rs = reference("c4_cptr", "always")
    h = gpu_engine(ref, dict(ref["opts"]))
    ncol = min(rs["its"], 6)
    h.vec_batch("v", ncol + 1)
    beta = rs["hist"][0]
    h.vec_set("v0", ref["b"]/beta)
    for j in range(ncol):
        h.pc_apply("v" + str(j), "z")
        h.spmv("z", "v" + str(j + 1))
        hg, n2, ran = h.orth_step("v", j + 1, "v" + str(j + 1), "always")
        col = np.append(hg, np.sqrt(n2))
        want = rs["info"]["hcol"][j]
        dev = float(np.max(np.abs(col - want))/np.linalg.norm(want))
        print("column", j, "dev %.3e" % dev)
        assert ran and dev <= RR.FGMRES_TOL
        h.vec_set("v" + str(j + 1), h.vec_get("v" + str(j + 1))/np.sqrt(n2))
    h.close()


# ---- 4. nothing is left behind ----------------------------------------------------------------------------------------------
def test_default_solve_is_untouched_by_an_earlier_always():
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()["c4"]
    spec, u0, *_ = builder(**kw)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    assert "ksp_reorth" not in opts
    a = HipEngine(spec, opts)
    ra, xa = newton(a, u0), a.get_state()
    a.close()
    b = HipEngine(spec, dict(opts, ksp_reorth="always"))
    rb, xb = newton(b, u0), b.get_state()
    ib = b.ksp_reorth_info()
    assert rb["reason"] > 0 and ib == dict(mode="always", steps=rb["lits"], refined=rb["lits"], skipped=0)
    # ... on the same context after switching back, and on a fresh one
    b.set_options(ksp_reorth="never")
    rb2, xb2 = newton(b, u0), b.get_state()
    assert b.ksp_reorth_info()["refined"] == ib["refined"]
    b.close()
    c = HipEngine(spec, opts)
    rc, xc = newton(c, u0), c.get_state()
    assert c.ksp_reorth_info() == dict(mode="never", steps=rc["lits"], refined=0, skipped=0)
    c.close()
    for r, x in ((rb2, xb2), (rc, xc)):
        assert (r["nits"], r["lits"], r["reason"]) == (ra["nits"], ra["lits"], ra["reason"])
        assert np.array_equal(x.view(np.uint64), xa.view(np.uint64))
    assert rc["vcycles"] == ra["vcycles"]                 # (a context's count runs on over its solves: fresh against fresh)
    # the counts are those of the CPU oracle, as before the option existed (what smoke() checks at this size)
    o = OracleEngine(spec, opts)
    ro = newton(o, u0)
    print("default", ra["nits"], ra["lits"], "always", rb["nits"], rb["lits"], "oracle", ro["nits"], ro["lits"])
    assert ra["nits"] == ro["nits"] and ra["reason"] == ro["reason"]
    # the refined solve reaches the same state (both stop on snes_rtol / snes_stol 1e-8 with linear solves to 1e-8)
    for f in range(xa.shape[0]):
        assert rel2(xb[f], xa[f]) < 1e-6


# ---- 5. slabs -----------------------------------------------------------------------------------------------------------------
SLAB_OPTS = dict(pc="cptr", ilu_tile=(1 << 30, 16, 1), amg_gather_cells=-1)       # (the same preconditioner however the planes are cut)


def slab_solve(spec, u0, u, opts, rank=0, nranks=1, group=None):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts, rank=rank, nranks=nranks, local_group=group)
    h.set_old(u0)
    h.set_dt(86.4)
    h.set_state(u)
    h.jacobian()
    h.pc_setup()
    h.copy_residual_to("b")
    out = (h.fgmres("b", "x"), h.vec_get("x"), h.ksp_reorth_info())
    h.close()
    return out


@pytest.mark.parametrize("mode", ["always", "ifneeded"])
def test_two_slabs_match_one_slab(mode):
    from thermalporous_amd import engine as E
    builder, args = RR.SHAPES["g3d"]
    spec, u0, *_ = getattr(cases, builder)(**args)
    assert spec["n"][2] == 6                              # 2 slabs of 3 planes
    u = cases.perturbed_state(spec, seed=3, amp=0.3)
    opts = dict(SLAB_OPTS, ksp_reorth=mode)
    (its1, reason1, rn1), x1, info1 = slab_solve(spec, u0, u, opts)
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(2, C.byref(group)) == 0
    out, err = [None]*2, []

    def worker(rank):
        try:
            out[rank] = slab_solve(spec, u0, u, opts, rank, 2, group)
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    x = np.concatenate([o[1] for o in out], axis=1)
    print("slabs", mode, "its", [o[0][0] for o in out], "one slab", its1, "x rel2 %.3e" % rel2(x, x1), [o[2] for o in out], info1)
    assert reason1 == 2 and all(o[0][1] == 2 for o in out)
    assert out[0][0][0] == out[1][0][0] == its1
    assert out[0][2] == out[1][2]                         # every rank takes the same decisions
    assert out[0][2]["steps"] == its1 and out[0][2]["refined"] + out[0][2]["skipped"] == its1
    if mode == "always":
        assert out[0][2]["refined"] == its1 == info1["refined"]
    assert rel2(x, x1) <= R.PARITY_TOL


# ---- switches the library reads once per process -----------------------------------------------------------------------------
def run_child(tmp_path_factory, env):
    """tests/reorth_env_check.py in a fresh process with only `env` of the switches set (one run per setting, shared): its .npz as a dict."""
    return switches.run_child("reorth_env_check.py", env, out=tmp_path_factory.mktemp("reorth_env")/"out.npz", cache=True)


@pytest.mark.parametrize("env", [{"TP_PIN": "0"}, {"TP_FGMRES_PIPE": "0"}, {"TP_REORTH_DOT_REVERSE": "1"}], ids=["pin0", "pipe0", "dotrev"])
def test_env_switches(tmp_path_factory, env):
    """The paths without the pinned result buffer (TP_PIN=0) and without the pipelined loop (TP_FGMRES_PIPE=0), and the second
    dot pass walked the other way, change no arithmetic: a Newton solve with "always" and one with "ifneeded" are bitwise those
    of the default paths (tests/reorth_env_check.py)."""
    base = run_child(tmp_path_factory, {})
    got = run_child(tmp_path_factory, env)
    assert sorted(got) == sorted(base) and len(base) == 6
    for k in base:
        assert np.array_equal(got[k], base[k]), k
    assert int(base["always.counts"][3]) == int(base["always.counts"][1]) > 0          # (refined == lits)
