"""The opt-in fp32 storage of the FGMRES bases on the GPU (tp_options.ksp_basis_single) against the numpy reference
tests/basis_single_ref.py composed with the oracle's SpMV and two-stage preconditioner.

Kernels alone, through the float-batch exports (tp_fvec_*): a stored slot is numpy's astype(float32) bitwise; dots and the
multi-axpy against numpy on the rounded data, to the tolerances tests/test_gpu_parity.py uses for the fp64 batch calls.
Tolerance of the linear-solve comparison (first min(its, 6) monitored residual norms and the final x): not fixed by hand.  On
the CPU the reference runs twice on every input, once with its sums taken in reversed order; the largest relative deviation
over all inputs is the floor two legitimate summation orders differ by, 3.15e-7 (c1_cpr; the others lie below 4e-10).  The GPU
sums in a third order, so 10 x that is allowed: basis_single_ref.PARITY_TOL = 3.2e-6 (profiles/basis_single_parity.txt;
tests/test_basis_single_host.py re-measures the floor).  Iteration counts agree to +-1 and cycle counts exactly; every input
was chosen, from the reference alone, clear of every threshold it meets (tests/test_basis_single_host.py).
The returned rnorm is the TRUE residual norm: ||b - J x|| with the oracle's SpMV to 1e-10 ||b|| (what the GPU's and the
oracle's Jacobian may differ by), and <= tol.  With TP_GRAPH=0 in the environment pc_apply is launched eagerly and nothing is
recorded: the program count the tests expect is PROGRAMS (1, or 0 under TP_GRAPH=0).  The switches read once per process are
covered by child processes (test_env_switches, tests/basis_single_env_check.py)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import basis_single_ref as R
import cases
import switches

pytestmark = pytest.mark.gpu

_REF = {}
BY_NAME = {p[0]: p for p in R.PARITY + [R.LONG]}


def _off(name):
    """The library's own reading of a switch: set and atoi(value) == 0."""
    v = os.environ.get(name)
    if v is None:
        return False
    try:
        return int(v.strip() or 0) == 0
    except ValueError:
        return True


PROGRAMS = 0 if _off("TP_GRAPH") else 1                 # the one (staging 0, staging 1) pair


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def reference(p, **over):
    """The oracle problem and the reference solve of an input, computed once and shared (never modified)."""
    name, shape, opts, dt, seed, kw = p
    key = (name, tuple(sorted(over.items())))
    if key not in _REF:
        base = _REF.get((name, ()))
        if base is None:
            spec, u0, u, o, J, F = R.oracle_problem(shape, opts, seed=seed, dt=dt)
            base = dict(spec=spec, u0=u0, u=u, J=J, b=F, o=o)
        info = {}
        x, its, reason, hist, ncyc, orth = R.solve_ref(base["o"], base["J"], base["b"], info=info, **{**R.solver_kw(kw)[0], **over})
        _REF[key] = dict(base, x=x, its=its, reason=reason, hist=hist, cycles=ncyc, info=info)
    return _REF[key]


def gpu_engine(ref, p, single=True, **kw):
    from thermalporous_amd.engine import HipEngine
    eng = dict(p[2], **R.solver_kw(p[5])[1])
    eng.update(kw.pop("opts", {}))
    h = HipEngine(ref["spec"], dict(eng, ksp_basis_single=single), **kw)
    h.set_old(ref["u0"])
    h.set_dt(p[3])
    h.set_state(ref["u"])
    h.jacobian()
    h.pc_setup()
    return h


def true_residual(ref, x, b=None):
    import oracle.linalg as la
    b = ref["b"] if b is None else b
    return np.linalg.norm((b - la.spmv_block(ref["J"], x)).ravel())


# ---- the kernels alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["c1", "c4"])
def test_float_batch_kernels(shape):
    """c1: 2 x 144 = 288 entries, under one 512-entry chunk; c4: 3 x 819 = 2457 entries, four chunks and a tail that is no
    multiple of 4, odd plane size.  k = 1..9 and 17: every remainder of the 4-vector unrolling, with and without full groups."""
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()[shape]
    spec, u0, *_ = builder(**kw)
    h = HipEngine(spec, dict(pc="cpr"))
    info = h.ksp_basis_info()
    nall = h.b*h.np_*h.n[2]
    assert info["stride"] == -(-nall//64)*64 and not info["single"] and info["capacity"] == info["staging"] == 0
    rng = np.random.default_rng(11)
    n = 17
    shp = (h.b,) + spec["phi"].shape
    V = rng.standard_normal((n,) + shp)*10.0**rng.integers(-6, 7, size=(n,) + shp)         # a wide range of exponents
    V[3].flat[5] = 1e-50                     # rounds to zero
    V[4].flat[7] = 1.0 + 2.0**-24            # a tie: round to even
    Vr = V.astype(np.float32)
    h.fvec_batch("f", n)
    for i in range(n):
        h.vec_set("t", V[i])
        h.fvec_store("f", i, "t")
        got = h.fvec_get("f", i)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), Vr[i].reshape(got.shape).view(np.uint32)), i
        # the fp64 vector comes back as the widened stored value
        assert np.array_equal(h.vec_get("t"), Vr[i].astype(np.float64).reshape(got.shape))
    w = rng.standard_normal(shp)
    Vd = Vr.astype(np.float64)
    for k in list(range(1, 10)) + [17]:
        h.vec_set("w", w)
        d = h.fdot_batch("f", k, "w")
        assert np.allclose(d, [np.vdot(Vd[i], w) for i in range(k)], rtol=1e-12, atol=1e-9), k
        coef = rng.standard_normal(k)
        h.faxpy_batch("f", k, coef, "w")
        assert rel2(h.vec_get("w"), w + np.tensordot(coef, Vd[:k], axes=1)) < 1e-13, k
    with pytest.raises(Exception):
        h.fdot_batch("f", 18, "w")
    h.close()


# ---- linear solves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", R.PARITY + [R.LONG], ids=[p[0] for p in R.PARITY + [R.LONG]])
def test_linear_solve_parity(p):
    ref = reference(p)
    h = gpu_engine(ref, p)
    assert h.ksp_basis_info()["single"]
    mon = []
    h.set_ksp_monitor(lambda its, rn, fn: mon.append((its, rn, list(fn))))
    h.vec_set("b", ref["b"])
    its, reason, rn = h.fgmres("b", "d")
    h.set_ksp_monitor(None)
    x = h.vec_get("d")
    info = h.ksp_basis_info()
    tol = R.solver_kw(p[5])[0]["rtol"]*ref["hist"][0]
    n = min(its, ref["its"], 6)
    dev = [abs(mon[i][1] - ref["hist"][i + 1])/ref["hist"][i + 1] for i in range(n)]
    ex = rel2(x, ref["x"])
    tr = true_residual(ref, x)
    print("parity", p[0], "its", its, "ref", ref["its"], "cycles", info["cycles"], "ref", ref["cycles"], "max hist dev %.3e" % max(dev),
          "x rel2 %.3e" % ex, "rnorm/tol %.3f" % (rn/tol), "|rnorm - true|/||b|| %.2e" % (abs(rn - tr)/ref["hist"][0]))
    assert reason == ref["reason"] == 2 and abs(its - ref["its"]) <= 1, (its, ref["its"], reason)
    assert info["cycles"] == ref["cycles"] == info["true_residuals"]
    assert [m[0] for m in mon] == list(range(1, its + 1))                  # once per iteration
    nb = ref["b"].shape[0]
    assert all(len(m[2]) == nb and np.isfinite(m[2]).all() for m in mon)
    # the monitor's per-field norms are those of the true residual of the iterate: the last ones add up to ||b - J x||
    assert abs(np.sqrt(sum(v*v for v in mon[-1][2])) - tr) <= 1e-10*ref["hist"][0]
    assert max(dev) <= R.PARITY_TOL, dev
    assert ex <= R.PARITY_TOL, ex
    assert abs(rn - tr) <= 1e-10*ref["hist"][0] and rn <= tol, (rn, tr, tol)
    assert h.ksp_info()["pc_programs"] == PROGRAMS
    h.close()


def test_tight_tolerance_converges_on_the_true_residual():
    """rtol 1e-10 is below what one cycle of the rounded basis can deliver: without the floor the recurrence residual would pass
    the tolerance with the true residual 270 x above it (tests/test_basis_single_host.py), and without the true-residual
    test that would be reported as convergence."""
    name, rtol = R.TIGHT
    p = BY_NAME[name]
    ref = reference(p, rtol=rtol)
    assert ref["reason"] == 2 and ref["cycles"] >= 2
    h = gpu_engine(ref, p, opts=dict(ksp_rtol=rtol))
    h.vec_set("b", ref["b"])
    its, reason, rn = h.fgmres("b", "d")
    x = h.vec_get("d")
    tol = rtol*ref["hist"][0]
    tr = true_residual(ref, x)
    info = h.ksp_basis_info()
    print("tight", name, "its", its, "ref", ref["its"], "cycles", info["cycles"], "true/tol %.3f" % (tr/tol))
    assert reason == 2 and tr <= tol and rn <= tol and info["cycles"] >= 2 and info["true_residuals"] == info["cycles"]
    assert abs(its - ref["its"]) <= 1
    h.close()


def test_discarded_speculation_leaves_no_trace():
    """ksp_rtol 0.05 on the pc_cptramg_QI input (the pc_cptr input's convergence is too even for any tolerance to do this): the
    reference converges in ONE iteration, its recurrence residual 0.0084 ||b|| a factor 2 and more under the threshold, and
    confirms it on the true residual of its one cycle.  The pipelined loop has by then queued the speculative v_1,
    z_1 = M^-1 v_1 and J z_1 (the predicted residual, ||b||, is above TP_SPEC_MARGIN x stop = 0.2 ||b||, by more than a factor 2
    as well), through the staging vectors into slot 1 of both bases; that work is discarded.  This solve and the ordinary one
    that follows on the same context are the reference's."""
    rtol = 0.05
    p = BY_NAME["c4_cptramg_QI"]
    ref1, ref = reference(p, rtol=rtol), reference(p)
    bn = ref["hist"][0]
    assert (ref1["its"], ref1["reason"], ref1["cycles"]) == (1, 2, 1) and ref1["hist"][1] <= 0.5*rtol*bn and 2*4*rtol <= 1.0
    h = gpu_engine(ref, p, opts=dict(ksp_rtol=rtol))
    h.vec_set("b", ref["b"])
    its, reason, rn = h.fgmres("b", "d")
    x = h.vec_get("d")
    tr = true_residual(ref, x)
    info = h.ksp_basis_info()
    print("discarded: its", its, "rnorm/||b|| %.4e" % (rn/bn), "ref %.4e" % (ref1["info"]["rnorm"]/bn), "x rel2 %.3e" % rel2(x, ref1["x"]))
    assert (its, reason, info["cycles"], info["true_residuals"]) == (1, 2, 1, 1)
    assert rel2(x, ref1["x"]) <= R.PARITY_TOL
    assert abs(rn - tr) <= 1e-10*bn and rn <= rtol*bn
    h.set_options(ksp_rtol=R.RTOL)
    its, reason, rn = h.fgmres("b", "d")
    assert reason == 2 and abs(its - ref["its"]) <= 1 and h.ksp_basis_info()["cycles"] == ref["cycles"]
    assert rel2(h.vec_get("d"), ref["x"]) <= R.PARITY_TOL and rn <= R.RTOL*bn
    h.close()


def test_limits():
    p = BY_NAME["c4_cptr"]
    ref = reference(p)
    h = gpu_engine(ref, p)
    h.vec_set("b", ref["b"])
    # ksp_max_it: the true residual norm is returned
    h.set_options(ksp_max_it=2)
    its, reason, rn = h.fgmres("b", "d")
    tr = true_residual(ref, h.vec_get("d"))
    assert (its, reason) == (2, -3) and abs(rn - tr) <= 1e-10*ref["hist"][0] and rn > 1e-8*ref["hist"][0]
    assert abs(rn - ref["hist"][2]) <= 1e-3*ref["hist"][2]                # (and it is what the recurrence says, two iterations in)
    h.set_options(ksp_max_it=200)
    # b = 0
    h.vec_set("z", np.zeros_like(ref["b"]))
    h.vec_set("d", np.ones_like(ref["b"]))
    assert h.fgmres("z", "d") == (0, 2, 0.0) and not h.vec_get("d").any()
    # NaN in b: -9, nothing else; the next solve on the same context is an ordinary one
    bn = ref["b"].copy()
    bn[1].flat[17] = np.nan
    h.vec_set("n", bn)
    its, reason, rn = h.fgmres("n", "d")
    assert (its, reason) == (0, -9)
    its, reason, rn = h.fgmres("b", "d")
    assert reason == 2 and abs(its - ref["its"]) <= 1 and h.ksp_basis_info()["cycles"] == ref["cycles"]
    assert rel2(h.vec_get("d"), ref["x"]) <= R.PARITY_TOL
    # the floor is an option: theta = 0.5 ends every cycle after a reduction by 2
    h.set_options(ksp_single_floor=0.5)
    its2, reason, rn = h.fgmres("b", "d")
    assert reason == 2 and h.ksp_basis_info()["cycles"] > ref["cycles"] and rn <= 1e-8*ref["hist"][0]
    with pytest.raises(ValueError):
        h.set_options(ksp_single_floor=1.0)
    with pytest.raises(NotImplementedError):
        h.set_options(ksp="bcgs")
    h.close()


def test_workspace_is_halved_and_programs_do_not_grow():
    p = R.LONG
    ref = reference(p)
    h = gpu_engine(ref, p)
    assert h.ksp_info()["bytes"] == 0
    h.vec_set("b", ref["b"])
    its, reason, rn = h.fgmres("b", "d")
    assert reason == 2 and its > 50
    ki, bi = h.ksp_info(), h.ksp_basis_info()
    nall = h.b*h.np_*h.n[2]
    assert bi["stride"] == -(-nall//64)*64 and bi["staging"] == 2 and bi["capacity"] >= 31
    assert ki["bytes"] == bi["capacity"]*2*bi["stride"]*4 + bi["staging"]*h.b*h.ntot*8
    assert ki["pc_programs"] == PROGRAMS                  # 58 iterations, one (input, output) pair
    f = gpu_engine(ref, p, single=False)
    f.vec_set("b", ref["b"])
    itf, reasonf, _ = f.fgmres("b", "d")
    kf = f.ksp_info()
    print("workspace: fp32 basis", ki["bytes"], "fp64", kf["bytes"], "ratio %.3f" % (ki["bytes"]/kf["bytes"]), "its", its, itf,
          "programs", ki["pc_programs"], kf["pc_programs"])
    assert reasonf == 2 and f.ksp_basis_info()["capacity"] == 0 and not f.ksp_basis_info()["single"]
    assert ki["bytes"] < 0.55*kf["bytes"]
    assert rel2(h.vec_get("d"), f.vec_get("d")) <= 1e-6
    h.close()
    f.close()


# ---- the default path ------------------------------------------------------------------------------------------------------------
def test_default_path_is_untouched():
    p = BY_NAME["c4_cptr"]
    ref = reference(p)
    h = gpu_engine(ref, p, single=False)
    h.vec_set("b", ref["b"])
    a = h.fgmres("b", "x1")
    x1 = h.vec_get("x1")
    b64 = h.ksp_info()["bytes"]
    assert b64 > 0 and h.ksp_basis_info()["capacity"] == 0
    h.set_options(ksp_basis_single=True)
    its, reason, _ = h.fgmres("b", "d")
    assert reason == 2 and h.ksp_basis_info()["capacity"] > 0
    assert h.ksp_info()["bytes"] < b64                    # the fp64 bases were freed
    h.set_options(ksp_basis_single=False)
    assert h.ksp_info()["bytes"] == 0                     # ... and so are the fp32 ones
    b = h.fgmres("b", "x1")
    assert a == b and np.array_equal(h.vec_get("x1"), x1) and h.ksp_info()["bytes"] == b64
    f = gpu_engine(ref, p, single=False)
    f.vec_set("b", ref["b"])
    assert f.fgmres("b", "x1") == a and np.array_equal(f.vec_get("x1"), x1)
    h.close()
    f.close()


def newton(h, u0, dt=86.4):
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(dt)
    return h.newton_solve()


def test_newton_with_the_option_off_is_the_default():
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()["c4"]
    spec, u0, *_ = builder(**kw)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    h = HipEngine(spec, dict(opts, ksp_basis_single=True))
    rs = newton(h, u0)
    assert rs["reason"] > 0 and h.ksp_basis_info()["cycles"] >= 1
    h.set_options(ksp_basis_single=False)
    rh = newton(h, u0)
    f = HipEngine(spec, opts)
    rf = newton(f, u0)
    assert (rh["nits"], rh["lits"], rh["reason"]) == (rf["nits"], rf["lits"], rf["reason"])
    assert np.array_equal(h.get_state(), f.get_state())
    h.close()
    f.close()


# ---- Newton and the time loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,opts", [("c3", dict(pc="cptr", ilu_tile=R.T2D)), ("c4", dict(pc="cptr"))], ids=["c3_cptr", "c4_cptr"])
def test_newton_reaches_the_fp64_state(shape, opts):
    from thermalporous_amd.engine import HipEngine
    builder, kw = R._shapes()[shape]
    spec, u0, *_ = builder(**kw)
    res = []
    for single in (False, True):
        h = HipEngine(spec, dict(opts, ksp_basis_single=single, ksp_rtol=1e-8, snes_max_it=25))
        r = newton(h, u0)
        res.append((r, h.get_state(), h.ksp_basis_info()))
        h.close()
    (rf, uf, _), (rs, us, bs) = res
    print("newton", shape, "fp64", rf["nits"], rf["lits"], "fp32 basis", rs["nits"], rs["lits"], "cycles of the last solve", bs["cycles"])
    assert rf["reason"] > 0 and rs["reason"] > 0 and rs["lits"] > 0 and rs["ksp_reason"] == 2 and bs["single"]
    # both loops stop on snes_rtol 1e-8 / snes_stol 1e-8 with linear solves to 1e-8: either state is within ~1e-8 (relative, per
    # field) of the root, times the few Newton steps taken; 1e-6 leaves two orders for that (tests/test_gpu_bcgs.py)
    for f in range(uf.shape[0]):
        assert rel2(us[f], uf[f]) < 1e-6, (f, rel2(us[f], uf[f]))


def test_time_loop_with_the_option():
    from thermalporous_amd.twophase import TwoPhase
    spec, u0, p, g, c = cases.c3_spe10_2d(14, 19, 2)
    m = TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters="pc_cptr", filename=None, verbosity=False)
    sp = dict(m.solver_parameters)
    m.engine.close()
    m = TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters={**sp, "ksp_basis_single": True}, filename=None, verbosity=False)
    assert m.engine_opts["ksp_basis_single"] is True and m.engine.ksp_basis_info()["single"]
    m.solve()
    assert m.failed_solves == 0 and m.total_lits > 0
    bi = m.engine.ksp_basis_info()
    assert bi["capacity"] > 0 and bi["staging"] == 2 and bi["cycles"] >= 1
    m.engine.close()


# ---- slabs -----------------------------------------------------------------------------------------------------------------------
def run_slabs(ref, p, nslabs):
    """tp_fgmres with ksp_basis_single on `nslabs` in-process slabs (threads sharing the GPU): [(its, reason, owned x, cycles)]."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nslabs, C.byref(group)) == 0
    out, err = [None]*nslabs, []

    def worker(rank):
        try:
            h = gpu_engine(ref, p, rank=rank, nranks=nslabs, local_group=group)
            h.vec_set("b", ref["b"])
            its, reason, rn = h.fgmres("b", "d")
            out[rank] = (its, reason, h.vec_get("d"), h.ksp_basis_info()["cycles"], rn)
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
    p = BY_NAME["c4_cptr_planes"]
    ref = reference(p)
    assert ref["spec"]["n"][2] == 13                    # 2 slabs: 7/6 planes, 3 slabs: the ragged 5/4/4
    h = gpu_engine(ref, p)
    h.vec_set("b", ref["b"])
    its1, reason1, rn1 = h.fgmres("b", "d")
    x1 = h.vec_get("d")
    cyc1 = h.ksp_basis_info()["cycles"]
    h.close()
    out = run_slabs(ref, p, nslabs)
    x = np.concatenate([o[2] for o in out], axis=1)
    assert x.shape == x1.shape
    print("slabs", nslabs, "its", [o[0] for o in out], "one slab", its1, "cycles", [o[3] for o in out], cyc1, "x rel2 %.3e" % rel2(x, x1))
    assert all(o[1] == reason1 == 2 for o in out)
    assert len({(o[0], o[3], o[4]) for o in out}) == 1 and abs(out[0][0] - its1) <= 1 and out[0][3] == cyc1      # every rank takes the same decisions
    assert rel2(x, x1) <= R.PARITY_TOL


# ---- switches read once per process ----------------------------------------------------------------------------------------
def run_child(tmp_path_factory, env):
    """tests/basis_single_env_check.py in a fresh process with only `env` of the switches set (one run per setting, shared): its .npz as a dict."""
    return switches.run_child("basis_single_env_check.py", env, out=tmp_path_factory.mktemp("basis_env")/"out.npz", cache=True)


@pytest.mark.parametrize("env", [{"TP_FGMRES_PIPE": "0"}, {"TP_PIN": "0"}, {"TP_GRAPH": "0"}, {"TP_MD_CHUNK": "4"},
                                 {"TP_BASIS_VEC": "2"}, {"TP_BASIS_VEC": "1"}, {"TP_BASIS_VEC": "2", "TP_MD_CHUNK": "4"},
                                 {"TP_BASIS_VEC": "1", "TP_MD_CHUNK": "4"}],
                         ids=["pipe0", "pin0", "graph0", "chunk4", "vec2", "vec1", "vec2_chunk4", "vec1_chunk4"])
def test_env_switches(tmp_path_factory, env):
    """TP_FGMRES_PIPE=0 (no speculative application: v_{j+1} is scaled with the norm from the host), TP_PIN=0 (the sums are copied
    to the host, which also rules out pipelining) and TP_GRAPH=0 (eager pc_apply) change no arithmetic: iterations, cycles,
    the returned norm and x are bitwise those of the default.  TP_MD_CHUNK=4 gives a wave half the entries, so the sums group
    differently: parity tolerance and +-1 iteration.  TP_BASIS_VEC = 2 / 1 (8- and 4-byte loads of the fp32 basis instead of 16-byte
    ones: the lane mappings that were measured against the default) give a lane other entries of its wave's chunk, so the
    sums group differently as well: the same tolerance.  Both inputs are parity inputs, clear of their thresholds."""
    base = run_child(tmp_path_factory, {})
    got = run_child(tmp_path_factory, env)
    names = sorted({k.split(".")[0] for k in base})
    assert names == ["c3_cptr", "c4_cptr"] and sorted(got) == sorted(base)
    for n in names:
        print("env", env, n, "its", int(got[n + ".its"]), "default", int(base[n + ".its"]), "x rel2 %.3e" % rel2(got[n + ".x"], base[n + ".x"]))
        assert int(base[n + ".reason"]) == int(got[n + ".reason"]) == 2 and int(base[n + ".programs"]) == 1
        assert int(got[n + ".programs"]) == (0 if "TP_GRAPH" in env else 1)
        assert int(got[n + ".cycles"]) == int(base[n + ".cycles"]) >= 2
        if "TP_MD_CHUNK" in env or "TP_BASIS_VEC" in env:
            assert abs(int(got[n + ".its"]) - int(base[n + ".its"])) <= 1
            assert rel2(got[n + ".x"], base[n + ".x"]) <= R.PARITY_TOL
        else:
            assert int(got[n + ".its"]) == int(base[n + ".its"]) and float(got[n + ".rnorm"]) == float(base[n + ".rnorm"])
            assert np.array_equal(got[n + ".x"].view(np.uint64), base[n + ".x"].view(np.uint64))
