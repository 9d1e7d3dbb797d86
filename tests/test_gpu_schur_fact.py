"""Factorisation types of the Schur split on (p,T) on the GPU (schur_fact / schur_scale) against the numpy
reference tests/schur_fact_ref.py, which composes the oracle's own V-cycles, coupling mat-vecs and decoupling.

Set-up as in test_gpu_pc_order.py: perturbed_state(seed=5, amp=0.3), dt 8640, rng(11) for the vectors.  Tolerances are the
file-wide bars of test_gpu_parity.py / test_gpu_pc_order.py: rel2 < 1e-10 for an application, and for FGMRES reason 2 on both
sides, iteration counts within 1, rel2(d) < 1e-6.

The structural identities are BITWISE: the variants re-sequence the kernels of the full factorisation on the same inputs (another
output buffer where K(A00) writes y0 directly), every kernel of the cycles sums in a fixed order, and the scale of diag is one
fp64 multiplication per entry."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import cases
import schur_fact_ref as SR
from switches import run_child

pytestmark = pytest.mark.gpu

VARIANTS = ("lower", "upper", "diag")
C4 = "c4_spe10_3d"
EDGE = [("deg_1x5x7", C4, dict(Nx=1, Ny=5, Nz=7, nphase=2), dict(pc="cptr")),
        ("deg_2x2x2", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cptr")),
        ("tinyplane_3x14x2", C4, dict(Nx=3, Ny=14, Nz=2, nphase=2), dict(pc="cptr")),                         # a plane of 6 cells
        ("blocks_20x26x18", C4, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr"))]                       # 9360 cells: > 8 x 256, no multiple of either
SYS = {s[0]: s for s in SR.SYSTEMS}


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


@functools.lru_cache(maxsize=None)
def _oracle(builder, kw, opts, nslabs=1):
    """One oracle system per (case, options), shared by every test that needs it and never modified."""
    return SR.oracle_system(builder, dict(kw), dict(opts), nslabs=nslabs)


def oracle(builder, kw, opts, nslabs=1):
    return _oracle(builder, tuple(sorted(kw.items())), tuple(sorted(opts.items())), nslabs)


def engine(spec, u0, u, opts, **extra):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, dict(opts, **extra))
    h.set_old(u0)
    h.set_dt(SR.DT)
    h.set_state(u)
    h.jacobian()
    h.pc_setup()
    return h


def switch(h, **kw):
    h.set_options(**kw)
    h.pc_setup()


def rand(u, seed=11):
    return np.random.default_rng(seed).standard_normal(u.shape)


# ---- 1. application parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,kw,opts", SR.SYSTEMS + EDGE, ids=[c[0] for c in SR.SYSTEMS + EDGE])
def test_applications_match_the_reference(name, builder, kw, opts):
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    h.vec_set("x", x)
    for fact in VARIANTS:
        switch(h, schur_fact=fact)
        h.stage1_apply("x", "y1")
        e1 = rel2(h.vec_get("y1"), SR.stage1_fact(o.pc, x, fact))
        h.pc_apply("x", "y")
        first = h.vec_get("y")
        e2 = rel2(first, SR.apply_fact(o.pc, "SI", x, fact))
        print("apply", name, fact, "stage1 rel2 = %.3e" % e1, "pc_apply rel2 = %.3e" % e2)
        assert e1 < 1e-10 and e2 < 1e-10, (name, fact, e1, e2)
        h.pc_apply("x", "y")                                # the replay of the recorded program
        assert np.array_equal(h.vec_get("y"), first)
        assert np.array_equal(h.vec_get("x"), x)            # decoupling "No": the right-hand sides ARE x; nothing may write them
    h.close()


# ---- 2. structure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4_2ph_cptr", "c4_2ph_cptrQI", "c3_1ph_cd", "c3_1ph_selfp"])
def test_structure_of_the_sequences(name):
    _, builder, kw, opts = SYS[name]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    h.vec_set("x", x)
    # the stage's right-hand sides, as the library forms them: decoupling "No": x itself; else [x - J 0] decoupled (tp_stage_rhs)
    h.vec_set("r", x)
    if opts.get("decoup", "No") != "No":
        h.vec_set("zero", np.zeros_like(x))
        h.stage_rhs("x", "zero", "r")
        r0, r1 = SR.stage1_rhs(o.pc, x)
        assert rel2(h.vec_get("r")[:2], np.array([r0, r1])) < 1e-12
    y = {}
    for fact in SR.FACTS:
        switch(h, schur_fact=fact)
        h.stage1_apply("x", "y")
        y[fact] = h.vec_get("y")
    # lower: y1 is full's y1, y0 is one cycle of the pressure hierarchy on r0 -- bitwise
    h.amg_vcycle(0, "r", 0, "v", 0)
    assert np.array_equal(y["lower"][1], y["full"][1])
    assert np.array_equal(y["lower"][0], h.vec_get("v")[0])
    assert not np.array_equal(y["lower"][0], y["full"][0])
    # upper: y1 is the KS cycle on r1 -- bitwise (selfp's KS, a cycle and a Jacobi sweep, is not exported: against the reference)
    if opts.get("schur_selfp"):
        assert rel2(y["upper"][1], SR.ks_of(o.pc)(SR.stage1_rhs(o.pc, x)[1])) < 1e-10
    else:
        h.amg_vcycle(1, "r", 1, "v", 1)
        assert np.array_equal(y["upper"][1], h.vec_get("v")[1])
    assert not np.array_equal(y["upper"][1], y["full"][1])
    # diag: y0 is lower's, y1 is schur_scale times upper's -- bitwise, for the default -1 and for 0.5
    assert np.array_equal(y["diag"][0], y["lower"][0]) and np.array_equal(y["diag"][1], -1.0*y["upper"][1])
    switch(h, schur_fact="diag", schur_scale=0.5)
    h.stage1_apply("x", "y")
    assert np.array_equal(h.vec_get("y")[1], 0.5*y["upper"][1]) and np.array_equal(h.vec_get("y")[0], y["lower"][0])
    assert h.schur_info()["scale"] == 0.5 and h.schur_info()["fact"] == "diag"
    assert all(not y[f][2:].any() for f in SR.FACTS)
    h.close()


@pytest.mark.parametrize("name", ["c4_2ph_cptr", "c3_1ph_cd"])
def test_counters_and_vcycles(name):
    _, builder, kw, opts = SYS[name]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, dict(opts, ksp_rtol=1e-8, snes_max_it=25))
    h.vec_set("x", x)
    n = 3
    for fact in SR.FACTS:
        switch(h, schur_fact=fact, schur_scale=-1.0)
        info = h.schur_info()
        assert (info["fact"], info["scale"], info["k0_applies"], info["ks_applies"]) == (fact, -1.0, 0, 0)      # since the set-up
        for _ in range(n):                                  # recorded once, replayed twice
            h.pc_apply("x", "y")
        info = h.schur_info()
        assert (info["k0_applies"], info["ks_applies"]) == ((2*n, n) if fact == "full" else (n, n)), (fact, info)
        h.stage1_apply("x", "y")                            # issued eagerly
        info = h.schur_info()
        assert (info["k0_applies"], info["ks_applies"]) == ((2*n + 2, n + 1) if fact == "full" else (n + 1, n + 1)), (fact, info)
    # tp_solve_info.vcycles follows vcycles_per_apply: 3 per used application under full, 2 under the others.  A context's count
    # runs on over its solves (test_gpu_pc_order.test_sis_accounting)
    last = None
    for fact in SR.FACTS + ("full",):
        switch(h, schur_fact=fact)
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(86.4)
        r = h.newton_solve()
        assert r["reason"] > 0 and r["lits"] > 0, (fact, r)
        if last is not None:
            assert r["vcycles"] - last == (3 if fact == "full" else 2)*r["lits"], (fact, r, last)
        last = r["vcycles"]
    h.close()


def test_eager_applications_count_alike():
    """Without the recording (TP_GRAPH=0 is read once per process: tests/schur_fact_env_check.py in a child) the counters and the
    results are the same."""
    run_child("schur_fact_env_check.py", {"TP_GRAPH": "0"}, timeout=300)


# ---- 3. FGMRES ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4_2ph_cptr", "c4_2ph_cptr_a11", "c4_2ph_cptrQI", "c3_1ph_cd"])
def test_fgmres_under_every_fact_type(name):
    _, builder, kw, opts = SYS[name]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts)
    h.residual()
    h.copy_residual_to("b")
    for i, fact in enumerate(SR.FACTS):
        switch(h, schur_fact=fact)
        its_h, reason_h, _ = h.fgmres("b", "d")
        d_o, its_o, reason_o = SR.fgmres_fact(o, J, F, fact)
        e = rel2(h.vec_get("d"), d_o)
        print("fgmres", name, fact, "gpu", its_h, "oracle", its_o, "rel2(d) = %.3e" % e)
        assert its_o == SR.COUNTS[name][i]
        assert reason_h == reason_o == 2 and abs(its_h - its_o) <= 1, (fact, its_h, its_o)
        assert e < 1e-6, (fact, e)
    h.close()


# ---- 4. the default is untouched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4_2ph_cptr", "c3_1ph_selfp"])
def test_explicit_full_is_bit_identical(name):
    _, builder, kw, opts = SYS[name]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    res = []
    for extra in ({}, {"schur_fact": "full"}, {"schur_fact": "full", "schur_scale": -1.0}):
        h = engine(spec, u0, u, dict(opts, ksp_rtol=1e-8, snes_max_it=25), **extra)
        h.vec_set("x", x)
        h.pc_apply("x", "y")
        y = h.vec_get("y")
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(86.4)
        r = h.newton_solve()
        res.append((y, h.get_state(), r["nits"], r["lits"], r["reason"], r["fnorm"], r["vcycles"]))
        h.close()
    a = res[0]
    assert a[4] > 0 and rel2(a[0], o.pc.apply(x)) < 1e-10
    for b in res[1:]:
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 5. options on a live context ---------------------------------------------------------------------------------------------
def test_set_options_switches_the_programs_and_a_refusal_leaves_the_context_usable():
    from thermalporous_amd.engine import HipEngine
    _, builder, kw, opts = SYS["c4_2ph_cptr"]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    h.vec_set("x", x)
    got = []
    for fact in ("full", "lower", "diag", "full"):
        switch(h, schur_fact=fact)
        h.pc_apply("x", "y")                                # the same vector pair every time: a stale program would be replayed
        got.append(h.vec_get("y"))
        e = rel2(got[-1], SR.apply_fact(o.pc, "SI", x, fact))
        print("switch", fact, "rel2 = %.3e" % e)
        assert e < 1e-10, (fact, e)
    assert np.array_equal(got[3], got[0])
    assert rel2(got[1], got[0]) > 1e-6 and rel2(got[2], got[1]) > 1e-6
    # (tp_set_options asks for a new set-up whatever changed: an application without one is refused, not served from a stale program)
    h.set_options(schur_fact="upper")
    with pytest.raises(Exception, match="pc_setup"):
        h.pc_apply("x", "y")
    switch(h, schur_fact="full")
    # refused by the host layer ...
    with pytest.raises(NotImplementedError, match=r"schur_fact.*cpr"):
        h.set_options(pc="cpr", schur_fact="lower")
    with pytest.raises(ValueError, match="schur_fact"):
        h.set_options(schur_fact="left")
    with pytest.raises(ValueError, match=r"schur_scale.*schur_fact"):
        h.set_options(schur_scale=0.5)
    assert h.opts["schur_fact"] == "full" and h.opts["pc"] == "cptr"
    # ... and by the library itself, naming both options; the context keeps its options and its set-up
    for pc, kind in (("cpr", 0), ("cptramg", 3), ("bilu", 4)):
        bad = HipEngine._make_options(dict(h.opts, pc=pc))
        bad.schur_fact = 1
        assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0
        msg = h.lib.tp_last_error().decode()
        assert "schur_fact" in msg and "pc_kind %d" % kind in msg, msg
    bad = HipEngine._make_options(dict(h.opts, pc="fieldsplit_cd", schur_a11=True, fs_additive=True))
    bad.schur_fact = 3
    assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0
    msg = h.lib.tp_last_error().decode()
    assert "schur_fact" in msg and "fs_additive" in msg, msg
    for field, value in (("schur_fact", 4), ("schur_fact", -1), ("schur_scale", float("nan")), ("schur_scale", 0.5)):
        bad = HipEngine._make_options(h.opts)
        setattr(bad, field, value)
        assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0 and field in h.lib.tp_last_error().decode(), (field, value)
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), got[0])
    h.close()
    # a cpr engine refuses the key and goes on
    spec1, u01, u1, o1, J1, F1 = oracle(builder, kw, dict(pc="cpr"))
    h = engine(spec1, u01, u1, dict(pc="cpr"))
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    before = h.vec_get("y")
    with pytest.raises(NotImplementedError, match=r"schur_fact.*cpr"):
        h.set_options(schur_fact="lower")
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), before) and rel2(before, o1.pc.apply(x)) < 1e-10
    h.close()


# ---- 6. combinations ------------------------------------------------------------------------------------------------------------
def test_combinations():
    import ctr_ref as CR
    import pc_order_ref as PR
    from test_gpu_inner import Composed
    _, builder, kw, opts = SYS["c4_2ph_cptr"]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts, schur_fact="lower", pc_order="SIS")
    h.vec_set("x", x)
    h.residual()
    h.copy_residual_to("b")
    # lower with pc_order SIS: both S stages use the factorisation
    h.pc_apply("x", "y")
    e = rel2(h.vec_get("y"), SR.apply_fact(o.pc, "SIS", x, "lower"))
    print("lower + SIS rel2 = %.3e" % e)
    assert e < 1e-10, e
    info = h.schur_info()
    assert (info["k0_applies"], info["ks_applies"]) == (2, 2)
    # lower with pc_ctr
    switch(h, pc_order="SI", pc_ctr=True)
    h.pc_apply("x", "y")
    e = rel2(h.vec_get("y"), CR.apply_seq(SR.FactPC(o.pc, "lower"), CR.make_ctr_amg(o.pc), "SIT", x))
    print("lower + pc_ctr rel2 = %.3e" % e)
    assert e < 1e-10, e
    # upper with an inner solve: ONE inner solve per application
    switch(h, pc_ctr=False, schur_fact="upper", s1_ksp="fgmres", s1_max_it=3)
    h.pc_apply("x", "y")
    e = rel2(h.vec_get("y"), SR.apply_fact(o.pc, "SI", x, "upper", k0=Composed(o.pc, "fgmres", 3).K))
    print("upper + s1 fgmres(3) rel2 = %.3e" % e)
    assert e < 1e-10, e
    assert h.inner_stats()[0] == 1
    h.pc_apply("x", "y")
    assert h.inner_stats()[0] == 2
    switch(h, schur_fact="full")
    h.pc_apply("x", "y")
    assert h.inner_stats()[0] == 2                          # (counted since the set-up) full: two per application
    # lower with BiCGStab: the project's bars for that solver (tests/test_gpu_bcgs.py)
    import bcgs_ref as BR
    switch(h, schur_fact="lower", s1_ksp="preonly", s1_max_it=1, ksp="bcgs")
    its, reason, rn = h.bcgs("b", "d")
    d_o, its_o, reason_o, hist = BR.bcgs_ref(lambda v: SR.la.spmv_block(J, v), lambda v: SR.apply_fact(o.pc, "SI", v, "lower"), F,
                                             rtol=o.opts["ksp_rtol"], maxit=o.opts["ksp_max_it"])
    e = rel2(h.vec_get("d"), d_o)
    tr = np.linalg.norm((F - SR.la.spmv_block(J, h.vec_get("d"))).ravel())
    print("lower + bcgs", "gpu", its, "ref", its_o, "rel2(d) = %.3e" % e, "true res / tol = %.3f" % (tr/(o.opts["ksp_rtol"]*np.linalg.norm(F))))
    assert reason == reason_o == 2 and abs(its - its_o) <= 1, (its, its_o, reason, reason_o)
    assert e <= BR.PARITY_TOL and tr <= 2*o.opts["ksp_rtol"]*np.linalg.norm(F)
    h.close()


# ---- 7. several slabs -----------------------------------------------------------------------------------------------------------
def run_on_slabs(spec, u0, u, opts, x, nranks):
    """pc_setup on every slab of an in-process group, then pc_apply of the global vector x and FGMRES on J d = F: the global
    results (as tests/test_gpu_pc_order.py sets its groups up)."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    out, err = [None]*nranks, []

    def worker(rank):
        try:
            h = E.HipEngine(spec, opts, rank=rank, nranks=nranks, local_group=group)
            h.set_old(u0)
            h.set_dt(SR.DT)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
            h.vec_set("x", x)
            h.pc_apply("x", "y")
            y = h.vec_get("y")
            h.residual()
            h.copy_residual_to("b")
            its, reason, _ = h.fgmres("b", "d")
            out[rank] = (y, h.vec_get("d"), its, reason, h.amg_layout(0)[0])
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    assert len({(o[2], o[3]) for o in out}) == 1
    return (np.concatenate([o[0] for o in out], axis=-3), np.concatenate([o[1] for o in out], axis=-3), out[0][2], out[0][3], out[0][4])


@pytest.mark.parametrize("gather", [-1, 400], ids=["replicated", "distributed"])
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("fact", ["lower", "upper"])
def test_fact_types_on_slabs(fact, nranks, gather):
    _, builder, kw, opts = SYS["c4_2ph_cptr"]               # 7 x 13 x 9 two-phase pc_cptr: 819 cells, level 0 above 400
    spec, u0, u, o, J, F = oracle(builder, kw, opts, nslabs=nranks)
    x = rand(u)
    y, d, its, reason, dist_levels = run_on_slabs(spec, u0, u, dict(opts, schur_fact=fact, amg_gather_cells=gather), x, nranks)
    assert (dist_levels > 0) == (gather > 0)                # the replicated and the slab-distributed stage-1 hierarchy
    err = rel2(y, SR.apply_fact(o.pc, "SI", x, fact))
    d_o, its_o, reason_o = SR.fgmres_fact(o, J, F, fact)
    print("slabs", fact, nranks, gather, "rel2 = %.3e" % err, "its", its, its_o, "rel2(d) = %.3e" % rel2(d, d_o))
    assert err < 1e-10, (fact, nranks, gather, err)
    assert reason == reason_o == 2 and abs(its - its_o) <= 1, (its, its_o)
    assert rel2(d, d_o) < 1e-6


# ---- 8. the time loop -----------------------------------------------------------------------------------------------------------
def _compare_runs(make):
    res = []
    for factory in (SR.reference_engine("lower"), None):
        m = make(factory)
        assert m.engine_opts["schur_fact"] == "lower"
        m.solve()
        assert m.failed_solves == 0 and m.total_lits > 0
        res.append((list(m.nits_vec), list(m.lits_vec)))
        if factory is None:
            info = m.engine.schur_info()
            assert info["fact"] == "lower" and info["k0_applies"] == info["ks_applies"] > 0
            m.engine.close()
    print("time loop: reference", res[0], "gpu", res[1])
    assert res[0][0] == res[1][0]
    # (lits_vec sums the Krylov iterations of a step's Newton iterations: +-1 per linear solve)
    assert len(res[0][1]) == len(res[1][1]) and all(abs(a - b) <= max(1, n) for a, b, n in zip(res[0][1], res[1][1], res[0][0]))


def test_time_loop_two_phase_pc_cptr_lower():
    from oracle.engine import OracleEngine
    from thermalporous_amd.twophase import TwoPhase
    spec, u0, p, g, c = cases.c3_spe10_2d(14, 19, 2)
    m = TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters="pc_cptr", filename=None, verbosity=False, _engine_factory=OracleEngine)
    sp = {**m.solver_parameters, "sub_0_cpr_stage1_pc_fieldsplit_schur_fact_type": "lower"}

    def make(factory):
        spec, u0, p, g, c = cases.c3_spe10_2d(14, 19, 2)
        return TwoPhase(g, c, p, end=0.006, maxdt=0.002, solver_parameters=dict(sp), filename=None, verbosity=False, _engine_factory=factory)
    _compare_runs(make)


def test_time_loop_single_phase_reference_script_dict():
    from test_schur_fact_host import REF_SCRIPT_CD
    sp = {"snes_type": "newtonls", "snes_monitor": True, "snes_converged_reason": True, "snes_max_it": 15, "ksp_type": "fgmres",
          "ksp_converged_reason": True, "ksp_view": False, "ksp_max_it": 200, "ksp_rtol": 1e-10, **REF_SCRIPT_CD}

    def make(factory):
        spec, u0, p, g, c = cases.c3_spe10_2d(Nx=14, Ny=19, nphase=1)
        return SinglePhaseOf(g, c, p, sp, factory)
    _compare_runs(make)


def SinglePhaseOf(g, c, p, sp, factory):
    from thermalporous_amd.singlephase import SinglePhase
    return SinglePhase(g, c, p, end=0.5, maxdt=0.25, small_dt_start=False, solver_parameters=dict(sp), filename=None, verbosity=False,
                       _engine_factory=factory)
