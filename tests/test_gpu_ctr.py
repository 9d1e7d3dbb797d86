"""The composite's temperature stage on the GPU (pc_ctr) against the numpy reference tests/ctr_ref.py, which
composes the oracle's own stage 1, ILU solve, block SpMV and one SemiAMG V-cycle on the T-T block of the undecoupled Jacobian.

Set-up as in test_gpu_pc_order.py: perturbed_state(seed=5, amp=0.3), dt 8640, rng(11) for the vectors.  Tolerances are that file's
bars: 1e-12 for an SpMV-like kernel (tp_ctr_rhs), 1e-10 for a preconditioner application, and for FGMRES reason 2 on both sides,
iteration counts within 1, rel2(d) < 1e-6.  On the systems used for applications and FGMRES the T cycle contracts (radius <= 0.9 on
the CPU); the 20 x 26 x 18 box, where it does not, is used for the kernel only."""
import ctypes as C
import functools

import numpy as np
import pytest

import ctr_ref as CR
import pc_order_ref as PR

pytestmark = pytest.mark.gpu

C4 = "c4_spe10_3d"


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


@functools.lru_cache(maxsize=None)
def _oracle(builder, kw, opts):
    """One oracle system and its T hierarchy per (case, options), shared by every test that needs it and never modified."""
    spec, u0, u, o, J, F = PR.oracle_system(builder, dict(kw), dict(opts))
    return spec, u0, u, o, J, F, CR.make_ctr_amg(o.pc)


def oracle(builder, kw, opts):
    return _oracle(builder, tuple(sorted(kw.items())), tuple(sorted(opts.items())))


def engine(spec, u0, u, opts, **extra):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, dict(opts, **extra))
    h.set_old(u0)
    h.set_dt(CR.DT)
    h.set_state(u)
    h.jacobian()
    h.pc_setup()
    return h


def switch(h, **kw):
    h.set_options(**kw)
    h.pc_setup()


def rand(u, seed=11, n=1):
    rng = np.random.default_rng(seed)
    out = [rng.standard_normal(u.shape) for _ in range(n)]
    return out[0] if n == 1 else out


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
RHS_CASES = [
    ("2d_1ph", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="cpr", ilu_tile=CR.T2D)),          # 5 slots, b = 2
    ("2d_2ph", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=2), dict(pc="cptr", ilu_tile=CR.T2D)),         # 5 slots, b = 3
    ("3d_2ph", C4, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr")),                                # 7 slots, b = 3
    ("3d_1ph", C4, dict(Nx=7, Ny=13, Nz=9, nphase=1), dict(pc="cpr", decoup="QI")),                    # 7 slots, b = 2
    ("deg_1x5x7", C4, dict(Nx=1, Ny=5, Nz=7, nphase=2), dict(pc="cpr")),
    ("deg_2x2x2", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cpr")),
    ("tinyplane_3x14x2", C4, dict(Nx=3, Ny=14, Nz=2, nphase=2), dict(pc="cpr")),                       # a plane of 6 cells
    ("blocks_20x26x18", C4, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr")),                     # 9360 cells: > 8 x 256, no multiple of either
]


@pytest.mark.parametrize("name,builder,kw,opts", RHS_CASES, ids=[c[0] for c in RHS_CASES])
def test_ctr_rhs_kernel(name, builder, kw, opts):
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts, pc_ctr=True)
    x, y = rand(u, n=2)                                     # y random in ALL fields
    h.vec_set("x", x)
    h.vec_set("y", y)
    h.vec_set("out", np.full(u.shape, 7.0))
    h.ctr_rhs("x", "y", "out")
    got, ref = h.vec_get("out"), CR.row_rhs_ref(o.pc, x, y)
    err = rel2(got[1], ref)
    print("ctr_rhs", name, "rel2 = %.3e" % err)
    assert err < 1e-12, (name, err)
    assert np.all(got[0] == 7.0) and np.all(got[2:] == 7.0)  # only plane 1 is written
    assert np.array_equal(h.vec_get("x"), x) and np.array_equal(h.vec_get("y"), y)
    for a, b, c in (("x", "x", "out"), ("x", "y", "y"), ("x", "y", "x")):
        with pytest.raises(Exception, match="must differ"):
            h.ctr_rhs(a, b, c)
    h.close()


# ---- 2. the stage on its own ---------------------------------------------------------------------------------------------------
CTR_APPLY_CASES = [CR.TABLE[2], CR.TABLE[1], ("deg_2x2x2", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cpr"))]


@pytest.mark.parametrize("name,builder,kw,opts", CTR_APPLY_CASES, ids=[c[0] for c in CTR_APPLY_CASES])
def test_ctr_apply_is_one_vcycle_on_the_temperature_block(name, builder, kw, opts):
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts, pc_ctr=True)
    x = rand(u)
    h.vec_set("x", x)
    h.vec_set("y", np.full(u.shape, 7.0))
    h.ctr_apply("x", "y")
    got = h.vec_get("y")
    err = rel2(got[1], amgT.vcycle(x[1]))
    print("ctr_apply", name, "rel2 = %.3e" % err)
    assert err < 1e-10, (name, err)
    assert not got[0].any() and not got[2:].any()            # every other field is exactly zero
    assert np.array_equal(h.vec_get("x"), x)
    with pytest.raises(Exception, match="must differ"):
        h.ctr_apply("x", "x")
    h.close()


def test_exports_refuse_without_the_option_or_the_setup():
    name, builder, kw, opts = CR.TABLE[2]
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts)
    for v in ("x", "y", "out"):
        h.vec_set(v, rand(u))
    for call in (lambda: h.ctr_rhs("x", "y", "out"), lambda: h.ctr_apply("x", "y"), h.ctr_info):
        with pytest.raises(Exception, match="pc_ctr is off"):
            call()
    h.set_options(pc_ctr=True)                              # on, but not set up yet
    for call in (lambda: h.ctr_rhs("x", "y", "out"), lambda: h.ctr_apply("x", "y"), h.ctr_info):
        with pytest.raises(Exception, match="not set up"):
            call()
    h.pc_setup()
    assert h.ctr_info()["enabled"]
    h.close()


# ---- 3. pc_apply against the reference sequence ---------------------------------------------------------------------------------
APPLY_CASES = [(n, b, kw, opts, CR.SEQS) for n, b, kw, opts in CR.TABLE] + \
              [("deg_2x2x2_cpr", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cpr"), CR.SEQS),
               PR.PARITY[4] + (("SIT",),)]


@pytest.mark.parametrize("name,builder,kw,opts,seqs", APPLY_CASES, ids=[c[0] for c in APPLY_CASES])
def test_pc_apply_matches_the_reference_sequence(name, builder, kw, opts, seqs):
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts, pc_ctr=True)
    h.vec_set("x", x)
    for seq in seqs:
        if seq != "SIT":
            switch(h, pc_order=CR.ORDER_OF[seq])
        h.pc_apply("x", "y")
        first = h.vec_get("y")
        err = rel2(first, CR.apply_seq(o.pc, amgT, seq, x))
        print("pc_apply", name, seq, "rel2 = %.3e" % err)
        assert err < 1e-10, (name, seq, err)
        h.pc_apply("x", "y")                                # the replay of the recorded program
        assert np.array_equal(h.vec_get("y"), first)
    h.close()


# ---- 4. the same sequence composed from the exported stages ------------------------------------------------------------------
def test_pc_apply_is_the_composition_of_the_exported_stages():
    name, builder, kw, opts = CR.TABLE[2]                   # 9 x 10 x 5 two-phase
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts, pc_ctr=True)
    for seq in CR.SEQS:
        switch(h, pc_order=CR.ORDER_OF[seq])
        h.vec_set("x", x)
        h.pc_apply("x", "y")
        got = h.vec_get("y")
        y = np.zeros_like(x)
        for k, s in enumerate(seq):
            r = x
            if k:
                h.vec_set("t", y)
                h.spmv("t", "jt")
                r = x - h.vec_get("jt")
            h.vec_set("r", r)
            {"S": h.stage1_apply, "I": h.ilu_solve, "T": h.ctr_apply}[s]("r", "e")
            y = y + h.vec_get("e")
        err = rel2(got, y)
        print("self-composition", seq, "rel2 = %.3e" % err)
        assert err < 1e-10, (seq, err)
    h.close()


# ---- 5. FGMRES --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,kw,opts", CR.TABLE, ids=[c[0] for c in CR.TABLE])
def test_fgmres_under_every_sequence(name, builder, kw, opts):
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts, pc_ctr=True)
    h.residual()
    h.copy_residual_to("b")
    for seq in CR.SEQS:
        switch(h, pc_order=CR.ORDER_OF[seq])
        its_h, reason_h, _ = h.fgmres("b", "d")
        d_o, its_o, reason_o = CR.fgmres_seq(o, amgT, J, F, seq)
        print("fgmres", name, seq, "gpu", its_h, "oracle", its_o)
        assert its_o == CR.count(name, seq)
        assert reason_h == reason_o == 2 and abs(its_h - its_o) <= 1, (seq, its_h, its_o)
        assert rel2(h.vec_get("d"), d_o) < 1e-6
    h.close()


# ---- 6. options on a live context ------------------------------------------------------------------------------------------------
def test_set_options_switches_the_programs_and_a_refusal_leaves_the_context_usable():
    from thermalporous_amd.engine import HipEngine
    name, builder, kw, opts = CR.TABLE[2]
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    y_off = h.vec_get("y")
    assert rel2(y_off, o.pc.apply(x)) < 1e-10
    switch(h, pc_ctr=True)
    h.pc_apply("x", "y")                                    # the same vector pair: the recorded SI program must not be replayed
    y_on = h.vec_get("y")
    assert rel2(y_on, CR.apply_seq(o.pc, amgT, "SIT", x)) < 1e-10
    # "on" differs by more than 1e-3 where the stage writes: the temperature field.  (The reference alone, SIT against SI on this
    # system: 74 on the T field, 0 on the other two, 1.3e-4 over the whole vector, whose norm the untouched pressure carries --
    # at most 1.3e-4 on every system of the table, so the whole-vector figure cannot tell on from off at 1e-3.)
    assert rel2(y_on[1], y_off[1]) > 1e-3
    assert np.array_equal(y_on[0], y_off[0]) and np.array_equal(y_on[2], y_off[2])      # T runs last and adds into field 1 only
    switch(h, pc_ctr=False)
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y_off)
    # refused by the host layer ...
    with pytest.raises(NotImplementedError, match=r"pc_ctr.*cptramg"):
        h.set_options(pc="cptramg", pc_ctr=True)
    with pytest.raises(ValueError, match="pc_ctr"):
        h.set_options(pc_ctr=2)
    # ... and by the library itself, naming both options; the context keeps its options and its set-up
    for pc, kind in (("cptramg", 3), ("bilu", 4), ("fieldsplit_cd", 2)):
        bad = HipEngine._make_options(dict(h.opts, pc=pc, decoup="No"))
        bad.pc_ctr = 1
        assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0
        msg = h.lib.tp_last_error().decode()
        assert "pc_ctr" in msg and "pc_kind %d" % kind in msg, msg
    bad = HipEngine._make_options(h.opts)
    bad.pc_ctr = 2
    assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0 and "pc_ctr" in h.lib.tp_last_error().decode()
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y_off)
    h.close()


def test_more_than_one_slab_is_refused_by_both_layers():
    from thermalporous_amd import engine as E
    name, builder, kw, opts = CR.TABLE[2]
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    with pytest.raises(NotImplementedError, match=r"pc_ctr.*nranks = 2"):
        E.HipEngine(spec, dict(opts, pc_ctr=True), rank=0, nranks=2)
    # the library: tp_create with a two-slab grid
    h = E.HipEngine(spec, opts)
    n0, n1, gn2 = (int(v) for v in spec["n"])
    g = E.tp_grid(n0, n1, gn2 - gn2//2, gn2, gn2//2, (C.c_double*3)(*[float(v) for v in spec["h"]]), int(spec["gaxis"]), h.nph, 1, 2)
    prm = E.tp_params(*[float(spec["prm"][k]) for k in E.tp_params._names])
    bad = E.HipEngine._make_options(h.opts)
    bad.pc_ctr = 1
    ctx = C.c_void_p()
    assert h.lib.tp_create(C.byref(g), C.byref(prm), C.byref(bad), 0, C.byref(ctx)) != 0
    msg = h.lib.tp_last_error().decode()
    assert "pc_ctr" in msg and "nranks" in msg, msg
    h.close()


# ---- 7. accounting ------------------------------------------------------------------------------------------------------------
def test_vcycle_accounting_and_ctr_info():
    builder, kw, opts = C4, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cpr")
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, dict(opts, ksp_rtol=1e-8, snes_max_it=25), pc_ctr=True)
    info = h.ctr_info()
    assert info["enabled"] and info["levels"] >= 2 and info["setups"] == 1 and info["applies"] == 0, info
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    assert rel2(h.vec_get("y"), CR.apply_seq(o.pc, amgT, "SIT", x)) < 1e-10
    assert h.ctr_info()["applies"] == 1
    h.ctr_apply("x", "y")
    assert h.ctr_info()["applies"] == 2
    # one Newton solve: one S and one T V-cycle per application; the context's count runs on over the application above
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(86.4)
    r = h.newton_solve()
    assert r["reason"] > 0 and r["lits"] > 0 and r["vcycles"] == 2*(1 + r["lits"]), r
    info = h.ctr_info()
    # launched applications: the Krylov iterations plus at most one discarded speculative application per linear solve
    assert 2 + r["lits"] <= info["applies"] <= 2 + r["lits"] + r["nits"], (info, r)
    assert info["setups"] > 1, info
    h.close()


# ---- 8. the default is untouched ---------------------------------------------------------------------------------------------
def test_explicit_false_is_bit_identical_to_the_key_being_absent():
    name, builder, kw, opts = CR.TABLE[3]
    spec, u0, u, o, J, F, amgT = oracle(builder, kw, opts)
    x = rand(u)
    res = []
    for extra in ({}, {"pc_ctr": False}):
        h = engine(spec, u0, u, dict(opts, ksp_rtol=1e-8, snes_max_it=25), **extra)
        h.vec_set("x", x)
        h.pc_apply("x", "y")
        y = h.vec_get("y")
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(86.4)
        r = h.newton_solve()
        res.append((y, h.get_state(), {k: r[k] for k in ("nits", "lits", "reason", "fnorm", "vcycles")}))
        h.close()
    a, b = res
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (a[2], b[2])
    assert rel2(a[0], o.pc.apply(x)) < 1e-10
