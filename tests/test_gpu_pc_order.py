"""Stage orders of the composite preconditioner on the GPU (pc_order) against the numpy reference
tests/pc_order_ref.py, which composes the oracle's own stage 1, ILU solve and block SpMV.

Set-up as in test_gpu_parity.test_linear_stages_parity: perturbed_state(seed=5, amp=0.3), dt 8640, rng(11) for the vectors.
Tolerances are the file-wide bars of test_gpu_parity.py: 1e-12 for an SpMV-like kernel (tp_stage_rhs; 1e-10 with the _temp
decoupling, whose coefficients pass through a 2x2 inverse), 1e-10 for a preconditioner application, and for FGMRES reason 2 on
both sides, iteration counts within 1, rel2(d) < 1e-6."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import cases
import pc_order_ref as PR

pytestmark = pytest.mark.gpu

LATER = ("IS", "ISI", "SIS")
T2D = (1 << 30, 64, 1)


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


@functools.lru_cache(maxsize=None)
def _oracle(builder, kw, opts, nslabs=1):
    """One oracle system per (case, options), shared by every test that needs it and never modified."""
    return PR.oracle_system(builder, dict(kw), dict(opts), nslabs=nslabs)


def oracle(builder, kw, opts, nslabs=1):
    return _oracle(builder, tuple(sorted(kw.items())), tuple(sorted(opts.items())), nslabs)


def engine(spec, u0, u, opts, **extra):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, dict(opts, **extra))
    h.set_old(u0)
    h.set_dt(PR.DT)
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
C4 = "c4_spe10_3d"
RHS_CASES = [
    ("2d_1ph_cpr_No", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="cpr", ilu_tile=T2D), 1e-12),       # 5 slots, b = 2, npri 1
    ("2d_2ph_cptr", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=2), dict(pc="cptr", ilu_tile=T2D), 1e-12),       # b = 3, npri 2
    ("3d_2ph_cpr_QI", C4, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cpr", decoup="QI"), 1e-12),              # 7 slots, one secondary row
    ("3d_2ph_cpr_QItemp", C4, dict(Nx=9, Ny=10, Nz=5, nphase=2), dict(pc="cpr", decoup="QI_temp"), 1e-10),     # both secondary rows
    ("3d_2ph_cptr_QI", C4, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", decoup="QI"), 1e-12),            # npri 2 and a secondary row
    ("3d_1ph_cpr_QI", C4, dict(Nx=7, Ny=13, Nz=9, nphase=1), dict(pc="cpr", decoup="QI"), 1e-12),              # b = 2 with a secondary row
    ("deg_1x5x7", C4, dict(Nx=1, Ny=5, Nz=7, nphase=2), dict(pc="cptr"), 1e-12),
    ("deg_2x2x2", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cptr"), 1e-12),
    ("tinyplane_3x14x2", C4, dict(Nx=3, Ny=14, Nz=2, nphase=2), dict(pc="cptr"), 1e-12),                       # a plane of 6 cells
    ("blocks_20x26x18", C4, dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr"), 1e-12),                      # 9360 cells: > 8 x 256, no multiple of either
]


@pytest.mark.parametrize("name,builder,kw,opts,tol", RHS_CASES, ids=[c[0] for c in RHS_CASES])
def test_stage_rhs_kernel(name, builder, kw, opts, tol):
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts)
    x, y = rand(u, n=2)                                     # y random in ALL fields
    npri = 1 if opts["pc"] == "cpr" else 2
    h.vec_set("x", x)
    h.vec_set("y", y)
    h.vec_set("out", np.full(u.shape, 7.0))
    h.stage_rhs("x", "y", "out")
    got, ref = h.vec_get("out"), PR.stage_rhs_ref(o.pc, x, y)
    err = rel2(got[:npri], ref)
    print("stage_rhs", name, "rel2 = %.3e" % err)
    assert ref.shape[0] == npri and err < tol, (name, err)
    assert np.all(got[npri:] == 7.0)                        # only the primary planes are written
    assert np.array_equal(h.vec_get("x"), x) and np.array_equal(h.vec_get("y"), y)
    with pytest.raises(Exception, match="must differ"):
        h.stage_rhs("x", "x", "out")
    h.close()


# ---- 2. pc_apply against the reference sequence ---------------------------------------------------------------------------------
APPLY_CASES = [(n, b, kw, opts) for n, b, kw, opts in PR.PARITY] + [("deg_2x2x2_cptr", C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), dict(pc="cptr"))]


@pytest.mark.parametrize("name,builder,kw,opts", APPLY_CASES, ids=[c[0] for c in APPLY_CASES])
def test_pc_apply_matches_the_reference_sequence(name, builder, kw, opts):
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts, pc_order="IS")
    h.vec_set("x", x)
    for order in LATER:
        if order != "IS":
            switch(h, pc_order=order)
        h.pc_apply("x", "y")
        first = h.vec_get("y")
        err = rel2(first, PR.apply_seq(o.pc, order, x))
        print("pc_apply", name, order, "rel2 = %.3e" % err)
        assert err < 1e-10, (name, order, err)
        h.pc_apply("x", "y")                                # the replay of the recorded program
        assert np.array_equal(h.vec_get("y"), first)
    h.close()


# ---- 3. the same sequence composed from the exported stages ------------------------------------------------------------------
def test_pc_apply_is_the_composition_of_the_exported_stages():
    name, builder, kw, opts = PR.PARITY[0]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    for order in PR.ORDERS:
        switch(h, pc_order=order)
        h.vec_set("x", x)
        h.pc_apply("x", "y")
        got = h.vec_get("y")
        y = np.zeros_like(x)
        for k, s in enumerate(order):
            r = x
            if k:
                h.vec_set("t", y)
                h.spmv("t", "jt")
                r = x - h.vec_get("jt")
            h.vec_set("r", r)
            if s == "S":
                h.stage1_apply("r", "e")
            else:
                h.ilu_solve("r", "e")
            y = y + h.vec_get("e")
        err = rel2(got, y)
        print("self-composition", order, "rel2 = %.3e" % err)
        assert err < 1e-10, (order, err)
    h.close()


# ---- 4. FGMRES --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,kw,opts", PR.PARITY[:3], ids=[c[0] for c in PR.PARITY[:3]])
def test_fgmres_under_every_order(name, builder, kw, opts):
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    h = engine(spec, u0, u, opts)
    h.residual()
    h.copy_residual_to("b")
    for i, order in enumerate(PR.ORDERS):
        switch(h, pc_order=order)
        its_h, reason_h, _ = h.fgmres("b", "d")
        d_o, its_o, reason_o = PR.fgmres_seq(o, J, F, order)
        print("fgmres", name, order, "gpu", its_h, "oracle", its_o)
        assert its_o == PR.COUNTS[name][i]
        assert reason_h == reason_o == 2 and abs(its_h - its_o) <= 1, (order, its_h, its_o)
        assert rel2(h.vec_get("d"), d_o) < 1e-6
    h.close()


# ---- 5. the default is untouched ---------------------------------------------------------------------------------------------
def test_explicit_default_is_bit_identical():
    name, builder, kw, opts = PR.PARITY[0]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    res = []
    for extra in ({}, {"pc_order": "SI"}):
        h = engine(spec, u0, u, opts, **extra)
        h.vec_set("x", x)
        h.pc_apply("x", "y")
        h.residual()
        h.copy_residual_to("b")
        its, reason, rn = h.fgmres("b", "d")
        res.append((h.vec_get("y"), h.vec_get("d"), its, reason, rn))
        h.close()
    a, b = res
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert rel2(a[0], o.pc.apply(x)) < 1e-10


# ---- 6. options on a live context ------------------------------------------------------------------------------------------------
def test_set_options_switches_the_programs_and_a_refusal_leaves_the_context_usable():
    from thermalporous_amd.engine import HipEngine
    name, builder, kw, opts = PR.PARITY[1]
    spec, u0, u, o, J, F = oracle(builder, kw, opts)
    x = rand(u)
    h = engine(spec, u0, u, opts)
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    y_si = h.vec_get("y")
    assert rel2(y_si, o.pc.apply(x)) < 1e-10
    switch(h, pc_order="ISI")
    h.pc_apply("x", "y")                                    # the same vector pair: the recorded SI program must not be replayed
    y_isi = h.vec_get("y")
    assert rel2(y_isi, PR.apply_seq(o.pc, "ISI", x)) < 1e-10 and rel2(y_isi, y_si) > 1e-3
    switch(h, pc_order="SI")
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y_si)
    # refused by the host layer ...
    with pytest.raises(NotImplementedError, match=r"pc_order.*bilu"):
        h.set_options(pc="bilu", pc_order="IS")
    with pytest.raises(ValueError, match="pc_order"):
        h.set_options(pc_order="SSI")
    # ... and by the library itself, naming both options; the context keeps its options and its set-up
    for pc, kind in (("bilu", 4), ("fieldsplit_cd", 2)):
        bad = HipEngine._make_options(dict(h.opts, pc=pc, decoup="No"))
        bad.pc_order = 3
        assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0
        msg = h.lib.tp_last_error().decode()
        assert "pc_order" in msg and "pc_kind %d" % kind in msg, msg
    bad = HipEngine._make_options(h.opts)
    bad.pc_order = 4
    assert h.lib.tp_set_options(h.ctx, C.byref(bad)) != 0 and "pc_order" in h.lib.tp_last_error().decode()
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y_si)
    h.close()


# ---- 7. several slabs ---------------------------------------------------------------------------------------------------------
def run_on_slabs(spec, u0, u, opts, x, nranks):
    """pc_setup on every slab of an in-process group, then pc_apply of the global vector x and FGMRES on J d = F: the global
    results (as tests/test_gpu_slabs.py sets its groups up)."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    out, err = [None]*nranks, []

    def worker(rank):
        try:
            h = E.HipEngine(spec, opts, rank=rank, nranks=nranks, local_group=group)
            h.set_old(u0)
            h.set_dt(PR.DT)
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
@pytest.mark.parametrize("order", ["ISI", "SIS"])
def test_orders_on_slabs(order, nranks, gather):
    name, builder, kw, opts = PR.PARITY[0]                  # 7 x 13 x 9 two-phase pc_cptr: 819 cells, level 0 above 400
    spec, u0, u, o, J, F = oracle(builder, kw, opts, nslabs=nranks)
    x = rand(u)
    y, d, its, reason, dist_levels = run_on_slabs(spec, u0, u, dict(opts, pc_order=order, amg_gather_cells=gather), x, nranks)
    assert (dist_levels > 0) == (gather > 0)                # the replicated and the slab-distributed stage-1 hierarchy
    err = rel2(y, PR.apply_seq(o.pc, order, x))
    d_o, its_o, reason_o = PR.fgmres_seq(o, J, F, order)
    print("slabs", order, nranks, gather, "rel2 = %.3e" % err, "its", its, its_o)
    assert err < 1e-10, (order, nranks, gather, err)
    assert reason == reason_o == 2 and abs(its - its_o) <= 1, (its, its_o)
    assert rel2(d, d_o) < 1e-6


# ---- 8. accounting ------------------------------------------------------------------------------------------------------------
class _Seq:
    """The oracle preconditioner with another stage 1 (an inner solve): what pc_order_ref.apply_seq reads."""

    def __init__(self, pc, stage1):
        self.stage1, self.ilu, self.J = stage1, pc.ilu, pc.J


@pytest.mark.parametrize("name,opts,per_stage", [("cpr_s1_fgmres3", dict(pc="cpr", s1_ksp="fgmres", s1_max_it=3), 3),
                                                 ("cpr_ilu1", dict(pc="cpr", ilu_levels=1), 1),
                                                 ("cptr_s1_richardson2", dict(pc="cptr", s1_ksp="richardson", s1_max_it=2), 5)],
                         ids=["cpr_s1_fgmres3", "cpr_ilu1", "cptr_s1_richardson2"])
def test_sis_accounting(name, opts, per_stage):
    from test_gpu_inner import Composed
    builder, kw = C4, dict(Nx=7, Ny=13, Nz=9, nphase=2)
    base = {k: v for k, v in opts.items() if not k.startswith("s1_")}
    spec, u0, u, o, J, F = oracle(builder, kw, base)
    x = rand(u)
    h = engine(spec, u0, u, dict(opts, ksp_rtol=1e-8, snes_max_it=25), pc_order="SIS")
    ref = _Seq(o.pc, Composed(o.pc, opts.get("s1_ksp", "preonly"), opts.get("s1_max_it", 1)).stage1)
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    err = rel2(h.vec_get("y"), PR.apply_seq(ref, "SIS", x))
    print("SIS", name, "rel2 = %.3e" % err)
    assert err < 1e-10, (name, err)
    if "s1_ksp" in opts:                                    # launched inner solves: K(A00) once per S stage (pc_cptr: twice)
        assert h.inner_stats()[0] == 2*(2 if opts["pc"] == "cptr" else 1)
    # one Newton solve: V-cycles = S stages x the per-stage figure x applications.  A context's count runs on over its solves (as
    # in test_gpu_krylov.test_vcycles_count_only_used_applications): the application above, then one per Krylov iteration
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(86.4)
    r1 = h.newton_solve()
    assert r1["reason"] > 0 and r1["lits"] > 0 and r1["vcycles"] == 2*per_stage*(1 + r1["lits"]), r1
    switch(h, pc_order="SI")
    h.set_state(u0)
    h.set_old(u0)
    r2 = h.newton_solve()
    assert r2["reason"] > 0 and r2["lits"] > 0 and r2["vcycles"] - r1["vcycles"] == per_stage*r2["lits"], (r1, r2)
    h.close()
