"""amg_gs_levels / amg_gs_sweeps on the GPU: red-black Gauss-Seidel on the top levels of the scalar V-cycles (k_amg_gs_first,
k_amg_gs_half) against amg_gs_ref.GsSemiAMG, the oracle's SemiAMG with the smoother restated.

Tolerances are the project's fp64 ones: V-cycle, stage 1 and pc_apply rel <= 1e-10 in the 2-norm, FGMRES counts
+-1, Newton counts equal, states rel <= 1e-8.  Every case asserts from tp_amg_layout / tp_amg_gs_info that it runs the GS levels
it claims and that the red and black cells of level 0 add up to its cells."""
import ctypes as C

import numpy as np
import pytest

import cases
from amg_gs_ref import oracle_engine, red_mask

pytestmark = pytest.mark.gpu

TOL = 1e-10


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def make(builder, kw, opts, dt=8640.0, seed=5, amp=0.3):
    """Reference (oracle with GsSemiAMG hierarchies) and GPU engine at the same perturbed state, both set up."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = builder(**kw)
    o, h = oracle_engine(spec, opts), HipEngine(spec, opts)
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    for e in (o, h):
        e.set_old(u0)
        e.set_dt(dt)
        e.set_state(u)
    schur = opts["pc"] in ("cptr", "fieldsplit_cd")
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    h.jacobian()
    o.pc.setup(J, Sm)
    h.pc_setup()
    return spec, u0, u, o, h, J


def check_layout(o, h, which, spec, levels, sweeps):
    """The GPU's plan is the reference's: `levels` GS levels of `sweeps` sweeps per leg, the colours of level 0 counted from the
    cells' index sums."""
    info = h.amg_gs_info(which)
    ref = o.pc.amg_p if which == 0 else o.pc.amg_T
    assert info["levels"] == levels == ref.n_gs_levels(), (info, ref.n_gs_levels())
    n0, n1, n2 = (int(v) for v in spec["n"])
    if levels:
        red = int(red_mask((n2, n1, n0)).sum())
        assert info["sweeps"] == sweeps == ref.gs_sweeps
        assert (info["red"], info["black"]) == (red, n0*n1*n2 - red), info
        assert info["red"] + info["black"] == n0*n1*n2
    else:
        assert info == dict(levels=0, sweeps=0, red=0, black=0), info
    assert h.amg_layout(which)[1] == list(ref.sched)
    return info


BOX = (cases.c4_spe10_3d, dict(Nx=12, Ny=22, Nz=10, nphase=2))


# (GS levels, sweeps per leg, time step): at dt = 8640 both hierarchies run full cycles; at dt = 8.64 the temperature operator S~ is
# diagonally dominant on level 0 (ratio 0.13 <= amg_dom_tau) and its hierarchy ends there, at a GS level, with B^g F^g 0
@pytest.fixture(scope="module", params=[(1, 1, 8640.0), (2, 1, 8640.0), (2, 2, 8640.0), (2, 1, 8.64)],
                ids=["L1g1", "L2g1", "L2g2", "L2g1_trunc"])
def box(request):
    L, g, dt = request.param
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_gs_levels=L, amg_gs_sweeps=g), dt=dt)
    yield L, g, spec, u0, u, o, h, J
    h.close()


def test_box_layout(box):
    """2640 cells (1320 red, 1320 black); level 1 has 1320 cells, level 2 (660 cells) is the tail, so L = 2 gives two GS levels.  The
    S~ hierarchy coarsens axis 0 first, the pressure hierarchy axis 2.  In the last variant the S~ hierarchy ends with relaxation
    only at level 0, a GS level."""
    L, g, spec, u0, u, o, h, J = box
    for which in (0, 1):
        info = check_layout(o, h, which, spec, L, g)
        assert info["red"] == info["black"] == 1320
        assert h.amg_tail_info(which)["tail_level"] == 2
        assert h.amg_line_info(which)["levels"] == 0
    assert h.amg_layout(1)[1][0] == 0 and h.amg_layout(0)[1][0] == 2
    lv, ratio0 = h.amg_trunc(1)
    want = o.pc.amg_T.trunc
    assert lv == (-1 if want is None else want), (lv, ratio0, want)
    if o.prob.dt < 100.0:                                          # the truncating variant
        assert 0 <= lv < L
    assert h.amg_trunc(0)[0] == -1 and o.pc.amg_p.trunc is None


def test_box_vcycles(box):
    L, g, spec, u0, u, o, h, J = box
    x = np.random.default_rng(11).standard_normal(u.shape)
    h.vec_set("x", x)
    for which, ref in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        h.amg_vcycle(which, "x", which, "y", which)
        d = rel2(h.vec_get("y")[which], ref.vcycle(x[which]))
        print("L=%d g=%d hierarchy %d: V-cycle vs GsSemiAMG %.3e" % (L, g, which, d))
        assert d <= TOL, (which, d)


def test_box_stage1_and_pc_apply(box):
    L, g, spec, u0, u, o, h, J = box
    x = np.random.default_rng(12).standard_normal(u.shape)
    h.vec_set("x", x)
    h.stage1_apply("x", "y")
    h.pc_apply("x", "z")
    d1, d2 = rel2(h.vec_get("y"), o.pc.stage1(x)), rel2(h.vec_get("z"), o.pc.apply(x))
    print("L=%d g=%d: stage 1 %.3e, pc_apply %.3e" % (L, g, d1, d2))
    assert d1 <= TOL and d2 <= TOL, (d1, d2)


def test_box_fgmres(box):
    import oracle.linalg as la
    L, g, spec, u0, u, o, h, J = box
    b = np.random.default_rng(13).standard_normal(u.shape)
    h.vec_set("b", b)
    its, reason, rn = h.fgmres("b", "sol")
    xo, ito, ro, _ = la.fgmres(lambda v: la.spmv_block(J, v), o.pc.apply, b, rtol=o.opts["ksp_rtol"], atol=o.opts["ksp_atol"],
                               restart=o.opts["ksp_restart"], maxit=o.opts["ksp_max_it"])
    print("L=%d g=%d: FGMRES its GPU %d, reference %d; solutions differ by %.3e" % (L, g, its, ito, rel2(h.vec_get("sol"), xo)))
    assert reason > 0 and ro > 0
    assert abs(its - ito) <= 1, (its, ito)


def test_box_newton_solve():
    """From the uniform state at dt 86.4 with L = 2, g = 1: the reference does 4 Newton / 29 Krylov iterations."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = BOX[0](**BOX[1])
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, amg_gs_levels=2)
    o, h = oracle_engine(spec, opts), HipEngine(spec, opts)
    for e in (o, h):
        e.set_state(u0)
        e.set_old(u0)
        e.set_dt(86.4)
    ro, rh = o.newton_solve(), h.newton_solve()
    uo, uh = o.get_state(), h.get_state()
    errs = [rel2(uh[f], uo[f]) for f in range(3)]
    print("Newton its: reference %d, GPU %d; FGMRES its %d, %d; state errors %r" % (ro["nits"], rh["nits"], ro["lits"], rh["lits"], errs))
    assert h.amg_gs_info(0)["levels"] == 2 and o.pc.amg_p.n_gs_levels() == 2
    assert (ro["nits"], ro["lits"]) == (4, 29), ro
    assert ro["reason"] > 0 and rh["reason"] == ro["reason"], (ro, rh)
    assert rh["nits"] == ro["nits"], (ro, rh)
    assert abs(rh["lits"] - ro["lits"]) <= ro["nits"], (ro, rh)
    assert max(errs) <= 1e-8, errs
    h.close()


def test_box_live_toggle():
    """0 -> 2 -> 0 on one context, a set-up after each: the hierarchies are re-planned and the pc_apply graphs re-captured, so
    the third result is the first bit for bit and the second is a fresh Gauss-Seidel context's; the second application of each
    is a replay of the recorded program and gives the first application's bits."""
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_gs_levels=2))
    x = np.random.default_rng(14).standard_normal(u.shape)
    h.vec_set("x", x)
    ys, levels = [], []
    for L in (0, 2, 0):
        h.set_options(amg_gs_levels=L)
        h.pc_setup()
        h.pc_apply("x", "y")
        first = h.vec_get("y").copy()
        h.pc_apply("x", "y")                       # (the second application replays the captured graph)
        ys.append(h.vec_get("y").copy())
        assert np.array_equal(first, ys[-1])
        levels.append(h.amg_gs_info(0)["levels"])
    assert levels == [0, 2, 0]
    assert np.array_equal(ys[0], ys[2])
    assert not np.array_equal(ys[0], ys[1])
    assert rel2(ys[1], o.pc.apply(x)) <= TOL
    h.close()


def test_inner_krylov_solve_around_the_gs_cycle():
    """pc_cpr with s1_ksp fgmres (fixed count): the inner solve's preconditioner is the Gauss-Seidel V-cycle."""
    import oracle.linalg as la
    k = 4
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cpr", amg_gs_levels=2, s1_ksp="fgmres", s1_max_it=k, s1_rtol=0.0, s1_atol=0.0))
    check_layout(o, h, 0, spec, 2, 1)
    x = np.random.default_rng(15).standard_normal(u.shape)
    A00 = la.decouple(J, "No", [0])[0][:, 0, 0]
    y = np.zeros_like(x)
    y[0] = la.fgmres(lambda v: la.spmv_scalar(A00, v), o.pc.amg_p.vcycle, x[0], rtol=0.0, atol=0.0, restart=k, maxit=k)[0]
    want = y + o.pc.ilu.solve(x - la.spmv_block(J, y))
    h.vec_set("x", x)
    h.stage1_apply("x", "y")
    h.pc_apply("x", "z")
    d1, d2 = rel2(h.vec_get("y"), y), rel2(h.vec_get("z"), want)
    print("inner fgmres(%d) around the GS cycle: stage 1 %.3e, pc_apply %.3e" % (k, d1, d2))
    assert h.inner_stats()[0] >= 2
    assert d1 <= TOL and d2 <= TOL, (d1, d2)
    h.close()


def tall_box(Nx=12, Ny=22, Nz=10, dz=40.0, nphase=2):
    """Homogeneous box whose cells are much taller than wide: the weakest coupling is along z (internal axis 0), so level 0
    coarsens another axis.  Dx / Dy is no power of two: with Dx = 2 Dy the x and y strengths tie exactly after one coarsening
    step, and the schedule then hangs on the last bit of the strengths' sums."""
    from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo
    from thermalporous_amd.physicalparameters import PhysicalParameters
    from thermalporous_amd.problem import build_spec
    from thermalporous_amd.wellheatercase import WellHeaterCase
    p = PhysicalParameters()
    p.rate = 2e-4
    p.S_o = 0.9
    p.T_inj = 373.15
    g = HomogeneousBoxGeo(Nx, Ny, Nz, p, Length=Nx*6.096, Length_y=Ny*2.5, Length_z=Nz*dz)
    L, Ly, Lz = g.Length, g.Length_y, g.Length_z
    c = WellHeaterCase(p, g, prod_points=[[140.0/365.76*L, 210.0/670.56*Ly, 0.2*Lz]], inj_points=[[265.0/365.76*L, 260.0/670.56*Ly, 0.8*Lz]])
    spec = build_spec(g, c, p, nphase)
    return spec, cases.uniform_state(spec, p.p_ref, p.T_prod, p.S_o), p, g, c


# name, builder, kw, opts, (internal extents, GS levels of the pressure hierarchy)
SHAPES = [
    # every extent odd, on level 0 (11 x 13 x 21 = 3003 cells) and on level 1 (11 x 13 x 11): the colours have unequal counts, 1502
    # red and 1501 black, and no line or plane starts a 64-lane wavefront; the box of the cases above has the even extents, where
    # the colour is not the parity of the linear index
    ("13x21x11", cases.c4_spe10_3d, dict(Nx=13, Ny=21, Nz=11, nphase=2), dict(pc="cptr", amg_gs_levels=2), ((11, 13, 21), 2)),
    # 2-D, single-phase: n2 = 1, an odd n0; one GS level (level 1 has 697 cells)
    ("41x33_2d", cases.c3_spe10_2d, dict(Nx=41, Ny=33, nphase=1), dict(pc="cpr", amg_gs_levels=1), ((41, 33, 1), 1)),
    # long axis 0, planes of 390 cells in 3 lines: few lines, the other two extents tiny
    ("3x4x130", cases.c4_spe10_3d, dict(Nx=3, Ny=4, Nz=130, nphase=2), dict(pc="cptr", amg_gs_levels=1), ((130, 3, 4), 1)),
    # cells much taller than wide: level 0 coarsens another axis than the SPE10 boxes'; two sweeps per leg
    ("tall_box", tall_box, dict(), dict(pc="cptr", amg_gs_levels=2, amg_gs_sweeps=2), ((10, 12, 22), 2)),
]


@pytest.mark.parametrize("name,builder,kw,opts,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(name, builder, kw, opts, want):
    spec, u0, u, o, h, J = make(builder, kw, opts)
    n, levels = want
    assert tuple(int(v) for v in spec["n"]) == n
    info = check_layout(o, h, 0, spec, levels, opts.get("amg_gs_sweeps", 1))
    if name == "13x21x11":
        assert (info["red"], info["black"]) == (1502, 1501)
        assert o.pc.amg_p.levels[1][0].shape == (11, 13, 11)
    if name == "tall_box":
        assert h.amg_layout(0)[1][0] in (1, 2)
    x = np.random.default_rng(16).standard_normal(u.shape)
    h.vec_set("x", x)
    h.amg_vcycle(0, "x", 0, "y", 0)
    dv = rel2(h.vec_get("y")[0], o.pc.amg_p.vcycle(x[0]))
    h.pc_apply("x", "z")
    dp = rel2(h.vec_get("z"), o.pc.apply(x))
    print("%s: pressure V-cycle %.3e, pc_apply %.3e" % (name, dv, dp))
    assert dv <= TOL and dp <= TOL, (name, dv, dp)
    h.close()


def test_grid_inside_the_tail_is_the_option_off_result():
    """9x14x8 = 1008 cells: every level is a tail level, no level is a GS level; L = 2 changes nothing, bit for bit, and
    tp_amg_gs_info is all zeros."""
    kw = dict(Nx=9, Ny=14, Nz=8, nphase=2)
    spec, u0, u, o, h, J = make(cases.c4_spe10_3d, kw, dict(pc="cptr", amg_gs_levels=2))
    spec, u0, u, o0, h0, J = make(cases.c4_spe10_3d, kw, dict(pc="cptr"))
    for which in (0, 1):
        assert h.amg_gs_info(which) == dict(levels=0, sweeps=0, red=0, black=0)
        assert h0.amg_gs_info(which) == dict(levels=0, sweeps=0, red=0, black=0)
        assert h.amg_tail_info(which)["tail_level"] == 0
    assert o.pc.amg_p.n_gs_levels() == 0
    x = np.random.default_rng(17).standard_normal(u.shape)
    for e in (h, h0):
        e.vec_set("x", x)
        e.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), h0.vec_get("y"))
    assert rel2(h.vec_get("y"), o.pc.apply(x)) <= TOL
    h.close()
    h0.close()


def test_device_side_refusals():
    """The C ABI refuses amg_gs_levels with amg_line_levels, amg_single, pc_kind 3, schur_a11 = 2, L > amg_full_levels, sweeps
    outside 1..4 and a sweep count without levels (tp_set_options), and with more than one slab (tp_create), naming both options;
    the context goes on working afterwards."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_gs_levels=1))
    x = np.random.default_rng(18).standard_normal(u.shape)
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    y0 = h.vec_get("y").copy()

    def refused(first, other, **kw):
        opt = HipEngine._make_options({**h.opts, **kw})             # (the host-side checks bypassed)
        rc = h.lib.tp_set_options(h.ctx, C.byref(opt))
        msg = h.lib.tp_last_error().decode()
        assert rc != 0 and first in msg and other in msg, (other, rc, msg)

    refused("amg_gs_levels", "amg_line_levels", amg_line_levels=1)
    refused("amg_gs_levels", "amg_single", amg_single=True)
    refused("amg_gs_levels", "pc_kind 3", pc="cptramg")
    refused("amg_gs_levels", "schur_a11", schur_selfp=True)
    refused("amg_gs_levels", "amg_full_levels", amg_gs_levels=4)
    refused("amg_gs_sweeps", "1..4", amg_gs_sweeps=5)
    refused("amg_gs_sweeps", "1..4", amg_gs_sweeps=0)
    refused("amg_gs_sweeps", "amg_gs_levels", amg_gs_levels=0, amg_gs_sweeps=2)
    # more than one slab: tp_create of a two-slab context
    from thermalporous_amd.engine import tp_grid, tp_params
    n0, n1, n2 = (int(v) for v in spec["n"])
    g = tp_grid(n0, n1, n2//2, n2, 0, (C.c_double*3)(*[float(v) for v in spec["h"]]), int(spec["gaxis"]), 2, 0, 2)
    prm = tp_params(*[float(spec["prm"][k]) for k in tp_params._names])
    ctx = C.c_void_p()
    rc = h.lib.tp_create(C.byref(g), C.byref(prm), C.byref(HipEngine._make_options(h.opts)), 0, C.byref(ctx))
    msg = h.lib.tp_last_error().decode()
    assert rc != 0 and not ctx and "amg_gs_levels" in msg and "nranks" in msg, (rc, msg)
    h.pc_setup()
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y0)
    assert h.amg_gs_info(0)["levels"] == 1
    h.close()
