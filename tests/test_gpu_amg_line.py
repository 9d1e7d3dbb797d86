"""amg_line_levels on the GPU: line-Jacobi along internal axis 0 on the top levels of the scalar V-cycles (k_amg_line_factor,
k_amg_line_sweep) against amg_line_ref.LineSemiAMG, the oracle's SemiAMG with the smoother restated.

Tolerances are the project's fp64 ones: V-cycle, stage 1 and pc_apply rel <= 1e-10 in the 2-norm, FGMRES counts
+-1, Newton counts equal, states rel <= 1e-8.  Every case asserts from tp_amg_layout / tp_amg_line_info that it runs the line
levels it claims."""
import ctypes as C

import numpy as np
import pytest

import cases
from amg_line_ref import oracle_engine

pytestmark = pytest.mark.gpu

TOL = 1e-10
LDS_BYTES = 48*1024          # the sweep's LDS budget: lines per workgroup = min(64, budget / (8 (n0 | 1)), lines)


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def group_of(n0, lines):
    return min(64, LDS_BYTES//(8*(n0 | 1)), lines)


def make(builder, kw, opts, dt=8640.0, seed=5, amp=0.3):
    """Reference (oracle with LineSemiAMG hierarchies) and GPU engine at the same perturbed state, both set up."""
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


def check_layout(o, h, which, n0, lines, levels):
    """The GPU's plan is the reference's: `levels` line levels, level 0 with lines of n0 cells in groups of group_of."""
    info = h.amg_line_info(which)
    ref = o.pc.amg_p if which == 0 else o.pc.amg_T
    assert info["levels"] == levels == ref.n_line_levels(), (info, ref.n_line_levels())
    assert info["n0"] == n0
    assert info["group"] == (group_of(n0, lines) if levels else 0), info
    assert (info["bytes"] > 0) == (levels > 0)
    assert h.amg_layout(which)[1] == list(ref.sched)
    return info


BOX = (cases.c4_spe10_3d, dict(Nx=12, Ny=22, Nz=10, nphase=2))


# (line levels, time step): at dt = 8640 both hierarchies run full cycles; at dt = 8.64 the temperature operator S~ is diagonally
# dominant on level 0 (ratio 0.13 <= amg_dom_tau) and its hierarchy ends there, at a line level, with two line sweeps
@pytest.fixture(scope="module", params=[(1, 8640.0), (2, 8640.0), (2, 8.64)], ids=["L1", "L2", "L2_trunc"])
def box(request):
    L, dt = request.param
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_line_levels=L), dt=dt)
    yield L, spec, u0, u, o, h, J
    h.close()


def test_box_layout(box):
    """2640 cells, 264 lines of 10 cells in groups of 64 (ragged last group of 8); level 1 has 1320 cells, level 2 (660 cells) is
    the tail.  The S~ hierarchy coarsens axis 0 first (lines of 10, then of 5), the pressure hierarchy axis 2 (lines of 10 on
    both levels).  In the third variant the S~ hierarchy ends with relaxation only at level 0, a line level."""
    L, spec, u0, u, o, h, J = box
    for which in (0, 1):
        info = check_layout(o, h, which, 10, 264, L)
        assert info["group"] == 64 and 264 % 64 != 0
        assert h.amg_tail_info(which)["tail_level"] == 2
    assert h.amg_layout(1)[1][0] == 0 and h.amg_layout(0)[1][0] == 2
    lv, ratio0 = h.amg_trunc(1)
    want = o.pc.amg_T.trunc
    assert lv == (-1 if want is None else want), (lv, ratio0, want)
    if o.prob.dt < 100.0:                                          # the truncating variant
        assert 0 <= lv < L
    assert h.amg_trunc(0)[0] == -1 and o.pc.amg_p.trunc is None


def test_box_vcycles(box):
    L, spec, u0, u, o, h, J = box
    x = np.random.default_rng(11).standard_normal(u.shape)
    h.vec_set("x", x)
    for which, ref in ((0, o.pc.amg_p), (1, o.pc.amg_T)):
        h.amg_vcycle(which, "x", which, "y", which)
        d = rel2(h.vec_get("y")[which], ref.vcycle(x[which]))
        print("L=%d hierarchy %d: V-cycle vs LineSemiAMG %.3e" % (L, which, d))
        assert d <= TOL, (which, d)


def test_box_stage1_and_pc_apply(box):
    L, spec, u0, u, o, h, J = box
    x = np.random.default_rng(12).standard_normal(u.shape)
    h.vec_set("x", x)
    h.stage1_apply("x", "y")
    h.pc_apply("x", "z")
    d1, d2 = rel2(h.vec_get("y"), o.pc.stage1(x)), rel2(h.vec_get("z"), o.pc.apply(x))
    print("L=%d: stage 1 %.3e, pc_apply %.3e" % (L, d1, d2))
    assert d1 <= TOL and d2 <= TOL, (d1, d2)


def test_box_fgmres(box):
    import oracle.linalg as la
    L, spec, u0, u, o, h, J = box
    b = np.random.default_rng(13).standard_normal(u.shape)
    h.vec_set("b", b)
    its, reason, rn = h.fgmres("b", "sol")
    xo, ito, ro, _ = la.fgmres(lambda v: la.spmv_block(J, v), o.pc.apply, b, rtol=o.opts["ksp_rtol"], atol=o.opts["ksp_atol"],
                               restart=o.opts["ksp_restart"], maxit=o.opts["ksp_max_it"])
    print("L=%d: FGMRES its GPU %d, reference %d; solutions differ by %.3e" % (L, its, ito, rel2(h.vec_get("sol"), xo)))
    assert reason > 0 and ro > 0
    assert abs(its - ito) <= 1, (its, ito)


def test_box_newton_solve():
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = BOX[0](**BOX[1])
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, amg_line_levels=2)
    o, h = oracle_engine(spec, opts), HipEngine(spec, opts)
    for e in (o, h):
        e.set_state(u0)
        e.set_old(u0)
        e.set_dt(86.4)
    ro, rh = o.newton_solve(), h.newton_solve()
    uo, uh = o.get_state(), h.get_state()
    errs = [rel2(uh[f], uo[f]) for f in range(3)]
    print("Newton its: reference %d, GPU %d; FGMRES its %d, %d; state errors %r" % (ro["nits"], rh["nits"], ro["lits"], rh["lits"], errs))
    assert h.amg_line_info(0)["levels"] == 2 and o.pc.amg_p.n_line_levels() == 2
    assert ro["reason"] > 0 and rh["reason"] == ro["reason"], (ro, rh)
    assert rh["nits"] == ro["nits"], (ro, rh)
    assert abs(rh["lits"] - ro["lits"]) <= ro["nits"], (ro, rh)
    assert max(errs) <= 1e-8, errs
    h.close()


def test_box_live_toggle():
    """0 -> 2 -> 0 on one context, a set-up after each: the hierarchies are re-planned and the pc_apply graphs re-captured, so
    the third result is the first bit for bit and the second is a fresh line-relaxation context's."""
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_line_levels=2))
    x = np.random.default_rng(14).standard_normal(u.shape)
    h.vec_set("x", x)
    ys, levels = [], []
    for L in (0, 2, 0):
        h.set_options(amg_line_levels=L)
        h.pc_setup()
        h.pc_apply("x", "y")
        h.pc_apply("x", "y")                       # (the second application replays the captured graph)
        ys.append(h.vec_get("y").copy())
        levels.append(h.amg_line_info(0)["levels"])
    assert levels == [0, 2, 0]
    assert np.array_equal(ys[0], ys[2])
    assert not np.array_equal(ys[0], ys[1])
    assert rel2(ys[1], o.pc.apply(x)) <= TOL
    h.close()


def test_inner_krylov_solve_around_the_line_cycle():
    """pc_cpr with s1_ksp fgmres (fixed count): the inner solve's preconditioner is the line-relaxation V-cycle."""
    import oracle.linalg as la
    k = 4
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cpr", amg_line_levels=2, s1_ksp="fgmres", s1_max_it=k, s1_rtol=0.0, s1_atol=0.0))
    check_layout(o, h, 0, 10, 264, 2)
    x = np.random.default_rng(15).standard_normal(u.shape)
    A00 = la.decouple(J, "No", [0])[0][:, 0, 0]
    y = np.zeros_like(x)
    y[0] = la.fgmres(lambda v: la.spmv_scalar(A00, v), o.pc.amg_p.vcycle, x[0], rtol=0.0, atol=0.0, restart=k, maxit=k)[0]
    want = y + o.pc.ilu.solve(x - la.spmv_block(J, y))
    h.vec_set("x", x)
    h.stage1_apply("x", "y")
    h.pc_apply("x", "z")
    d1, d2 = rel2(h.vec_get("y"), y), rel2(h.vec_get("z"), want)
    print("inner fgmres(%d) around the line cycle: stage 1 %.3e, pc_apply %.3e" % (k, d1, d2))
    assert h.inner_stats()[0] >= 2
    assert d1 <= TOL and d2 <= TOL, (d1, d2)
    h.close()


def tall_box(Nx=12, Ny=22, Nz=10, dz=40.0, nphase=2):
    """Homogeneous box whose cells are much taller than wide: the weakest coupling is along z (internal axis 0).  Dx / Dy is
    no power of two: with Dx = 2 Dy the x and y strengths (ratio Dx^2 / Dy^2 = 4) tie exactly after one coarsening step, and the
    schedule then hangs on the last bit of the strengths' sums."""
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


# name, builder, kw, opts, (n0, lines, line levels of the pressure hierarchy)
SHAPES = [
    # long lines: 12 lines of 130 cells (one group of 12), 4 lines of 341 (one group of 4; 64 such lines would not fit the LDS)
    ("3x4x130", cases.c4_spe10_3d, dict(Nx=3, Ny=4, Nz=130, nphase=2), dict(pc="cptr", amg_line_levels=1), (130, 12, 1)),
    ("2x2x341", cases.c4_spe10_3d, dict(Nx=2, Ny=2, Nz=341, nphase=2), dict(pc="cptr", amg_line_levels=1), (341, 4, 1)),
    # 2-D, single-phase: 33 lines of 40 cells along x, less than one full wave of lines
    ("40x33_2d", cases.c3_spe10_2d, dict(Nx=40, Ny=33, nphase=1), dict(pc="cpr", amg_line_levels=1), (40, 33, 1)),
    # cells much taller than wide: level 0 coarsens another axis, level 1's lines are as long as level 0's
    ("tall_box", tall_box, dict(), dict(pc="cptr", amg_line_levels=2), (10, 264, 2)),
]


@pytest.mark.parametrize("name,builder,kw,opts,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(name, builder, kw, opts, want):
    spec, u0, u, o, h, J = make(builder, kw, opts)
    n0, lines, levels = want
    assert tuple(spec["n"])[0] == n0 and int(np.prod(spec["n"]))//n0 == lines
    check_layout(o, h, 0, n0, lines, levels)
    if name == "2x2x341":
        assert group_of(341, 64) < 64                              # the line-length regime where the LDS budget limits the group
    if name == "tall_box":
        assert h.amg_layout(0)[1][0] in (1, 2)                     # level 0 keeps n0: level 1 has lines of 10 too
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
    """9x14x8 = 1008 cells: every level is a tail level, no level is a line level; L = 2 changes nothing, bit for bit."""
    kw = dict(Nx=9, Ny=14, Nz=8, nphase=2)
    spec, u0, u, o, h, J = make(cases.c4_spe10_3d, kw, dict(pc="cptr", amg_line_levels=2))
    spec, u0, u, o0, h0, J = make(cases.c4_spe10_3d, kw, dict(pc="cptr"))
    for which in (0, 1):
        info = h.amg_line_info(which)
        assert info["levels"] == 0 and info["bytes"] == 0 and info["group"] == 0, info
        assert h.amg_tail_info(which)["tail_level"] == 0
    assert o.pc.amg_p.n_line_levels() == 0
    x = np.random.default_rng(17).standard_normal(u.shape)
    for e in (h, h0):
        e.vec_set("x", x)
        e.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), h0.vec_get("y"))
    assert rel2(h.vec_get("y"), o.pc.apply(x)) <= TOL
    h.close()
    h0.close()


def test_device_side_refusals():
    """The C ABI refuses amg_line_levels with amg_single, pc_kind 3, schur_a11 = 2 and L > amg_full_levels (tp_set_options),
    naming both options; the context goes on working afterwards."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, u, o, h, J = make(*BOX, dict(pc="cptr", amg_line_levels=1))
    x = np.random.default_rng(18).standard_normal(u.shape)
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    y0 = h.vec_get("y").copy()

    def refused(other, **kw):
        opt = HipEngine._make_options({**h.opts, **kw})             # (the host-side checks bypassed)
        rc = h.lib.tp_set_options(h.ctx, C.byref(opt))
        msg = h.lib.tp_last_error().decode()
        assert rc != 0 and "amg_line_levels" in msg and other in msg, (other, rc, msg)

    refused("amg_single", amg_single=True)
    refused("pc_kind 3", pc="cptramg")
    refused("schur_a11", schur_selfp=True)
    refused("amg_full_levels", amg_line_levels=4)
    # more than one slab: tp_create of a two-slab context
    from thermalporous_amd.engine import tp_grid, tp_params
    n0, n1, n2 = (int(v) for v in spec["n"])
    g = tp_grid(n0, n1, n2//2, n2, 0, (C.c_double*3)(*[float(v) for v in spec["h"]]), int(spec["gaxis"]), 2, 0, 2)
    prm = tp_params(*[float(spec["prm"][k]) for k in tp_params._names])
    ctx = C.c_void_p()
    rc = h.lib.tp_create(C.byref(g), C.byref(prm), C.byref(HipEngine._make_options(h.opts)), 0, C.byref(ctx))
    msg = h.lib.tp_last_error().decode()
    assert rc != 0 and not ctx and "amg_line_levels" in msg and "nranks" in msg, (rc, msg)
    h.pc_setup()
    h.pc_apply("x", "y")
    assert np.array_equal(h.vec_get("y"), y0)
    h.close()
