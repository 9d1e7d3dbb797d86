"""Graded tensor-product grids on the GPU (tp_set_spacing; the graded instantiations of k_assemble, k_assemble_bc, k_trans and
k_bc_trans in csrc/tp_assembly.hip) against the numpy reference tests/graded_ref.py: entries of R, J and S~ with
test_gpu_assembly_edges' rule, the default path bit for bit, a linear temperature, a hydrostatic column, conservation, Dirichlet
sides on a graded grid, Newton solves with test_gpu_bc's assertions, and the library's refusals."""
import ctypes as C

import numpy as np
import pytest

import cases
from bc_ref import assert_both_directions, make_boundary
from graded_ref import cell_centres_internal, equal_widths, field_change, hydrostatic_graded_column, random_widths, spec_lengths
from oracle.engine import OracleEngine
from oracle.tpfa import Problem, _hi, _lo
from test_gpu_assembly_edges import TOL, assert_entries
from test_gpu_bc import C4, NEWTON, _assert_step

pytestmark = pytest.mark.gpu

ENTRY = [
    ("1ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=1), None),
    ("2ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=2), None),
    ("2ph_3d_6x5x4", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), None),       # the two axis permutations, gravity on
    ("2ph_3d_5x6x4", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4, nphase=2), None),       # internal axis 0
    ("1ph_3d_4x5x6", cases.c4_spe10_3d, dict(Nx=4, Ny=5, Nz=6, nphase=1), None),
    ("2ph_line_1x1x5", cases.c4_spe10_3d, dict(Nx=1, Ny=1, Nz=5, nphase=2), (0,)),     # only z (internal axis 0) graded
]


def _opts(nphase):
    return dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")


def _graded_spec(builder, kw, seed=7, only=None):
    """The builder's spec (wells and heaters stay in) with seeded uniform(0.4, 2.5) widths rescaled to the axis lengths; `only`:
    the internal axes that are graded, the others keep equal widths."""
    spec, u0, *_ = builder(**kw)
    hs = random_widths(spec["n"], spec_lengths(spec), seed)
    if only is not None:
        eq = equal_widths(spec)
        hs = tuple(hs[a] if a in only else eq[a] for a in range(3))
    spec["hs"] = hs
    return spec, u0


def _engine(spec, u, dt=8640.0, opts=None):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts or _opts(spec["nphase"]))
    h.set_old(u)
    h.set_dt(dt)
    h.set_state(u)
    return h


def _reference(P, u, dt=8640.0):
    P.set_old(u)
    P.set_dt(dt)
    R = P.residual(u)
    J, Sm = P.jacobian(u, want_schur=True)
    return R, J, Sm


def _bits(h):
    R = h.residual()
    J, Sm = h.jacobian(want_schur=True)
    return R.tobytes(), J.tobytes(), Sm.tobytes()


@pytest.mark.parametrize("pid,builder,kw,only", ENTRY, ids=[e[0] for e in ENTRY])
def test_graded_entries_against_the_reference(pid, builder, kw, only):
    spec, _ = _graded_spec(builder, kw, only=only)
    u = cases.perturbed_state(spec, seed=3)
    if pid.endswith("6x5x4") or pid.endswith("5x6x4"):
        assert spec["gaxis"] == 0
    Ro, Jo, So = _reference(Problem(spec), u)
    h = _engine(spec, u)
    assert h.spacing is not None and h.spacing_info()["graded"]
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    # the spacing is visible in what is compared: the GPU's result is not the uniform oracle's
    Ru, Ju, Su = _reference(Problem({k: v for k, v in spec.items() if k != "hs"}), u)
    change = field_change(Rh, Ru, spec)
    print("%s: the residual fields differ from the uniform oracle's by %r" % (pid, change))
    assert min(change) > 0.01
    # (the off-diagonal slots: the diagonal carries the wells and the accumulation, far above any face term)
    assert np.abs(Jh[1:] - Ju[1:]).max() > 0.01*np.abs(Ju[1:]).max() and np.abs(Sh[1:] - Su[1:]).max() > 0.01*np.abs(Su[1:]).max()
    h.close()


@pytest.mark.parametrize("pid,builder,kw,only", [ENTRY[1], ENTRY[2], ENTRY[4]], ids=[ENTRY[1][0], ENTRY[2][0], ENTRY[4][0]])
def test_equal_widths_match_the_uniform_engine(pid, builder, kw, only):
    spec, *_ = builder(**kw)
    u = cases.perturbed_state(spec, seed=3)
    h0 = _engine(spec, u)
    R0 = h0.residual()
    J0, S0 = h0.jacobian(want_schur=True)
    h1 = _engine(dict(spec, hs=equal_widths(spec)), u)
    assert h1.spacing_info()["graded"] and not h0.spacing_info()["graded"]
    R1 = h1.residual()
    J1, S1 = h1.jacobian(want_schur=True)
    assert_entries(R1, J1, S1, R0, J0, S0, pid)
    h0.close()
    h1.close()


def test_default_path_is_untouched():
    """c4 box 7x13x9: an engine that never hears of spacing and one on which spacing is set and then cleared give bitwise equal
    R, J and S~; while the spacing is set the bits differ."""
    spec, *_ = cases.c4_spe10_3d(Nx=7, Ny=13, Nz=9, nphase=2)
    u = cases.perturbed_state(spec, seed=3)
    a, b = _engine(spec, u), _engine(spec, u)
    plain = _bits(a)
    assert _bits(b) == plain
    b.set_spacing(random_widths(spec["n"], spec_lengths(spec), 11))
    info = b.spacing_info()
    assert info["graded"] and all(lo < hi for lo, hi in zip(info["hmin"], info["hmax"]))
    moved = _bits(b)
    assert all(x != y for x, y in zip(moved, plain))
    b.set_spacing(None)
    info = b.spacing_info()
    assert not info["graded"] and info["hmin"] == info["hmax"] == tuple(float(v) for v in spec["h"])
    assert b.spacing is None and _bits(b) == plain
    assert _bits(a) == plain
    a.close()
    b.close()


@pytest.mark.parametrize("nphase", [1, 2])
def test_linear_temperature_gives_no_energy_residual_inside(nphase):
    """2-D 9x6, no sources, uniform phi, static kT, p and S, T = 300 + 0.7 x_0 - 0.4 x_1 at the true cell centres, old state =
    state: the conductive fluxes of an interior cell cancel to TOL of the largest single face flux."""
    spec, u0, *_ = cases.c3_spe10_2d(Nx=9, Ny=6, nphase=nphase)
    spec["sources"] = None
    spec["phi"] = np.full_like(np.asarray(spec["phi"], dtype=float), 0.2)
    spec["kT"] = np.full_like(np.asarray(spec["phi"], dtype=float), 2.5)
    spec["hs"] = random_widths(spec["n"], spec_lengths(spec), 13)
    x0, x1, _ = cell_centres_internal(spec["hs"])
    u = np.array(u0, dtype=float)
    u[1] = 300.0 + 0.7*x0[None, None, :] - 0.4*x1[None, :, None]
    P = Problem(spec)
    kT = P.props(*P.split(u))["kT"][0] + 0*u[1]
    flux = max(np.abs(P.geom.conduction(a, kT[_lo(a)], kT[_hi(a)])[0]*np.diff(u[1], axis=2 - a)).max() for a in (0, 1))
    assert flux > 0.0
    h = _engine(spec, u)
    R = h.residual()
    inner = np.abs(R[1][:, 1:-1, 1:-1]).max()
    edge = np.abs(R[1]).max()
    print("nphase %d: interior energy rows %.3e, boundary rows %.3e, largest face flux %.3e" % (nphase, inner, edge, flux))
    assert inner < TOL*flux and edge > 0.1*flux
    # the uniform formula on the same state does not cancel
    h0 = _engine({k: v for k, v in spec.items() if k != "hs"}, u)
    assert np.abs(h0.residual()[1][:, 1:-1, 1:-1]).max() > 0.01*flux
    h.close()
    h0.close()


# The kernels form the accumulation of the current and of the old state in two places (k_assemble, k_accum_old), whose products
# the compiler contracts differently: with old state = state their difference is not 0 but up to an ulp of the mass density
# (3e-14 of ~180) times V_c/dt.  At dt = 864 s that is 1e-16 in the mass row, 1e-5 of the scale T^K L rho g d ~ 1e-11 of this
# column's faces -- accumulation rounding, the same on a uniform grid, not a face flux.  The time step is free here and enters
# nothing else, so it is taken large enough that this term lies four orders below the bound: 3e-14 * 27 / 1e10 = 8e-23 against
# 1e-8 * 2.5e-11 = 2.5e-19; the mass row then is the face fluxes alone, as the check needs.
HYDROSTATIC_DT = 1e10


def test_hydrostatic_graded_column_carries_no_flow():
    """1x1x6, one phase, widths proportional to (1, 4, 2, 8, 1, 4), uniform T, p at the centres from a finely integrated hydrostat
    (graded_ref.hydrostatic_graded_column: no use of the face formula), old state = state: the mass row is the face fluxes alone,
    each below 1e-8 of T^K L rho g d of its face."""
    spec, u, scale = hydrostatic_graded_column()
    h = _engine(spec, u, dt=HYDROSTATIC_DT)
    R = h.residual()[0].reshape(-1)
    f = np.cumsum(R)[:-1]                      # R_i = f_i - f_(i-1) along the column (w0 = 1): the flux through face i
    print("face fluxes / (T^K L rho g d):", f/scale)
    assert np.all(np.abs(f) < 1e-8*scale) and abs(np.sum(R)) < 1e-8*scale.min()
    h.close()
    # a wrong distance shows: the uniform formula on the same column
    h0 = _engine({k: v for k, v in spec.items() if k != "hs"}, u, dt=HYDROSTATIC_DT)
    f0 = np.cumsum(h0.residual()[0].reshape(-1))[:-1]
    print("the uniform formula:", f0/scale)
    assert np.abs(f0/scale).max() > 0.05
    h0.close()


def test_conservation():
    spec, _ = _graded_spec(cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), seed=17)
    spec["sources"] = None
    u = cases.perturbed_state(spec, seed=3)
    h = _engine(spec, u)
    R = h.residual()
    for f in range(3):
        print("field %d: sum %.3e, sum of |R| %.3e" % (f, R[f].sum(), np.abs(R[f]).sum()))
        assert np.abs(R[f]).sum() > 0.0 and abs(R[f].sum()) < 1e-12*np.abs(R[f]).sum()
    h.close()


SIDES = [
    ("2ph_3d_6x5x4_all_open", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), {s: "open" for s in range(6)}),
    ("2ph_2d_7x5_one_thermal", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=2), {1: "thermal"}),
]


@pytest.mark.parametrize("pid,builder,kw,kinds", SIDES, ids=[e[0] for e in SIDES])
def test_spacing_with_sides(pid, builder, kw, kinds):
    spec, _ = _graded_spec(builder, kw, seed=19)
    u = cases.perturbed_state(spec, seed=3)
    spec["boundary"] = make_boundary(spec, u, kinds, seed=4)
    P = Problem(spec)
    Ro, Jo, So = _reference(P, u)
    assert_both_directions(P)
    ref = P.last_flux.copy()
    h = _engine(spec, u)
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    flux = h.boundary_flux()
    for q in range(P.b):
        if np.abs(ref[:, q]).max() == 0.0:         # (a thermal side alone moves no mass)
            assert np.all(flux[:, q] == 0.0)
            continue
        assert np.abs(flux[:, q] - ref[:, q]).max() < 1e-11*np.abs(ref[:, q]).max(), (q, flux[:, q], ref[:, q])
    assert np.abs(flux[sorted(kinds), 1]).min() > 0.0
    # the boundary faces see the spacing: the uniform sides on the same state give other sums
    h0 = _engine({k: v for k, v in spec.items() if k != "hs"}, u)
    h0.residual()
    assert np.abs(h0.boundary_flux()[:, 1] - flux[:, 1]).max() > 0.01*np.abs(flux[:, 1]).max()
    h.close()
    h0.close()


# ---- Newton ----------------------------------------------------------------------------------------------------------------
def _two_steps(o, h, u0, dt, steps=2):
    for e in (o, h):
        e.set_state(u0)
    for step in range(steps):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(dt)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("step %d: oracle nits %d lits %d, engine nits %d lits %d" % (step, ro["nits"], ro["lits"], rh["nits"], rh["lits"]))
        _assert_step(ro, rh, o, h)


@pytest.mark.parametrize("name,nphase,opts,dt", NEWTON, ids=[c[0] for c in NEWTON])
def test_newton_parity_on_a_graded_box(name, nphase, opts, dt):
    """test_gpu_bc's presets, sizes and assertions on the c4 box 7x13x9 with random widths on every axis."""
    from thermalporous_amd.engine import HipEngine
    spec, u0 = _graded_spec(cases.c4_spe10_3d, dict(nphase=nphase, **C4), seed=23)
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    _two_steps(o, h, u0, dt)
    h.close()


def test_newton_parity_with_line_relaxation_on_thin_layers():
    """amg_line_levels on a box whose z widths (internal axis 0, the lines' axis) span a ratio of 8: tests/amg_line_ref.py swaps
    its line smoother into any TwoStagePC, so the same oracle is asserted against."""
    from amg_line_ref import swap_into
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.spacing import geometric_widths
    spec, u0, *_ = cases.c4_spe10_3d(Nx=12, Ny=22, Nz=10, nphase=2)
    assert spec["gaxis"] == 0
    hs = list(equal_widths(spec))
    hs[0] = geometric_widths(10, spec_lengths(spec)[0], 8.0**0.25, refine="both")
    assert abs(hs[0].max()/hs[0].min() - 8.0) < 1e-9
    spec["hs"] = tuple(hs)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, amg_line_levels=2)
    o = OracleEngine(spec, {k: v for k, v in opts.items() if k != "amg_line_levels"})
    swap_into(o.pc, 2)
    h = HipEngine(spec, opts)
    _two_steps(o, h, u0, 86.4, steps=1)
    assert h.amg_line_info(0)["levels"] == 2 and o.pc.amg_p.n_line_levels() == 2
    h.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_refusals_return_the_error_code_with_a_message():
    from thermalporous_amd import engine as E
    spec, *_ = cases.c4_spe10_3d(Nx=4, Ny=5, Nz=6, nphase=1)
    u = cases.perturbed_state(spec, seed=3)
    h = _engine(spec, u)
    lib = h.lib
    n = h.gn
    good = [np.ascontiguousarray(w) for w in random_widths(n, spec_lengths(spec), 5)]

    def call(ctx, w):
        return lib.tp_set_spacing(ctx, _dp(w[0]), C.c_int64(w[0].size), _dp(w[1]), C.c_int64(w[1].size), _dp(w[2]), C.c_int64(w[2].size))
    plain = h.residual().tobytes()
    # arrays of wrong length
    short = [good[0][:-1].copy(), good[1], good[2]]
    assert call(h.ctx, short) != 0
    assert "widths for axis 0" in lib.tp_last_error().decode()
    # a zero width, a NaN
    for bad in (0.0, float("nan"), -1.0):
        w = [good[0], good[1].copy(), good[2]]
        w[1][2] = bad
        assert call(h.ctx, w) != 0
        assert "axis 1" in lib.tp_last_error().decode() and "positive" in lib.tp_last_error().decode()
    # one null among three
    assert lib.tp_set_spacing(h.ctx, _dp(good[0]), C.c_int64(n[0]), None, C.c_int64(0), _dp(good[2]), C.c_int64(n[2])) != 0
    assert "null widths" in lib.tp_last_error().decode()
    # none of them changed the context
    assert not h.spacing_info()["graded"] and h.residual().tobytes() == plain
    with pytest.raises(ValueError, match="widths but the grid has"):
        h.set_spacing(short)
    h.close()
    # a slab-group context: tp_set_spacing fails; the engine refuses before any context exists
    group = C.c_void_p()
    assert lib.tp_local_group_create(2, C.byref(group)) == 0
    try:
        s = E.HipEngine(spec, _opts(1), rank=0, nranks=2, local_group=group)
        part = [good[0], good[1], good[2][:s.n[2]].copy()]
        assert call(s.ctx, part) != 0
        msg = lib.tp_last_error().decode()
        assert "slab group" in msg and "nranks = 2" in msg
        s.close()
        with pytest.raises(NotImplementedError, match="nranks = 2"):
            E.HipEngine(dict(spec, hs=tuple(good)), _opts(1), rank=0, nranks=2, local_group=group)
    finally:
        lib.tp_local_group_destroy(group)
    # and the other way round: a context with spacing takes no slab group
    g1 = E.HipEngine(dict(spec, hs=tuple(good)), _opts(1))
    group = C.c_void_p()
    assert lib.tp_local_group_create(2, C.byref(group)) == 0
    try:
        assert lib.tp_comm_init_local(g1.ctx, group) != 0
        assert "spacing" in lib.tp_last_error().decode()
    finally:
        lib.tp_local_group_destroy(group)
    g1.close()
