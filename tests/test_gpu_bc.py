"""Dirichlet sides on the GPU (k_assemble_bc of csrc/tp_assembly.hip, tp_set_boundary, tp_boundary_flux) against the numpy
reference of the boundary face (tests/bc_ref.py): entries of R, J and S~ with test_gpu_assembly_edges' rule, the default path
bit for bit, the per-side flux sums, and Newton solves with test_newton_parity's assertions."""
import ctypes as C

import numpy as np
import pytest

import cases
from bc_ref import assert_both_directions, hydrostatic_boundary, hydrostatic_column, make_boundary, side_shape
from oracle.engine import OracleEngine
from oracle.tpfa import Problem
from test_gpu_assembly_edges import assert_entries
from test_gpu_parity import rel2

pytestmark = pytest.mark.gpu

LATERAL_OPEN = {0: "thermal", 1: "thermal", 2: "open", 3: "open", 4: "open", 5: "open"}      # internal axis 0 is z
ENTRY = [
    ("1ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=1), {0: "open", 1: "open", 2: "open", 3: "open"}),
    ("2ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=2), {0: "open", 1: "thermal", 2: "open", 3: "open"}),
    ("2ph_3d_6x5x4", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), LATERAL_OPEN),
    ("2ph_3d_5x6x4", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4, nphase=2), LATERAL_OPEN),
    # a line along z: its five cells carry all four lateral sides each, the end cells five sides
    ("2ph_line_1x1x5", cases.c4_spe10_3d, dict(Nx=1, Ny=1, Nz=5, nphase=2), LATERAL_OPEN),
    # every cell carries both sides of two axes (z and y); the one-face x ends are thermal
    ("2ph_3x1x1", cases.c4_spe10_3d, dict(Nx=3, Ny=1, Nz=1, nphase=2), {0: "thermal", 1: "thermal", 2: "open", 3: "open", 4: "thermal", 5: "thermal"}),
    # open top and bottom as well: gravity in the driving force of a boundary face
    ("2ph_3d_6x5x4_all_open", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), {s: "open" for s in range(6)}),
    ("1ph_3d_4x5x6_all_open", cases.c4_spe10_3d, dict(Nx=4, Ny=5, Nz=6, nphase=1), {s: "open" for s in range(6)}),
]


def _opts(nphase):
    return dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")


def _setup(builder, kw, kinds, seed=3):
    spec, *_ = builder(**kw)
    u = cases.perturbed_state(spec, seed=seed)
    spec["boundary"] = make_boundary(spec, u, kinds, seed=seed + 1)
    return spec, u


def _reference(spec, u, dt=8640.0):
    P = Problem(spec)
    P.set_old(u)
    P.set_dt(dt)
    R = P.residual(u)
    J, Sm = P.jacobian(u, want_schur=True)
    assert_both_directions(P)
    return P, R, J, Sm


def _engine(spec, u, dt=8640.0, opts=None):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts or _opts(spec["nphase"]))
    h.set_old(u)
    h.set_dt(dt)
    h.set_state(u)
    return h


@pytest.mark.parametrize("pid,builder,kw,kinds", ENTRY, ids=[e[0] for e in ENTRY])
def test_boundary_entries_against_the_reference(pid, builder, kw, kinds):
    spec, u = _setup(builder, kw, kinds)
    P, Ro, Jo, So = _reference(spec, u)
    if pid.endswith("6x5x4") or pid.endswith("5x6x4"):
        assert P.gaxis == 0
    # the boundary is visible in what is compared
    closed = Problem(spec, boundary={})
    closed.set_old(u)
    closed.set_dt(P.dt)
    R0 = closed.residual(u)
    assert all(np.abs(Ro[f] - R0[f]).max() > 1e-4*np.abs(Ro[f]).max() for f in range(P.b))
    h = _engine(spec, u)
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    # the residual of tp_jacobian's assembly is the same one
    assert np.array_equal(h._strip_halo(_raw_residual(h), h.b), Rh)
    h.close()


def _raw_residual(h):
    out = np.empty(h.b*h.ntot)
    h._ck(h.lib.tp_get_residual(h.ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _bits(h):
    R = h.residual()
    J, Sm = h.jacobian(want_schur=True)
    return R.tobytes(), J.tobytes(), Sm.tobytes()


def test_default_path_is_untouched():
    """c4 box 7x13x9: an engine on which tp_set_boundary(side, 0, ...) was called and one that never heard of boundaries give
    bitwise equal R, J and S~; setting a side and removing it returns to those bits."""
    spec, *_ = cases.c4_spe10_3d(Nx=7, Ny=13, Nz=9, nphase=2)
    u = cases.perturbed_state(spec, seed=3)
    a, b = _engine(spec, u), _engine(spec, u)
    plain = _bits(a)
    for side in range(6):
        b.set_boundary(side, "none")
    assert _bits(b) == plain
    B = make_boundary(spec, u, {3: "open", 0: "thermal"}, seed=5)
    for side, e in B.items():
        b.set_boundary(side, e["kind"], p=e["p"], T=e["T"], S=e["S"])
    moved = _bits(b)
    assert all(x != y for x, y in zip(moved, plain))
    assert np.abs(b.boundary_flux()).max() > 0.0
    b.set_boundary(3, "none")
    b.set_boundary(0, "none")
    assert _bits(b) == plain
    assert not b.boundary and np.array_equal(b.boundary_flux(), np.zeros((6, 3)))
    assert _bits(a) == plain
    a.close()
    b.close()


@pytest.mark.parametrize("pid,builder,kw,kinds", [ENTRY[0], ENTRY[2], ENTRY[6]], ids=[ENTRY[0][0], ENTRY[2][0], ENTRY[6][0]])
def test_boundary_flux(pid, builder, kw, kinds):
    spec, u = _setup(builder, kw, kinds)
    P, Ro, _, _ = _reference(spec, u)
    P.residual(u)
    ref = P.last_flux.copy()
    h = _engine(spec, u)
    Rh = h.residual()
    flux = h.boundary_flux()
    assert flux.shape == (6, P.b)
    for q in range(P.b):
        assert np.abs(ref[:, q]).max() > 0.0
        assert np.abs(flux[:, q] - ref[:, q]).max() < 1e-11*np.abs(ref[:, q]).max(), (q, flux[:, q], ref[:, q])
    # the same sums after the Jacobian's assembly, and zero rows for the sides that are not set
    h.jacobian()
    assert np.array_equal(h.boundary_flux(), flux)
    assert all(np.all(flux[s] == 0.0) for s in range(6) if s not in kinds)
    # what the boundary adds to the sum of the residual over the cells is what leaves through the sides
    no_bc = dict(spec)
    del no_bc["boundary"]
    h0 = _engine(no_bc, u)
    d = Rh - h0.residual()
    for q in range(P.b):
        print("%s equation %d: sum over cells %.17g, sum over sides %.17g, sum of |contributions| %.3g"
              % (pid, q, d[q].sum(), flux[:, q].sum(), np.abs(d[q]).sum()))
        assert abs(d[q].sum() - flux[:, q].sum()) < 1e-10*np.abs(d[q]).sum()
    h.close()
    h0.close()


def test_open_end_at_the_hydrostatic_pressure_carries_no_flow():
    """test_bc_host's hydrostatic check on the kernel: ghost pressures from a finely integrated hydrostat, which does not contain
    the half-cell factor g h/4; the flux through both open ends vanishes to 1e-6 of what the gravity head alone drives."""
    spec, u, pb = hydrostatic_column()
    fl = {}
    for name, B in (("hydrostatic", hydrostatic_boundary(spec, u, pb)),
                    ("equal_p", hydrostatic_boundary(spec, u, {0: u[0, 0, 0, 0], 1: u[0, 0, 0, -1]}))):
        h = _engine(dict(spec, boundary=B), u, dt=864.0)
        h.residual()
        fl[name] = h.boundary_flux()
        h.close()
    for side in (0, 1):
        print("side %d: mass flux %.3e at the hydrostatic ghost, %.3e at equal pressures" % (side, fl["hydrostatic"][side, 0], fl["equal_p"][side, 0]))
        assert abs(fl["equal_p"][side, 0]) > 0.0
        assert abs(fl["hydrostatic"][side, 0]) < 1e-6*abs(fl["equal_p"][side, 0])
        assert abs(fl["hydrostatic"][side, 1]) < 1e-6*abs(fl["equal_p"][side, 1])
    assert fl["equal_p"][0, 0] > 0.0 and fl["equal_p"][1, 0] < 0.0


@pytest.mark.parametrize("nphase", [1, 2])
def test_ghost_pressure_of_a_thermal_side_changes_no_bit(nphase):
    """tp_set_boundary itself with kind thermal and arbitrary p_b (HipEngine.set_boundary would replace them by p_ref): two very
    different sets of ghost pressures, on a side of the gravity axis and on a lateral one, give the same bits of R, J, S~ and of
    the flux sums."""
    from bc_ref import side_slice
    spec, *_ = cases.c4_spe10_3d(Nx=6, Ny=5, Nz=4, nphase=nphase)
    u = cases.perturbed_state(spec, seed=3)
    B = make_boundary(spec, u, {1: "thermal", 4: "thermal"}, seed=8)
    h = _engine(spec, u)
    rng = np.random.default_rng(2)
    seen = []
    for lo, hi in ((1.0, 5.0), (60.0, 400.0)):
        for side, e in B.items():
            vals = [rng.uniform(lo, hi, e["p"].shape), e["T"]] + ([e["S"]] if nphase == 2 else [])
            v = np.ascontiguousarray(np.stack([np.asarray(x, dtype=float).reshape(-1) for x in vals]))
            h._ck(h.lib.tp_set_boundary(h.ctx, side, 2, v.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(e["p"].size)))
        seen.append(_bits(h) + (h.boundary_flux().tobytes(),))
    assert seen[0] == seen[1]
    # and they are the bits HipEngine.set_boundary gives, which passes p_ref
    for side, e in B.items():
        h.set_boundary(side, "thermal", p=e["p"], T=e["T"], S=e["S"])
    assert _bits(h) + (h.boundary_flux().tobytes(),) == seen[0]
    assert np.abs(h.boundary_flux()[[1, 4], 1]).min() > 0.0 and np.all(h.boundary_flux()[:, 0] == 0.0)
    h.close()


# ---- Newton ----------------------------------------------------------------------------------------------------------------
C4 = dict(Nx=7, Ny=13, Nz=9)
NEWTON = [
    ("cptr", 2, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25), 86.4),
    ("cpr_TI", 2, dict(pc="cpr", decoup="TI", ksp_rtol=1e-8, snes_max_it=25), 86.4),
    ("cptramg_QI", 2, dict(pc="cptramg", decoup="QI", ksp_rtol=1e-8, snes_max_it=25), 86.4),
    ("1ph_fieldsplit_cd", 1, dict(pc="fieldsplit_cd", ksp_rtol=1e-8), 864.0),
]


def _newton_problem(nphase):
    """c4 7x13x9 with its wells and heaters; one open lateral side (the low side of internal axis 2) at the initial state,
    thermal top and bottom (the sides of internal axis 0) at T_prod."""
    spec, u0, p, *_ = cases.c4_spe10_3d(nphase=nphase, **C4)
    assert spec["gaxis"] == 0
    spec["boundary"] = {
        0: {"kind": "thermal", "p": p.p_ref, "T": p.T_prod, "S": p.S_o if nphase == 2 else None},
        1: {"kind": "thermal", "p": p.p_ref, "T": p.T_prod, "S": p.S_o if nphase == 2 else None},
        4: {"kind": "open", "p": p.p_ref, "T": p.T_prod, "S": p.S_o if nphase == 2 else None},
    }
    for side, e in spec["boundary"].items():
        shape = side_shape(spec["n"], side)
        for k in ("p", "T", "S"):
            if e[k] is not None:
                e[k] = np.full(shape, float(e[k]))
    return spec, u0


def _assert_step(ro, rh, o, h):
    assert ro["reason"] > 0 and rh["reason"] == ro["reason"], (ro, rh)
    assert rh["nits"] == ro["nits"]
    assert abs(rh["lits"] - ro["lits"]) <= max(2, 0.1*ro["lits"])
    uo, uh = o.get_state(), h.get_state()
    assert rel2(uh[0], uo[0]) < 1e-8 and rel2(uh[1], uo[1]) < 1e-8
    if o.b == 3:
        assert np.abs(uh[2] - uo[2]).max() < 1e-8


def _two_steps(spec, u0, opts, dt, between=None):
    from thermalporous_amd.engine import HipEngine
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    for e in (o, h):
        e.set_state(u0)
    for step in range(2):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(dt)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("step %d: oracle nits %d lits %d, engine nits %d lits %d" % (step, ro["nits"], ro["lits"], rh["nits"], rh["lits"]))
        _assert_step(ro, rh, o, h)
        if step == 0 and between is not None:
            between(o, h)
    flux = h.boundary_flux()
    h.close()
    return flux


@pytest.mark.parametrize("name,nphase,opts,dt", NEWTON, ids=[c[0] for c in NEWTON])
def test_newton_parity_with_boundaries(name, nphase, opts, dt):
    spec, u0 = _newton_problem(nphase)
    flux = _two_steps(spec, u0, opts, dt)
    assert np.all(flux[[2, 3, 5]] == 0.0) and np.abs(flux[[0, 1, 4], 1]).min() > 0.0


def test_boundary_values_change_between_steps():
    """The bottom's T_b is replaced after step 1; step 2 matches the oracle given the same change."""
    spec, u0 = _newton_problem(2)
    name, nphase, opts, dt = NEWTON[0]

    before = []

    def between(o, h):
        before.append(h.boundary_flux()[0, 1])
        e = dict(spec["boundary"][0])
        e["T"] = e["T"] + 40.0
        h.set_boundary(0, e["kind"], p=e["p"], T=e["T"], S=e["S"])
        o.prob.boundary[0] = e
    hot = _two_steps(spec, u0, opts, dt, between=between)
    # a wall 40 K hotter than the rock next to it: heat enters through the bottom (negative: it leaves the domain's residual)
    assert hot[0, 1] < 0.0 and hot[0, 1] < before[0] - 10.0*abs(before[0])
