"""Saturation functions on the GPU (tp_set_saturation_functions; the SATFN instantiations of k_assemble, k_assemble_bc, k_accum_old
and k_sources in csrc/tp_assembly.hip) against the numpy reference tests/satfn_ref.py, whose Jacobian and S~
are complex steps of its own residual: entries of R, J and S~ with test_gpu_assembly_edges' rule at states that hold every
branch of every curve, the default path bit for bit, the degenerate Corey case against the existing oracle, no flow below the
residual saturation, conservation, the capillary-gravity column, wells, Dirichlet sides, a graded grid, slabs, Newton solves
with test_gpu_bc's assertions, the time loop, and the library's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cases
from bc_ref import assert_both_directions, make_boundary
from graded_ref import field_change, random_widths, spec_lengths
from oracle.tpfa import INJ, PROD, Problem
from oracle.engine import OracleEngine
from satfn_ref import DEFAULT, DEGENERATE, M1, M2, M3, MODELS, capillary_gravity_column, column_face_fluxes
from test_gpu_assembly_edges import TOL, assert_entries
from test_gpu_bc import _assert_step
from test_gpu_slabs import rel2, run_slabs

pytestmark = pytest.mark.gpu

BOXES = [
    ("2ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=2)),
    ("2ph_3d_6x5x4", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2)),       # the two axis permutations, gravity on
    ("2ph_3d_5x6x4", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4, nphase=2)),       # internal axis 0
    ("2ph_line_1x1x5", cases.c4_spe10_3d, dict(Nx=1, Ny=1, Nz=5, nphase=2)),
]
B654 = BOXES[1]
OPTS = dict(pc="cptr")


def _engine(spec, u, dt=8640.0, opts=None):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts or OPTS)
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


def _gpu(h):
    R = h.residual()
    J, Sm = h.jacobian(want_schur=True)
    return R, J, Sm


def _bits(h):
    return tuple(a.tobytes() for a in _gpu(h))


def _with(spec, sat):
    return dict(spec, satfn={**DEFAULT, **sat})


def _edge_state(spec, sat):
    """cases.perturbed_state(seed=3), whose S_o in [0.02, 0.98] lies on both sides of both ends, with the first three cells set
    exactly to S_o = Sr_o, S_o = 1 - Sr_w, and the S_o at which Se_w = pc_se_min."""
    sat = {**DEFAULT, **sat}
    u = cases.perturbed_state(spec, seed=3)
    S = u[2].reshape(-1)
    D = 1.0 - sat["Sr_o"] - sat["Sr_w"]
    S[0], S[1], S[2] = sat["Sr_o"], 1.0 - sat["Sr_w"], 1.0 - sat["Sr_w"] - sat["pc_se_min"]*D
    return u


def _branches(sat, S):
    """The branches of the curves of `sat` that hold at least one cell of S: (curve, "low" | "in" | "high")."""
    sat = {**DEFAULT, **sat}
    D = 1.0 - sat["Sr_o"] - sat["Sr_w"]
    Se_o, Se_w = (S - sat["Sr_o"])/D, ((1.0 - sat["Sr_w"]) - S)/D
    out = set()
    for name, Se, lo in (("kr_o", Se_o, 0.0), ("kr_w", Se_w, 0.0), ("pc", Se_w, sat["pc_se_min"] if sat["capillary"] == "brooks_corey" else 0.0)):
        if name == "pc" and sat["capillary"] is None:
            continue
        for tag, m in (("low", Se <= lo), ("in", (Se > lo) & (Se < 1.0)), ("high", Se >= 1.0)):
            if m.any():
                out.add((name, tag))
    return out


def _all_branches(sat):
    names = ("kr_o", "kr_w") + (("pc",) if {**DEFAULT, **sat}["capillary"] else ())
    return {(n, t) for n in names for t in ("low", "in", "high")}


# ---- entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,builder,kw", BOXES, ids=[b[0] for b in BOXES])
@pytest.mark.parametrize("model", ["M1", "M2", "M3"])
def test_entries_against_the_reference(model, pid, builder, kw):
    sat = MODELS[model]
    spec, *_ = builder(**kw)
    spec = _with(spec, sat)
    u = _edge_state(spec, sat)
    S = u[2].reshape(-1)
    assert S[0] == sat["Sr_o"] and S[1] == 1.0 - sat["Sr_w"]
    want = _all_branches(sat)
    if pid == "2ph_line_1x1x5":
        # five cells, three of them set: beside those only two states remain, and no cell of the line reaches Se_o >= 1 (at
        # S_o = 1 - Sr_w the quotient rounds to 1 - 2^-52); the three boxes above hold that branch
        want -= {("kr_o", "high")}
    assert _branches(sat, S) >= want, (model, pid, sorted(want - _branches(sat, S)))
    Ro, Jo, So = _reference(Problem(spec), u)
    h = _engine(spec, u)
    assert h.saturation_info()["active"]
    Rh, Jh, Sh = _gpu(h)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, (model, pid))
    # the curves are visible in what is compared: the result is not the linear model's
    Pl = Problem({k: v for k, v in spec.items() if k != "satfn"})
    Pl.set_old(u)
    Pl.set_dt(8640.0)
    change = field_change(Rh, Pl.residual(u), spec)
    print("%s %s: the residual fields differ from the linear oracle's by %r" % (model, pid, change))
    assert min(change) > 0.01
    h.close()


def test_default_path_is_untouched():
    """c4 box 7x13x9: an engine never told about saturation functions, one on which M2 is set and then cleared and one given the
    explicit linear / no-p_c setting give bitwise equal R, J and S~; while M2 is set the bits differ."""
    spec, *_ = cases.c4_spe10_3d(Nx=7, Ny=13, Nz=9, nphase=2)
    u = cases.perturbed_state(spec, seed=3)
    a, b, c = _engine(spec, u), _engine(spec, u), _engine(spec, u)
    plain = _bits(a)
    assert _bits(b) == plain
    b.set_saturation_functions(M2)
    info = b.saturation_info()
    assert info["active"] and info["relperm"] == "corey" and info["n_o"] == 4.0 and info["capillary"] == "linear" and info["p_ct"] == 0.05
    moved = _bits(b)
    assert all(x != y for x, y in zip(moved, plain))
    b.set_saturation_functions(None)
    assert not b.saturation_info()["active"] and b.satfn is None and _bits(b) == plain
    c.set_saturation_functions(dict(relperm="linear", capillary=None, Sr_o=0.3, n_w=5.0))
    assert not c.saturation_info()["active"] and c.satfn is None and _bits(c) == plain
    assert _bits(a) == plain
    for h in (a, b, c):
        h.close()


def test_degenerate_corey_equals_the_existing_oracle():
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    u = cases.perturbed_state(spec, seed=3)
    o = OracleEngine(spec, OPTS)
    o.set_old(u)
    o.set_dt(8640.0)
    o.set_state(u)
    Ro = o.residual()
    Jo, So = o.jacobian(want_schur=True)
    h = _engine(_with(spec, DEGENERATE), u)
    assert h.saturation_info()["active"]
    Rh, Jh, Sh = _gpu(h)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    rh, ro = h.well_rates(), o.well_rates()
    for k in ro:
        assert np.allclose(rh[k], ro[k], rtol=1e-12, atol=1e-30), k
    h.close()


def test_no_flow_below_the_residual_saturation():
    """M1: an interior cell at S_o = Sr_o - 0.05 and a pressure above all its neighbours holds immobile oil: in every
    neighbour's row, the block that carries the derivatives with respect to that cell's state has an oil row of exact zeros."""
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    spec = _with(spec, M1)
    n0, n1, n2 = spec["n"]
    u = _edge_state(spec, M1)
    i0, i1, i2 = 1, 2, 3
    u[2][i2, i1, i0] = M1["Sr_o"] - 0.05
    u[0][i2, i1, i0] = u[0].max() + 5.0
    h = _engine(spec, u)
    _, Jh, _ = _gpu(h)
    seen = 0
    for a, (d0, d1, d2) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        for sgn, slot in ((-1, 2 + 2*a), (1, 1 + 2*a)):      # the neighbour below sees the cell in its +a slot, the one above in -a
            j0, j1, j2 = i0 + sgn*d0, i1 + sgn*d1, i2 + sgn*d2
            assert 0 <= j0 < n0 and 0 <= j1 < n1 and 0 <= j2 < n2
            block = Jh[slot, :, :, j2, j1, j0]
            assert np.all(block[2] == 0.0), (slot, block)
            assert np.abs(block[0]).max() > 0.0          # (water does leave the cell: the block is not empty)
            seen += 1
    assert seen == 6
    h.close()


def test_conservation():
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    spec = _with(spec, M2)
    spec["sources"] = None
    u = _edge_state(spec, M2)
    h = _engine(spec, u)
    R = h.residual()
    for f in range(3):
        print("field %d: sum %.3e, sum of |R| %.3e" % (f, R[f].sum(), np.abs(R[f]).sum()))
        assert np.abs(R[f]).sum() > 0.0 and abs(R[f].sum()) < 1e-12*np.abs(R[f]).sum()
    h.close()


# (the time step is free and enters nothing but the accumulation, whose rounding it keeps below the face fluxes: the reasoning of
# test_gpu_graded.HYDROSTATIC_DT)
COLUMN_DT = 1e10


def test_capillary_gravity_column_carries_no_flow():
    """1 x 1 x 8, API 40, linear p_c: the state tests/satfn_ref.py marches up from Se_w = 0.9 at the bottom so that both driving
    forces vanish on every face; old state = state: each phase's flux through each face is below 1e-8 of T^K L rho g dz."""
    spec, u, scale = capillary_gravity_column()
    P = Problem(spec)
    h = _engine(spec, u, dt=COLUMN_DT)
    F = column_face_fluxes(P, h.residual())
    print("face fluxes / (T^K L rho g dz): water", F[0]/scale[0], "oil", F[1]/scale[1])
    assert np.all(np.abs(F) < 1e-8*scale)
    h.close()
    # the capillary pressure is what holds the water up: without it the same column flows
    h0 = _engine({k: v for k, v in spec.items() if k != "satfn"}, u, dt=COLUMN_DT)
    F0 = column_face_fluxes(P, h0.residual())
    print("linear curves, no p_c: water", F0[0]/scale[0])
    assert np.abs(F0[0]/scale[0]).max() > 0.05
    h0.close()


# ---- wells -------------------------------------------------------------------------------------------------------------------
def test_wells_follow_the_curves():
    """M1: a producer cell below Sr_o lifts no oil, one above 1 - Sr_w no water, exactly; a constant-rate producer and an injector
    beside them; rates, R, J and S~ against the reference."""
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    spec = _with(spec, M1)
    src = spec["sources"]
    ip = int(np.nonzero(src["kind"] == PROD)[0][0])
    ii = int(np.nonzero(src["kind"] == INJ)[0][0])
    pick = [ip, ip, ip, ii]
    cells = np.array([13, 41, 66, 97], dtype=np.int64)
    spec["sources"] = {k: np.array([src[k][j] for j in pick]) for k in src}
    spec["sources"]["cell"] = cells
    spec["sources"]["const"] = np.array([0, 0, 1, 0], dtype=np.int32)
    u = _edge_state(spec, M1)
    S = u[2].reshape(-1)
    S[13], S[41], S[66] = 0.1, 0.9, 0.55
    P = Problem(spec)
    Ro, Jo, So = _reference(P, u)
    c = cells
    _, ro = P.source_terms(u[0].reshape(-1)[c], u[1].reshape(-1)[c], S[c], return_rates=True)
    h = _engine(spec, u)
    Rh, Jh, Sh = _gpu(h)
    rh = h.well_rates()
    print("rates:", rh)
    assert rh["oil_rate"][0] == 0.0 and rh["water_rate"][0] != 0.0
    assert rh["water_rate"][1] == 0.0 and rh["oil_rate"][1] != 0.0
    assert rh["rate"][2] == spec["sources"]["max_rate"][2] and rh["oil_rate"][2] != 0.0 and rh["water_rate"][2] != 0.0
    assert rh["rate"][3] != 0.0
    for k in ro:
        assert np.abs(rh[k] - ro[k].real).max() <= TOL*np.abs(ro[k]).max(), k
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, "wells")
    h.close()


# ---- with the other two model features ---------------------------------------------------------------------------------------
def test_with_dirichlet_sides():
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    spec = _with(spec, M2)
    assert spec["gaxis"] == 0
    u = _edge_state(spec, M2)
    axes = spec["axes"]
    z_lo, x_hi = 2*axes.index(2), 2*axes.index(0) + 1           # 'z-' and 'x+' as internal sides
    spec["boundary"] = make_boundary(spec, u, {z_lo: "open", x_hi: "thermal"}, seed=4)
    P = Problem(spec)
    Ro, Jo, So = _reference(P, u)
    assert_both_directions(P)
    ref = P.last_flux.copy()
    h = _engine(spec, u)
    Rh, Jh, Sh = _gpu(h)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    flux = h.boundary_flux()
    for q in range(3):
        assert np.abs(flux[:, q] - ref[:, q]).max() < 1e-11*np.abs(ref[:, q]).max(), (q, flux[:, q], ref[:, q])
    h.close()


def test_on_a_graded_grid():
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    spec = _with(spec, M2)
    spec["hs"] = random_widths(spec["n"], spec_lengths(spec), 7)
    u = _edge_state(spec, M2)
    Ro, Jo, So = _reference(Problem(spec), u)
    h = _engine(spec, u)
    assert h.spacing_info()["graded"] and h.saturation_info()["active"]
    Rh, Jh, Sh = _gpu(h)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    h.close()


def test_on_two_slabs():
    """M2 through test_gpu_slabs.run_slabs with two in-process slabs against one slab, with that suite's assertions."""
    from thermalporous_amd.engine import HipEngine
    pid, builder, kw = B654
    spec, u0, *_ = builder(**kw)
    spec = _with(spec, M2)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    dts = [40.0, 80.0]
    h = HipEngine(spec, opts)
    h.set_state(u0)
    ref = []
    for dt in dts:
        h.set_old(None)
        h.set_dt(dt)
        ref.append(h.newton_solve())
    u_ref = h.get_state()
    h.close()
    assert all(r["reason"] > 0 for r in ref)
    infos, u_n = run_slabs(spec, opts, u0, dts, 2)
    for i_n, i_1 in zip(infos, ref):
        assert i_n["reason"] == i_1["reason"] and i_n["nits"] == i_1["nits"]
        assert abs(i_n["lits"] - i_1["lits"]) <= max(3, 0.2*i_1["lits"])
    for f in range(3):
        assert rel2(u_n[f], u_ref[f]) < 1e-7


# ---- Newton ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["M1", "M2"])
def test_newton_parity(model):
    from thermalporous_amd.engine import HipEngine
    pid, builder, kw = B654
    spec, u0, *_ = builder(**kw)
    spec = _with(spec, MODELS[model])
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    for e in (o, h):
        e.set_state(u0)
    for step in range(3):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(86.4)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("step %d: oracle nits %d lits %d, engine nits %d lits %d" % (step, ro["nits"], ro["lits"], rh["nits"], rh["lits"]))
        _assert_step(ro, rh, o, h)
    h.close()


# ---- time loop ---------------------------------------------------------------------------------------------------------------
def test_time_loop_of_the_water_flood():
    """examples/test3D_waterflood_corey.py's box at 6 x 5 x 4 under M2: no failed solve, S_o in [0, 1], and with a water injector
    and a producer as the only sources the oil in place never increases (beyond the Newton tolerance, 1e-8 relative)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import test3D_waterflood_corey as ex
    finally:
        sys.path.pop(0)
    m = ex.build(6, 5, 4, satfn=M2, maxdt=0.5, end=4.0)
    assert m.spec["satfn"]["relperm"] == "brooks_corey" and m.engine.saturation_info()["active"]
    assert set(m.spec["sources"]["kind"].tolist()) == {PROD, INJ}
    oil, step = [], m.step

    def recording_step():
        out = step()
        oil.append(m.oil_mass())
        return out
    m.step = recording_step
    m.solve()
    S = m.u._read()[2]
    print("steps %d, failed solves %d, S_o in [%.4f, %.4f], oil in place %.6g -> %.6g" % (len(oil), m.failed_solves, S.min(), S.max(), oil[0], oil[-1]))
    assert m.failed_solves == 0 and len(oil) >= 8
    assert S.min() >= 0.0 and S.max() <= 1.0
    assert all(b <= a*(1.0 + 1e-8) for a, b in zip(oil, oil[1:])) and oil[-1] < oil[0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_error_code_with_a_message():
    from thermalporous_amd import engine as E
    pid, builder, kw = B654
    spec, *_ = builder(**kw)
    u = cases.perturbed_state(spec, seed=3)
    h = _engine(spec, u)
    lib = h.lib
    plain = h.residual().tobytes()

    def call(ctx, **bad):
        st = E.pack_satfn(M3)
        for k, v in bad.items():
            setattr(st, k, v)
        return lib.tp_set_saturation_functions(ctx, C.byref(st))
    for key, bad in (("Sr_o + Sr_w", dict(Sr_o=0.6, Sr_w=0.4)), ("Sr_o", dict(Sr_o=-0.1)), ("n_o", dict(n_o=0.5)), ("n_w", dict(n_w=0.0)),
                     ("lmbda", dict(lmbda=0.0)), ("lmbda", dict(lmbda=-1.0)), ("pc_se_min", dict(pc_se_min=0.0)),
                     ("pc_se_min", dict(pc_se_min=1.5)), ("kro_max", dict(kro_max=0.0)), ("p_ct", dict(p_ct=-1.0)),
                     ("Sr_w", dict(Sr_w=float("nan"))), ("p_ct", dict(p_ct=float("inf"))), ("krw_max", dict(krw_max=float("-inf"))),
                     ("relperm", dict(relperm=2)), ("capillary", dict(capillary=3))):
        assert call(h.ctx, **bad) != 0, bad
        assert key in lib.tp_last_error().decode(), (key, lib.tp_last_error().decode())
    # none of them changed the context
    assert not h.saturation_info()["active"] and h.residual().tobytes() == plain
    with pytest.raises(ValueError, match="lmbda"):
        h.set_saturation_functions(dict(M3, lmbda=0.0))
    h.close()
    # a single-phase context
    spec1, *_ = cases.c4_spe10_3d(Nx=4, Ny=5, Nz=6, nphase=1)
    h1 = _engine(spec1, cases.perturbed_state(spec1, seed=3), opts=dict(pc="fieldsplit_cd"))
    assert call(h1.ctx) != 0
    assert "single-phase" in lib.tp_last_error().decode()
    assert lib.tp_set_saturation_functions(h1.ctx, None) == 0                      # (clearing is no setting)
    with pytest.raises(NotImplementedError, match="single-phase"):
        h1.set_saturation_functions(M1)
    h1.close()
