"""The graded (GRADED), boundary (k_assemble_bc, k_bc_trans, k_bc_trans_g) and saturation-function (SATFN) instantiations of the
assembly in csrc/tp_assembly.hip, alone and combined -- the triple k_assemble_bc<2, JAC, SCHUR, true, true> among them -- at the
states where a TPFA kernel goes wrong (tests/edge_cases.py): saturations 0, 1, -0.05 and 1.05 in the cells and 0 and 1 in the
ghosts, exact upwind ties inside and on boundary faces (gt, not ge), dead cells inside and on a side, porosity 0 and 1 on a side,
no conduction at all (every guard of a conduction denominator false), a side list longer than one workgroup, and neighbour
width ratios of 4.  tp_residual, tp_jacobian (J and S~) and tp_boundary_flux against the numpy reference class that matches the
combination (edge_cases.combo_problem), old state = state, dt = 8640.

Per case: test_gpu_assembly_edges' rule (1e-11 of the largest entry of the field / block); a per-row rule -- per cell and
equation, the row of J (7 b entries) and of S~ (7 entries) within TOL_ROW of the row's own largest reference entry, the residual
per cell within TOL_ROW of edge_cases.per_cell_scales' scale -- under which a thin cell of a graded grid is held to its own
size and not to the grid's largest entry; rows the reference has exactly zero exactly zero; the side sums.

TOL_ROW = max(1e-11, 10 x 3.1e-15) = 1e-11: 3.1e-15 is the largest per-row difference between the analytic and the
complex-step Jacobian of the graded reference with sides at the inputs of row 3, measured by
test_graded_host.test_per_row_bound_of_the_combination_tests.

The conditions that make a case informative are asserted on the reference, on the CPU, by edge_cases.combo_input.  Every input is
finite and so is every reference output."""
import numpy as np
import pytest

import edge_cases as ec
from test_gpu_assembly_edges import assert_entries
from test_gpu_bc import _assert_step

pytestmark = pytest.mark.gpu

CASES = ec.combo_cases()


def _opts(nphase):
    return dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")


def _engine(spec, u, dt=ec.COMBO_DT):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, _opts(spec["nphase"]))
    h.set_old(u)
    h.set_dt(dt)
    h.set_state(u)
    return h


def _simpler(spec):
    """[(what, spec without it)]: the next-simpler combinations."""
    return [(name, {k: v for k, v in spec.items() if k != key})
            for name, key in (("spacing", "hs"), ("sides", "boundary"), ("curves", "satfn")) if spec.get(key) is not None]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_combination_against_its_reference(case):
    from bc_ref import side_slice
    spec, u = ec.combo_input(case)
    P, Ro, Jo, So = ec.combo_reference(spec, u)
    b = P.b
    sides = spec.get("boundary") or {}
    h = _engine(spec, u)
    assert h.spacing_info()["graded"] == bool(case["graded"])
    if spec["nphase"] == 2:
        assert h.saturation_info()["active"] == (case["model"] is not None)
    Rh = h.residual()
    flux_r = h.boundary_flux() if sides else None
    Jh, Sh = h.jacobian(want_schur=True)
    flux_j = h.boundary_flux() if sides else None
    h.close()
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, case["id"])

    # ---- per row: every cell against its own scale
    eJ, eS = ec.per_row_errors(Jh, Sh, Jo, So)
    eR = ec.per_cell_residual_error(P, u, Rh, Ro, Jo)
    print("%s: largest per-row difference J %.3e, S~ %.3e, per-cell residual %.3e" % (case["id"], eJ, eS, eR))
    assert eJ <= ec.TOL_ROW, (case["id"], "J per row", eJ)
    assert eS <= ec.TOL_ROW, (case["id"], "S~ per row", eS)
    assert eR <= ec.TOL_ROW, (case["id"], "R per cell", eR)
    # ---- rows the reference has exactly zero (a dead cell of porosity 0: its mass rows) are exactly zero
    zero = np.abs(Jo).max(axis=(0, 2)) == 0.0
    assert np.all(np.abs(Jh).max(axis=(0, 2))[zero] == 0.0)
    szero = np.abs(So).max(axis=0) == 0.0
    assert np.all(np.abs(Sh).max(axis=0)[szero] == 0.0)

    # ---- the side sums
    if sides:
        ref = P.last_flux
        assert flux_r.shape == (6, b) and flux_j.tobytes() == flux_r.tobytes()
        for q in range(b):
            top = np.abs(ref[:, q]).max()
            if top == 0.0:
                assert np.all(flux_r[:, q] == 0.0), q
            else:
                assert np.abs(flux_r[:, q] - ref[:, q]).max() <= 1e-11*top, (q, flux_r[:, q], ref[:, q])
        assert all(np.all(flux_r[s] == 0.0) for s in range(6) if s not in sides)
        mass = [0] if b == 2 else [0, 2]
        all_dead = 0
        for s, e in sides.items():
            if e["kind"] == "open" and all(np.all(np.asarray(k)[side_slice(s)] == 0.0) for k in spec["K"]):
                assert np.all(flux_r[s, mass] == 0.0), (s, flux_r[s])
                all_dead += 1
        if case["kind"] == "dead_on_side" and "2x2x2" in case["box"]:
            assert all_dead == 6
        if case["row"] == 7:
            on = np.zeros(P.shape, dtype=bool)
            for s in sides:
                on[side_slice(s)] = True
            assert on.sum() > 256, "the side list fits one workgroup"

    # ---- the combination is visible in what is compared: the GPU's residual is not the next-simpler reference's
    every_cell_dead = all(np.all(np.asarray(k) == 0.0) for k in spec["K"])
    for what, simpler in _simpler(spec):
        Rs = ec.combo_reference(simpler, u)[1]
        # (the reference itself says in which fields the difference can be seen: uniform p moves no mass, a box of dead cells
        # only conducts, below its heaters' scale)
        seen = [f for f in range(b) if np.abs(Ro[f] - Rs[f]).max() > 2e-4*np.abs(Ro[f]).max()]
        assert seen or every_cell_dead, (case["id"], what)
        if case["kind"] in ("sat", "plain", "boundary_sat_edges") and "2x2x2" not in case["box"]:
            assert len(seen) == b, (case["id"], what, seen)
        for f in seen:
            assert np.abs(Rh[f] - Rs[f]).max() > 1e-4*np.abs(Rh[f]).max(), (case["id"], what, f)


# ---- Newton ------------------------------------------------------------------------------------------------------------------
def test_newton_parity_on_a_graded_box_with_sides_and_curves():
    """Two-phase 6x5x4 with its wells and heaters, pc_cptr, geometric widths along x and z, an open lateral side and a thermal
    top, model M2: two time steps against the oracle engine on the same spec, with test_gpu_graded_model's assertions
    (equal Newton counts, linear iterations within max(2, 10 %), states to 1e-8)."""
    import cases
    from bc_ref import side_shape
    from graded_ref import equal_widths, spec_lengths
    from oracle.engine import OracleEngine
    from oracle.tpfa import GradedGeometry
    from satfn_ref import DEFAULT, M2
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.spacing import geometric_widths
    spec, u0, p, *_ = cases.c4_spe10_3d(Nx=6, Ny=5, Nz=4, nphase=2)
    assert spec["gaxis"] == 0 and spec["axes"][0] == 2
    ax = spec["axes"].index(0)                                      # x as an internal axis
    hs = list(equal_widths(spec))
    L = spec_lengths(spec)
    hs[0] = geometric_widths(spec["n"][0], L[0], 1.5, refine="both")
    hs[ax] = geometric_widths(spec["n"][ax], L[ax], 1.4, refine="low")
    spec["hs"] = tuple(hs)
    spec["satfn"] = {**DEFAULT, **M2}
    spec["boundary"] = {}
    for side, kind in ((2*ax, "open"), (1, "thermal")):
        shape = side_shape(spec["n"], side)
        spec["boundary"][side] = {"kind": kind, "p": np.full(shape, float(p.p_ref)), "T": np.full(shape, float(p.T_prod)),
                                  "S": np.full(shape, float(p.S_o))}
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    assert isinstance(o.prob.geom, GradedGeometry) and o.prob.sat is not None and sorted(o.prob.boundary) == sorted(spec["boundary"])
    assert h.spacing_info()["graded"] and h.saturation_info()["active"] and sorted(h.boundary) == sorted(spec["boundary"])
    for e in (o, h):
        e.set_state(u0)
    for step in range(2):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(86.4)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("step %d: oracle nits %d lits %d, engine nits %d lits %d" % (step, ro["nits"], ro["lits"], rh["nits"], rh["lits"]))
        _assert_step(ro, rh, o, h)
    flux = h.boundary_flux()
    assert np.abs(flux[[2*ax, 1], 1]).min() > 0.0 and np.abs(flux[2*ax, [0, 2]]).min() > 0.0 and np.all(flux[1, [0, 2]] == 0.0)
    h.close()
