"""Completed wells on the host (no GPU): the numpy reference against a dense complex-step Jacobian, the active-set rounds against
a brute-force solve, the connection index from the true geometry, the spec round-trip and the refusals."""
import numpy as np
import pytest

import cases
from wells_ref import (line_cells, make_well, peaceman, solve_bhp, solve_bhp_brute, tune_wells, wells_problem)


def _small(nphase, seed=3, **kw):
    spec, *_ = cases.c4_spe10_3d(Nx=3, Ny=4, Nz=4, nphase=nphase)
    spec = dict(spec, sources=None)
    u = cases.perturbed_state(spec, seed=seed)
    assert spec["gaxis"] == 0
    n = spec["n"]
    wells = [make_well(spec, "P", "prod", line_cells(spec, 0, (1, 1)), 0, 1.0, 1.0),
             make_well(spec, "I", "inj", line_cells(spec, 0, (0, 2), 1, n[0]), 0, 1.0, 1.0),
             make_well(spec, "H", "prod", line_cells(spec, 2, (2, 2)), 2, 1.0, 1.0),
             make_well(spec, "B", "inj", line_cells(spec, 1, (3, 0)), 1, 1.0, 1.0)]
    prob = wells_problem(spec, wells=wells)
    wells = tune_wells(prob, u, wells, {"P": ("rate", 0.3), "I": ("rate", 0.3), "H": ("bhp", 0.4), "B": ("bhp", 0.4)})
    prob.set_dt(8640.0)
    return spec, u, prob, wells


@pytest.mark.parametrize("nphase", [1, 2])
def test_diagonal_part_plus_rank1_is_the_full_jacobian(nphase):
    spec, u, prob, wells = _small(nphase)
    st = prob.well_state(u)
    modes = [s["mode"] for s in st]
    assert modes == ["rate", "rate", "bhp", "bhp"], modes
    assert any(not s["open"].all() for s in st) and max(s["rounds"] for s in st) >= 2
    assert prob.kink_margin(u) > 1e-3
    J = prob.jacobian(u)
    assert any(np.abs(c).max() > 0 and np.abs(b).max() > 0 for c, b in prob.last_factors)
    D = prob.dense_jacobian(u)
    from oracle import linalg as la
    b, n = prob.b, int(np.prod(prob.shape))
    scale = np.abs(D).max()
    worst = 0.0
    for col in range(b):
        for j in range(n):
            e = np.zeros((b, n))
            e[col, j] = 1.0
            e = e.reshape((b,) + prob.shape)
            y = (la.spmv_block(J, e) + prob.rank1(e)).reshape(b, n)
            worst = max(worst, np.abs(y - D[:, :, col, j]).max())
    print("largest deviation %.3e of %.3e" % (worst, scale))
    assert worst < 1e-12*scale
    # and without the rank-1 term the rate-mode wells' rows are visibly wrong
    x = np.random.default_rng(1).standard_normal((b,) + prob.shape)
    rows = np.concatenate([w["cells"] for w, s in zip(wells, st) if s["mode"] == "rate"])
    r1, y7 = prob.rank1(x).reshape(b, n)[:, rows], la.spmv_block(J, x).reshape(b, n)[:, rows]
    assert np.linalg.norm(r1) > 1e-3*np.linalg.norm(y7)


def test_reference_schur_diagonal_is_the_explicit_temperature_derivative():
    spec, u, prob, wells = _small(2)
    J, Sm = prob.jacobian(u, want_schur=True)
    J0, Sm0 = _plain(spec, u).jacobian(u, want_schur=True)
    d = (Sm - Sm0)[0].reshape(-1)
    prods = [w for w in wells if w["kind"] == "prod"]
    touched = np.concatenate([w["cells"] for w in prods])
    assert np.abs(d[touched]).max() > 0.0
    inj = np.concatenate([w["cells"] for w in wells if w["kind"] == "inj"])
    assert np.all(d[inj] == 0.0)
    rest = np.setdiff1d(np.arange(d.size), np.concatenate([touched, inj]))
    assert np.all(d[rest] == 0.0) and np.all((Sm - Sm0)[1:] == 0.0)


def _plain(spec, u):
    from oracle.tpfa import Problem
    P = Problem(spec)
    P.set_old(u)
    P.set_dt(8640.0)
    return P


@pytest.mark.parametrize("kind", ["prod", "inj"])
def test_active_set_rounds_against_brute_force(kind):
    rng = np.random.default_rng(11)
    seen_rounds = set()
    for trial in range(400):
        n = int(rng.integers(1, 9))
        a = rng.uniform(0.1, 3.0, n)*(rng.random(n) > 0.1)
        th = 40.0 + rng.normal(0.0, 1.0, n)
        Q = float(rng.uniform(0.01, 2.0)*max(a.sum(), 0.1))
        far = -1e9 if kind == "prod" else 1e9
        bhp, mode, opn, rounds, sa = solve_bhp(kind, a, th, Q, far)
        if not a.sum() > 0.0:
            assert mode == "bhp"
            continue
        assert mode == "rate"
        seen_rounds.add(rounds)
        q = np.where(opn, -a*(th - bhp), 0.0)
        assert abs(q.sum() - (-Q if kind == "prod" else Q)) < 1e-12*Q
        found = [f for f in solve_bhp_brute(kind, a, th, Q)]
        assert found, "no consistent open set"
        # the consistent sets may differ in perforations with a = 0 only: one bhp
        assert all(abs(f[0] - bhp) < 1e-12*abs(bhp) for f in found), (bhp, found)
    assert max(seen_rounds) >= 3 and 1 in seen_rounds


def test_limit_switches_the_mode():
    a, th = np.array([1.0, 2.0, 0.5]), np.array([40.0, 41.0, 39.0])
    bhp, mode, opn, _, _ = solve_bhp("prod", a, th, 1.0, 30.0)
    assert mode == "rate" and bhp > 30.0
    b2, mode, opn, _, _ = solve_bhp("prod", a, th, 1.0, float(bhp) + 0.5)
    assert mode == "bhp" and b2 == float(bhp) + 0.5 and list(opn) == [bool(t > b2) for t in th]
    b3, mode, opn, _, _ = solve_bhp("inj", a, th, 1.0, 39.5)
    assert mode == "bhp" and b3 == 39.5 and list(opn) == [False, False, True]


# ---- host package --------------------------------------------------------------------------------------------------------------
def _geo(graded=True):
    from thermalporous_amd.physicalparameters import PhysicalParameters
    from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo
    from thermalporous_amd.spacing import geometric_widths
    p = PhysicalParameters()
    g = HomogeneousBoxGeo(4, 5, 6, p, Length=40.0, Length_y=30.0, Length_z=12.0)
    if graded:
        g.set_spacing(x=geometric_widths(4, 40.0, 1.5), y=geometric_widths(5, 30.0, 1.2, refine="high"), z=geometric_widths(6, 12.0, 1.3))
    rng = np.random.default_rng(5)
    g.K_x = rng.uniform(1.0, 5.0, (4, 5, 6))*1e-13
    g.K_y = rng.uniform(1.0, 5.0, (4, 5, 6))*1e-13
    g.K_z = rng.uniform(0.1, 0.5, (4, 5, 6))*1e-13
    return p, g


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_connection_index_from_the_true_geometry(axis):
    from thermalporous_amd.completedwells import CompletedWellCase
    p, g = _geo()
    hx, hy, hz = g.cell_widths()
    cx, cy, cz = g.centres_1d()
    case = CompletedWellCase(p, g)
    a = "xyz".index(axis)
    L = (40.0, 30.0, 12.0)
    cross = [d for d in range(3) if d != a]
    pt = (cx[2], cy[1], cz[3])
    w = case.add_producer("P", xy=tuple(pt[d] for d in cross), z=(0.0, L[a]), axis=axis, rate=1e-4, bhp=10.0, radius=0.05, skin=0.5)
    N = (4, 5, 6)
    assert len(w["ijk"]) == N[a]
    K = (g.K_x, g.K_y, g.K_z)
    H = (hx, hy, hz)
    for k, c in enumerate(w["ijk"]):
        fixed = (2, 1, 3)
        assert all(c[d] == fixed[d] for d in cross) and c[a] == k
        Ka, Kb = K[cross[0]][c], K[cross[1]][c]
        Da, Db, Lc = H[cross[0]][c[cross[0]]], H[cross[1]][c[cross[1]]], H[a][c[a]]
        ro = 0.28*np.sqrt(np.sqrt(Kb/Ka)*Da**2 + np.sqrt(Ka/Kb)*Db**2)/((Kb/Ka)**0.25 + (Ka/Kb)**0.25)
        want = 2*np.pi*Lc*np.sqrt(Ka*Kb)/(np.log(ro/0.05) + 0.5)
        assert abs(w["WI"][k] - want) < 1e-14*want
        assert w["z"][k] == cz[c[2]]
    assert w["z_ref"] == max(w["z"])
    # the widths matter: the same well on the uniform grid has other indices
    p2, g2 = _geo(graded=False)
    g2.K_x, g2.K_y, g2.K_z = g.K_x, g.K_y, g.K_z
    w2 = CompletedWellCase(p2, g2).add_producer("P", cells=w["ijk"], axis=axis, rate=1e-4, bhp=10.0, radius=0.05, skin=0.5)
    assert np.abs(w2["WI"]/w["WI"] - 1.0).max() > 1e-2


def test_connection_index_reduces_to_the_hard_coded_one():
    from thermalporous_amd.completedwells import connection_index
    from thermalporous_amd.wellcase import peaceman_WI
    assert abs(connection_index(2e-13, 3e-13, 5.0, 5.0, 5.0) - peaceman_WI(2e-13, 3e-13)) < 1e-15*peaceman_WI(2e-13, 3e-13)
    assert abs(peaceman(2e-13, 3e-13, 5.0, 5.0, 5.0) - peaceman_WI(2e-13, 3e-13)) < 1e-15*peaceman_WI(2e-13, 3e-13)


def test_spec_round_trip_and_base_case_passes_through():
    from thermalporous_amd.completedwells import CompletedWellCase
    from thermalporous_amd.engine import check_wells
    from thermalporous_amd.heatercase import HeaterCase
    from thermalporous_amd.problem import build_spec, phys_flat_to_internal
    p, g = _geo()
    base = HeaterCase(p, g, heater_points=[[10.0, 10.0, 6.0]])
    ref = build_spec(g, base, p, 2)
    case = CompletedWellCase(p, g, base=base)
    case.add_producer("P1", xy=(12.0, 9.0), z=(2.0, 11.0), rate=2e-4, bhp=20.0)
    case.add_injector("I1", xy=(25.0, 6.0), z=(0.0, 40.0), axis="x", rate=1e-4, bhp=60.0)
    spec = build_spec(g, case, p, 2)
    for k in ref["sources"]:
        assert np.array_equal(spec["sources"][k], ref["sources"][k])          # the base's entries, untouched
    assert "wells" not in ref and [w["name"] for w in spec["wells"]] == ["P1", "I1"]
    ws = check_wells(spec["wells"], 4*5*6)
    for w, e in zip(ws, case.well_entries()):
        assert np.array_equal(w["cells"], phys_flat_to_internal(e["cells"], g, spec["axes"]))
        assert np.array_equal(w["WI"], e["WI"]) and np.array_equal(w["z"], e["z"])
        assert (w["kind"], w["rate"], w["bhp"], w["z_ref"], w["shut"]) == (e["kind"], e["rate"], e["bhp"], e["z_ref"], False)
    # the internal cells are the cells: elevation = the centre along the gravity axis of the internal index
    n = spec["n"]
    zc = np.cumsum(spec["hs"][spec["gaxis"]]) - 0.5*spec["hs"][spec["gaxis"]]
    for w in ws:
        idx = [w["cells"] % n[0], (w["cells"]//n[0]) % n[1], w["cells"]//(n[0]*n[1])]
        assert np.allclose(zc[idx[spec["gaxis"]]], w["z"], rtol=1e-14)
    # the spacing is locked as the other cases lock it
    with pytest.raises(RuntimeError, match="set_spacing"):
        g.set_spacing()


def test_refusals_on_the_host():
    from thermalporous_amd.completedwells import CompletedWellCase
    from thermalporous_amd.engine import check_wells, check_wells_slabs
    p, g = _geo()
    case = CompletedWellCase(p, g)
    case.add_producer("P", xy=(12.0, 9.0), z=(2.0, 11.0), rate=2e-4, bhp=20.0)
    with pytest.raises(ValueError, match="already perforated by well 'P'"):
        case.add_injector("I", xy=(12.0, 9.0), z=(0.0, 3.0), rate=1e-4, bhp=60.0)
    with pytest.raises(ValueError, match="two wells are called 'P'"):
        case.add_producer("P", xy=(30.0, 9.0), z=(2.0, 11.0), rate=2e-4, bhp=20.0)
    with pytest.raises(ValueError, match="rate"):
        case.add_producer("Q", xy=(30.0, 9.0), z=(2.0, 11.0), rate=-1.0, bhp=20.0)
    with pytest.raises(ValueError, match="no cell centre"):
        case.add_producer("Q", xy=(30.0, 9.0), z=(100.0, 110.0), rate=1.0, bhp=20.0)
    with pytest.raises(ValueError, match="outside the grid"):
        case.add_producer("Q", cells=[(9, 0, 0)], rate=1.0, bhp=20.0)
    with pytest.raises(ValueError, match="axis"):
        case.add_producer("Q", xy=(30.0, 9.0), z=(2.0, 11.0), axis="w", rate=1.0, bhp=20.0)
    good = dict(name="W", kind="prod", rate=1.0, bhp=2.0, cells=[3, 4], WI=[1.0, 2.0], z=[0.0, 1.0])
    assert check_wells([good], 10)[0]["z_ref"] == 1.0
    for bad, msg in ((dict(good, rate=-1.0), "rate = -1.0"), (dict(good, WI=[1.0, 0.0]), "WI = 0.0 at perforation 1"),
                     (dict(good, cells=[3, 10]), "cell 10 lies outside"), (dict(good, bhp=np.nan), "finite"),
                     (dict(good, kind="heater"), "kind = 'heater'"), (dict(good, z=[0.0]), "one of each per perforation")):
        with pytest.raises(ValueError, match=msg):
            check_wells([bad], 10)
    with pytest.raises(ValueError, match="cell 4 is already perforated by well 'W'"):
        check_wells([good, dict(good, name="V", cells=[4, 5])], 10)
    with pytest.raises(NotImplementedError, match="W.*nranks = 2"):
        check_wells_slabs([good], nranks=2)
    check_wells_slabs([], nranks=2)
    check_wells_slabs(None, nranks=4)


def test_cabi_declares_the_wells():
    import os
    import re
    from thermalporous_amd import engine
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "thermalporous_hip.h")).read()
    for sym in ("tp_set_wells", "tp_set_well_control", "tp_well_info", "tp_well_perf_rates", "tp_well_factors"):
        assert sym in engine.API_SYMBOLS and re.search(r"\bint %s\(" % sym, hdr)
    assert all(hasattr(engine.HipEngine, m) for m in ("set_wells", "set_well_control", "well_info", "well_perf_rates", "well_factors"))
    import ctypes as C
    assert C.sizeof(engine.tp_well) == 40 and C.sizeof(engine.tp_perf) == 24 and C.sizeof(engine.tp_well_state) == 56
