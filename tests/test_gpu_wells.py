"""Completed wells on the GPU (k_wells, k_well_rho, k_well_apply of csrc/tp_wells.hip; tp_set_wells and its queries) against the
numpy reference (tests/wells_ref.py): entries of R, J, S~ and of the rank-1 factors with test_gpu_assembly_edges' rule, the Krylov
operator, the well's own invariants, and Newton solves with test_gpu_bc's assertions."""
import ctypes as C
import threading

import numpy as np
import pytest

import cases
from satfn_ref import M2
from test_gpu_assembly_edges import TOL, assert_entries
from test_gpu_bc import _assert_step
from test_gpu_parity import rel2
from wells_ref import line_cells, make_well, tune_wells, wells_oracle, wells_problem

pytestmark = pytest.mark.gpu

DT = 8640.0
PLAN4 = {"P": ("rate", 0.3), "I": ("rate", 0.3), "H": ("bhp", 0.4), "B": ("bhp", 0.4)}


def _opts(nphase):
    return dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")


def _four_wells(spec, hs=None):
    """A vertical producer and injector (internal axis 0 is z in 3-D), a producer along internal axis 2 (its cells a whole plane
    apart in memory) and an injector along axis 1."""
    n = spec["n"]
    return [make_well(spec, "P", "prod", line_cells(spec, 0, (1, 1)), 0, 1.0, 1.0, hs),
            make_well(spec, "I", "inj", line_cells(spec, 0, (0, 2), 1, n[0]), 0, 1.0, 1.0, hs),
            make_well(spec, "H", "prod", line_cells(spec, 2, (2, 2)), 2, 1.0, 1.0, hs),
            make_well(spec, "B", "inj", line_cells(spec, 1, (3, 0)), 1, 1.0, 1.0, hs)]


def _wells_2d(spec, hs=None):
    """7 x 5: a producer along x (internal axis 0), an injector along y, and one-cell wells in BHP mode."""
    return [make_well(spec, "P", "prod", line_cells(spec, 0, (1, 0)), 0, 1.0, 1.0, hs),
            make_well(spec, "I", "inj", line_cells(spec, 1, (5, 0), 2, 5), 1, 1.0, 1.0, hs),
            make_well(spec, "H", "prod", line_cells(spec, 0, (3, 0), 0, 4), 0, 1.0, 1.0, hs),
            make_well(spec, "B", "inj", line_cells(spec, 1, (6, 0), 2, 4), 1, 1.0, 1.0, hs)]


def _column_wells(spec, hs=None):
    """3 x 3 x 70: a producer over all 70 layers (more perforations than a wavefront has lanes) and an injector over 66."""
    return [make_well(spec, "P", "prod", line_cells(spec, 0, (1, 1)), 0, 1.0, 1.0, hs),
            make_well(spec, "B", "inj", line_cells(spec, 0, (0, 2), 2, 68), 0, 1.0, 1.0, hs)]


def _graded(spec):
    from graded_ref import random_widths, spec_lengths
    return random_widths(spec["n"], spec_lengths(spec), seed=4)


def _open_side(spec, u):
    from bc_ref import make_boundary
    return make_boundary(spec, u, {4: "open", 1: "thermal"}, seed=6)


ENTRY = [
    ("2ph_3d_6x5x4", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), _four_wells, PLAN4, {}),
    ("2ph_3d_5x6x4", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4, nphase=2), _four_wells, PLAN4, {}),
    ("1ph_3d_6x5x4", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=1), _four_wells, PLAN4, {}),
    ("2ph_2d_7x5", cases.c3_spe10_2d, dict(Nx=7, Ny=5, nphase=2), _wells_2d, PLAN4, {}),
    ("2ph_column_3x3x70", cases.c4_spe10_3d, dict(Nx=3, Ny=3, Nz=70, nphase=2), _column_wells, {"P": ("rate", 0.3), "B": ("bhp", 0.4)}, {}),
    ("2ph_3d_6x5x4_graded", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), _four_wells, PLAN4, dict(graded=True)),
    ("2ph_3d_6x5x4_open_side", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), _four_wells, PLAN4, dict(side=True)),
    ("2ph_3d_6x5x4_M2", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), _four_wells, PLAN4, dict(satfn=M2)),
    ("2ph_3d_5x6x4_M2_graded", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4, nphase=2), _four_wells, PLAN4, dict(satfn=M2, graded=True)),
    ("2ph_3d_6x5x4_M2_graded_open_side", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=4, nphase=2), _four_wells, PLAN4,
     dict(satfn=M2, graded=True, side=True)),
]
_CACHE = {}


def _case(pid):
    """spec (with tuned wells), state, the reference problem with its R, J, S~ and well states: computed once per case."""
    if pid in _CACHE:
        return _CACHE[pid]
    _, builder, kw, wells_fn, plan, extra = next(e for e in ENTRY if e[0] == pid)
    spec, *_ = builder(**kw)
    u = cases.perturbed_state(spec, seed=3)
    if extra.get("graded"):
        spec["hs"] = _graded(spec)
    if extra.get("side"):
        spec["boundary"] = _open_side(spec, u)
    if extra.get("satfn"):
        from thermalporous_amd.physicalparameters import check_satfn
        spec["satfn"] = check_satfn(dict(extra["satfn"]))
        u[2] = np.clip(u[2], 0.25, 0.8)                 # inside the mobile range of M2
    wells = wells_fn(spec, spec.get("hs"))
    P = wells_problem(spec, wells=wells)
    P.set_dt(DT)
    spec["wells"] = tune_wells(P, u, wells, plan)
    R = P.residual(u)
    J, Sm = P.jacobian(u, want_schur=True)
    st = P.well_state(u)
    _CACHE[pid] = (spec, u, P, R, J, Sm, st)
    return _CACHE[pid]


def _engine(spec, u, opts=None, dt=DT):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts or _opts(spec["nphase"]))
    h.set_old(u)
    h.set_dt(dt)
    h.set_state(u)
    return h


def _assert_states(P, u, st, info):
    """What the issue asks of the states, on the reference and (rounds) on the kernel."""
    modes = [s["mode"] for s in st]
    assert "rate" in modes and "bhp" in modes, modes
    assert any(not s["open"].all() for s in st), "no closed perforation"
    assert any(s["open"].any() and not s["open"].all() for s in st)
    assert {w["kind"] for w in P.wells} == {"prod", "inj"}
    assert max(i["rounds"] for i in info) >= 2 and max(s["rounds"] for s in st) >= 2
    assert P.kink_margin(u) > 1e-3, P.kink_margin(u)


@pytest.mark.parametrize("pid", [e[0] for e in ENTRY])
def test_well_entries_against_the_reference(pid):
    spec, u, P, Ro, Jo, So, st = _case(pid)
    h = _engine(spec, u)
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    info = h.well_info()
    _assert_states(P, u, st, info)
    # the wells are visible in what is compared: without them the residual at their cells is another one
    bare = wells_problem(dict(spec, wells=[]), wells=[])
    bare.set_old(u)
    bare.set_dt(DT)
    R0 = bare.residual(u)
    cells = np.concatenate([w["cells"] for w in P.wells])
    for f in range(P.b):
        d = np.abs((Ro[f] - R0[f]).reshape(-1)[cells])
        print("%s field %d: wells' part of R up to %.3e, R up to %.3e" % (pid, f, d.max(), np.abs(Ro[f]).max()))
    assert np.abs((Ro[0] - R0[0]).reshape(-1)[cells]).max() > 1e-6*np.abs(Ro[0]).max()
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    # the same rule on the wells' own cells, whose scale is theirs and not the whole grid's
    for f in range(P.b):
        a, b = Rh[f].reshape(-1)[cells], Ro[f].reshape(-1)[cells]
        assert np.abs(a - b).max() < TOL*np.abs(b).max(), (pid, "residual at the wells, field", f)
        for c in range(P.b):
            a, b = Jh[0, f, c].reshape(-1)[cells], Jo[0, f, c].reshape(-1)[cells]
            assert np.abs(a - b).max() <= TOL*np.abs(b).max(), (pid, "diagonal block at the wells", f, c)
    # factors, bhp, mode, rates
    fac = h.well_factors()
    cref = np.concatenate([c for c, _ in P.last_factors], axis=1)
    bref = np.concatenate([b for _, b in P.last_factors], axis=1)
    cgpu = np.concatenate([c for c, _ in fac], axis=1)
    bgpu = np.concatenate([b for _, b in fac], axis=1)
    assert np.abs(cref).max() > 0.0 and np.abs(bref).max() > 0.0
    for r in range(P.b):
        assert np.abs(cgpu[r] - cref[r]).max() < TOL*np.abs(cref[r]).max(), (pid, "factor c", r)
        if np.abs(bref[r]).max() == 0.0:
            assert np.all(bgpu[r] == 0.0)
        else:
            assert np.abs(bgpu[r] - bref[r]).max() < TOL*np.abs(bref[r]).max(), (pid, "factor b", r)
    rates = h.well_perf_rates()
    for w, s, i, q in zip(P.wells, st, info, rates):
        assert i["mode"] == s["mode"] and i["nopen"] == int(s["open"].sum()) and i["rounds"] == s["rounds"], (w["name"], i, s["mode"])
        assert abs(i["bhp"] - s["bhp"]) < 1e-12*abs(s["bhp"])
        assert np.array_equal(q["rate"] != 0.0, s["open"] & (np.real(s["a"]) > 0.0))
        assert np.abs(q["rate"] - s["q"]).max() < TOL*np.abs(s["q"]).max()
        assert np.abs(q["water_rate"] - s["qw"]).max() <= TOL*np.abs(s["q"]).max()
        assert np.abs(q["oil_rate"] - s["qo"]).max() <= TOL*np.abs(s["q"]).max()
        if s["mode"] == "bhp":
            assert i["bhp"] == w["bhp"]                                   # bitwise the limit
        else:
            Q = -w["rate"] if w["kind"] == "prod" else w["rate"]
            assert abs(q["rate"].sum() - Q) < 1e-12*w["rate"] and abs(i["rate"] - Q) < 1e-12*w["rate"]
    h.close()


# ---- the Krylov operator -----------------------------------------------------------------------------------------------------
def _operator_case():
    spec, u, P, Ro, Jo, So, st = _case("2ph_3d_6x5x4")
    return spec, u, P, Jo, st


def _full_op(P, J, x):
    from oracle import linalg as la
    return la.spmv_block(J, x) + P.rank1(x)


def test_spmv_applies_the_rank1_terms():
    from oracle import linalg as la
    spec, u, P, Jo, st = _operator_case()
    h = _engine(spec, u)
    h.jacobian()
    rows = np.concatenate([w["cells"] for w, s in zip(P.wells, st) if s["mode"] == "rate"])
    for seed in (1, 2, 3):
        x = np.random.default_rng(seed).standard_normal(u.shape)
        h.vec_set("x", x)
        h.spmv("x", "y")
        y = h.vec_get("y")
        ref = _full_op(P, Jo, x)
        assert np.abs(y - ref).max() < 1e-12*np.abs(ref).max()
        y7 = la.spmv_block(Jo, x)
        d = (y - y7).reshape(P.b, -1)[:, rows]
        assert np.linalg.norm(d) > 1e-3*np.linalg.norm(y7.reshape(P.b, -1)[:, rows])
    h.close()


@pytest.mark.parametrize("name,opts", [("fgmres", {}), ("bcgs", dict(ksp="bcgs")), ("fgmres_basis_single", dict(ksp_basis_single=True)),
                                       ("fgmres_monitor", dict(monitor=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_krylov_solves_the_full_operator(name, opts):
    """The right-hand side is the Newton one, the residual at the state.  (A random vector is none the fp32 basis is made for: on
    this box, whose equations' scales lie eight orders apart, tp_fgmres with ksp_basis_single stalls at 1e-3 ||b|| on a standard
    normal b with or without wells -- measured on the engine without wells, so it is no property of theirs.)"""
    spec, u, P, Jo, st = _operator_case()
    opts = dict(opts)
    monitor = opts.pop("monitor", False)
    rtol = 1e-8
    h = _engine(spec, u, dict(_opts(2), ksp_rtol=rtol, **opts))
    h.jacobian(want_schur=True)
    h.pc_setup()
    seen = []
    if monitor:
        h.set_ksp_monitor(lambda its, rn, fn: seen.append((its, rn, list(fn))))
    b = _case("2ph_3d_6x5x4")[3].copy()
    h.vec_set("b", b)
    its, reason, rn = (h.bcgs if name == "bcgs" else h.fgmres)("b", "x")
    x = h.vec_get("x")
    assert reason == 2 and its > 0
    bn = np.linalg.norm(b)
    full = np.linalg.norm(b - _full_op(P, Jo, x))
    from oracle import linalg as la
    seven = np.linalg.norm(b - la.spmv_block(Jo, x))
    print("%s: %d iterations, ||b - A x|| / ||b|| = %.3e with the wells' terms, %.3e without" % (name, its, full/bn, seven/bn))
    # the solver's tolerance, plus the rounding of the reference's own product
    assert full <= 1.05*rtol*bn + 1e-13*np.abs(Jo).max()*np.linalg.norm(x)/np.sqrt(x.size)
    assert seven > 100.0*rtol*bn                     # the 7-point operator alone is not what was solved
    if monitor:
        # the monitor's per-field norms are those of the full operator's true residual at the last iterate
        assert len(seen) == its
        r = (b - _full_op(P, Jo, x)).reshape(P.b, -1)
        for f in range(P.b):
            assert abs(seen[-1][2][f] - np.linalg.norm(r[f])) <= 1e-6*np.linalg.norm(r[f]) + 1e-12*bn
    h.close()


# ---- properties --------------------------------------------------------------------------------------------------------------
def _bits(h):
    R = h.residual()
    J, Sm = h.jacobian(want_schur=True)
    return R.tobytes(), J.tobytes(), Sm.tobytes()


def test_shut_and_removed_wells_give_the_no_well_bits():
    spec, u, P, *_ = _case("2ph_3d_6x5x4")
    bare = dict(spec)
    del bare["wells"]
    a, b = _engine(bare, u), _engine(spec, u)
    plain = _bits(a)
    with_wells = _bits(b)
    assert all(x != y for x, y in zip(with_wells, plain))
    for i in range(len(spec["wells"])):
        b.set_well_control(i, shut=True)
    assert _bits(b) == plain
    assert all(w["mode"] == "shut" and w["rate"] == 0.0 for w in b.well_info())
    assert all(np.all(c == 0.0) and np.all(bb == 0.0) for c, bb in b.well_factors())
    for i in range(len(spec["wells"])):
        b.set_well_control(i, shut=False, rate=0.0)
    assert _bits(b) == plain
    for i, w in enumerate(spec["wells"]):
        b.set_well_control(i, rate=w["rate"])
    assert _bits(b) == with_wells
    b.set_wells(None)
    assert _bits(b) == plain and b.well_info() == []
    # and the operator without wells is the 7-point product
    x = np.random.default_rng(1).standard_normal(u.shape)
    ys = []
    for h in (a, b):
        h.vec_set("x", x)
        h.spmv("x", "y")
        ys.append(h.vec_get("y").tobytes())
    assert ys[0] == ys[1]
    a.close()
    b.close()


@pytest.mark.parametrize("nphase", [1, 2])
@pytest.mark.parametrize("kind", ["prod", "inj"])
def test_one_perforation_reproduces_the_legacy_entry(nphase, kind):
    """A one-perforation well with no head against the tp_source entry with the same WI and wt = 1: in BHP mode the Peaceman entry,
    in rate mode the constant_rate entry; R, J and S~ to 1e-13 of the entry's own contribution scale, factors zero."""
    spec, *_ = cases.c4_spe10_3d(Nx=4, Ny=3, Nz=3, nphase=nphase)
    u = cases.perturbed_state(spec, seed=5)
    n = spec["n"]
    cell = 1 + n[0]*(1 + n[1]*1)
    pc = float(u[0].reshape(-1)[cell])
    WI = float(make_well(spec, "w", kind, [cell], 0, 1.0, 1.0)["WI"][0])
    sg = -1.0 if kind == "prod" else 1.0
    bare = dict(spec, sources=None)
    h0 = _engine(bare, u)
    base = (h0.residual(),) + h0.jacobian(want_schur=True)
    h0.close()
    for mode in ("bhp", "rate"):
        bhp = pc + sg*0.7                                  # the legacy drawdown
        if mode == "bhp":
            # Peaceman entry, never capped; the well: a rate target it cannot reach, so the limit rules
            src = dict(cell=[cell], kind=[0 if kind == "prod" else 1], wt=[1.0], bhp=[bhp], max_rate=[sg*1e30], WI=[WI], const=[0])
            well = dict(name="w", kind=kind, rate=1e30, bhp=bhp, cells=[cell], WI=[WI], z=[0.0])
        else:
            Q = 0.3*WI*1e3
            src = dict(cell=[cell], kind=[0 if kind == "prod" else 1], wt=[1.0], bhp=[bhp], max_rate=[sg*Q], WI=[WI], const=[1])
            well = dict(name="w", kind=kind, rate=Q, bhp=pc + sg*1e6, cells=[cell], WI=[WI], z=[0.0])
        src = {k: np.asarray(v) for k, v in src.items()}
        hl = _engine(dict(bare, sources=src), u)
        hw = _engine(dict(bare, wells=[well]), u)
        legacy = (hl.residual(),) + hl.jacobian(want_schur=True)
        mine = (hw.residual(),) + hw.jacobian(want_schur=True)
        info = hw.well_info()[0]
        assert info["mode"] == mode, info
        (cf, bf), = hw.well_factors()
        assert np.all(cf == 0.0) and np.all(bf == 0.0)
        for name, L, M, B0 in zip(("R", "J", "S~"), legacy, mine, base):
            dl, dm = L - B0, M - B0                                     # what the entry / the well added
            if name == "S~" and kind == "inj":
                assert np.all(dl == 0.0) and np.all(dm == 0.0)
                continue
            assert np.abs(dl).max() > 0.0
            print("%dph %s %s %s: largest difference %.3e of %.3e" % (nphase, kind, mode, name, np.abs(M - L).max(), np.abs(dl).max()))
            where = np.abs(dl) > 0.0                                    # the entries the legacy entry touches
            assert np.array_equal(M[~where], L[~where])
            assert np.abs(M - L)[where].max() <= 1e-13*np.abs(L[where]).max()
        hl.close()
        hw.close()


def test_head_follows_the_old_state_and_stays_frozen_within_the_step():
    """A two-perforation producer in a 1 x 1 x 5 column: rho_w is the mobility-weighted density of the OLD state; another current
    state changes the rates but not rho_w; another old state changes it."""
    spec, *_ = cases.c4_spe10_3d(Nx=1, Ny=1, Nz=5, nphase=2, homogeneous=True)     # (equal WI: both perforations carry flow)
    spec = dict(spec, sources=None)
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (5, 1, 1)
    u_old = cases.perturbed_state(spec, seed=2, amp=0.2)
    u_new = cases.perturbed_state(spec, seed=9, amp=0.2)
    well = make_well(spec, "P", "prod", [1, 3], 0, 1.0, 1.0)
    P = wells_problem(spec, wells=[well])
    P.set_dt(DT)
    spec["wells"] = tune_wells(P, u_old, [well], {"P": ("rate", 5.0)})
    P.set_old(u_old)
    rho_old = P.rho_w[0]
    head = rho_old*spec["prm"]["g"]*(well["z"][1] - well["z"][0])
    assert head > 1e-3                                    # MPa: the two perforations are two layers apart
    h = _engine(spec, u_old)
    for state in (u_old, u_new):
        Ro = P.residual(state)
        Jo, So = P.jacobian(state, want_schur=True)
        Rh = h.residual(state)
        Jh, Sh = h.jacobian(want_schur=True)
        assert_entries(Rh, Jh, Sh, Ro, Jo, So, "column")
        i, s = h.well_info()[0], P.well_state(state)[0]
        assert abs(i["rho"] - rho_old) < 1e-13*rho_old and i["mode"] == s["mode"] == "rate" and s["open"].all()
        assert abs(i["bhp"] - s["bhp"]) < 1e-12*abs(s["bhp"])
        q = h.well_perf_rates()[0]["rate"]
        assert np.abs(q - s["q"]).max() < TOL*np.abs(s["q"]).max()
        # the head is in the rates: without it the split between the two perforations is another one
        a, th0 = np.real(s["a"]), state[0].reshape(-1)[[1, 3]]
        q0 = -a*(th0 - (np.sum(a*th0) - spec["wells"][0]["rate"])/a.sum())
        assert np.abs(q0 - s["q"]).max() > 1e-3*np.abs(s["q"]).max()
    h.set_old(u_new)
    P.set_old(u_new)
    assert abs(P.rho_w[0] - rho_old) > 1e-6*rho_old
    h.residual(u_new)
    assert abs(h.well_info()[0]["rho"] - P.rho_w[0]) < 1e-13*rho_old
    h.close()


# ---- Newton and the time loop ------------------------------------------------------------------------------------------------
C4 = dict(Nx=7, Ny=13, Nz=9)
NEWTON = [
    ("cptr", 2, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25), 86.4),
    ("cpr", 2, dict(pc="cpr", ksp_rtol=1e-8, snes_max_it=25), 86.4),
    ("1ph_fieldsplit_cd", 1, dict(pc="fieldsplit_cd", ksp_rtol=1e-8), 864.0),
    ("cptr_bt", 2, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, linesearch="bt"), 86.4),
    ("cptr_bcgs", 2, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, ksp="bcgs"), 86.4),
]


def _newton_problem(nphase):
    """c4 7x13x9 with its own wells and heaters, plus a rate-controlled producer over all nine layers, an injector over six that
    sits at its BHP limit, and a horizontal producer."""
    spec, u0, p, *_ = cases.c4_spe10_3d(nphase=nphase, **C4)
    assert spec["gaxis"] == 0
    wells = [make_well(spec, "P", "prod", line_cells(spec, 0, (2, 3)), 0, 1.0, 1.0),
             make_well(spec, "I", "inj", line_cells(spec, 0, (5, 9), 2, 8), 0, 1.0, 1.0),
             make_well(spec, "H", "prod", line_cells(spec, 2, (4, 1), 5, 10), 2, 1.0, 1.0)]
    P = wells_problem(spec, wells=wells)
    spec["wells"] = tune_wells(P, u0, wells, {"P": ("rate", 1.5), "I": ("bhp", 2.0), "H": ("rate", 1.0)})
    return spec, u0


def _two_steps(spec, u0, opts, dt, between=None):
    from thermalporous_amd.engine import HipEngine
    o, h = wells_oracle(spec, opts), HipEngine(spec, opts)
    for e in (o, h):
        e.set_state(u0)
    modes = []
    for step in range(2):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(dt)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("step %d: oracle nits %d lits %d, engine nits %d lits %d" % (step, ro["nits"], ro["lits"], rh["nits"], rh["lits"]))
        _assert_step(ro, rh, o, h)
        io, ih = o.well_info(), h.well_info()
        for a, b in zip(io, ih):
            assert a["mode"] == b["mode"] and abs(np.real(a["bhp"]) - b["bhp"]) < 1e-7*abs(b["bhp"]), (a["mode"], b)
        modes.append([b["mode"] for b in ih])
        if step == 0 and between is not None:
            between(o, h)
    h.close()
    return modes, ih


@pytest.mark.parametrize("name,nphase,opts,dt", NEWTON, ids=[c[0] for c in NEWTON])
def test_newton_parity_with_wells(name, nphase, opts, dt):
    spec, u0 = _newton_problem(nphase)
    modes, info = _two_steps(spec, u0, opts, dt)
    assert "rate" in modes[-1]
    for w, i in zip(spec["wells"], info):
        if i["mode"] == "rate":
            Q = -w["rate"] if w["kind"] == "prod" else w["rate"]
            assert abs(i["rate"] - Q) < 1e-12*w["rate"]


def test_well_control_changes_between_steps():
    """The producer's rate target is halved after step 1; step 2 matches the oracle given the same change."""
    spec, u0 = _newton_problem(2)
    name, nphase, opts, dt = NEWTON[0]
    Q = spec["wells"][0]["rate"]
    seen = []

    def between(o, h):
        seen.append(h.well_info()[0]["rate"])
        h.set_well_control("P", rate=0.5*Q)
        o.set_well_control(0, rate=0.5*Q)
    modes, info = _two_steps(spec, u0, opts, dt, between=between)
    assert modes[0][0] == modes[1][0] == "rate"
    assert abs(seen[0] + Q) < 1e-12*Q and abs(info[0]["rate"] + 0.5*Q) < 1e-12*Q


def _depletion_problem():
    """A closed homogeneous box, no other source, one producer over all layers at a rate that the box cannot sustain."""
    spec, u0, p, *_ = cases.c4_spe10_3d(Nx=4, Ny=4, Nz=6, nphase=2, homogeneous=True)
    spec = dict(spec, sources=None)
    well = make_well(spec, "P", "prod", line_cells(spec, 0, (1, 2)), 0, 1.0, 1.0)
    P = wells_problem(spec, wells=[well])
    P.set_old(u0)
    a = np.real(P.well_state(u0)[0]["a"])
    drop = 1.5                                           # MPa between the initial pressure and the limit
    well = dict(well, rate=float(0.4*a.sum()), bhp=float(u0[0].mean() - drop))      # the rate needs a drawdown of 0.4 MPa
    spec["wells"] = [well]
    return spec, u0, drop


def test_closed_box_depletes_from_rate_to_bhp_control():
    from thermalporous_amd.engine import HipEngine
    spec, u0, drop = _depletion_problem()
    Q = spec["wells"][0]["rate"]
    h = HipEngine(spec, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25))
    h.set_state(u0)
    # the time step: the box's pore volume times an upper bound of its compressibility (1e-3 / MPa) would give up `drop` in about eighteen
    # steps at the full rate
    pore = float(np.sum(spec["phi"])*np.prod(spec["h"]))
    dt = 1e-3*pore*drop/(18.0*Q)
    modes, rates, pbar = [], [], []
    for step in range(14):
        h.set_old(None)
        h.set_dt(dt)
        r = h.newton_solve()
        assert r["reason"] > 0, r
        i = h.well_info()[0]
        modes.append(i["mode"])
        rates.append(i["rate"])
        pbar.append(float(h.get_state()[0].mean()))
    h.close()
    print("modes", modes, "rates/Q", [round(q/Q, 4) for q in rates], "mean p", [round(v, 3) for v in pbar])
    assert modes[0] == "rate" and modes[-1] == "bhp"
    first = modes.index("bhp")
    assert all(m == "rate" for m in modes[:first]) and all(m == "bhp" for m in modes[first:])      # it never goes back
    assert all(abs(q + Q) < 1e-12*Q for q in rates[:first])
    assert all(-Q*(1.0 + 1e-12) <= q <= 0.0 for q in rates)                                          # never more than the target
    assert all(b < a for a, b in zip(pbar, pbar[1:]))                                                # it depletes
    assert rates[-1] > rates[first] - 1e-15                                                          # and the rate declines


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library():
    from thermalporous_amd.engine import EngineError, HipEngine, tp_perf, tp_well
    spec, u, P, *_ = _case("2ph_3d_6x5x4")
    bare = dict(spec)
    del bare["wells"]
    h = _engine(bare, u)
    base = _bits(h)
    np_ = h.np_
    cell = int(spec["wells"][0]["cells"][0]) + np_

    def call(wells, perfs):
        wa, pa = (tp_well*len(wells))(*wells), (tp_perf*len(perfs))(*perfs)
        return h.lib.tp_set_wells(h.ctx, len(wells), wa, len(perfs), pa)

    def err():
        return h.lib.tp_last_error().decode()
    ok_w, ok_p = tp_well(0, 0, 1.0, 1.0, 0.0, 0, 1), tp_perf(cell, 1.0, 0.0)
    for wells, perfs, msg in (
            ([tp_well(0, 0, -1.0, 1.0, 0.0, 0, 1)], [ok_p], "well 0: rate = -1"),
            ([tp_well(0, 0, float("nan"), 1.0, 0.0, 0, 1)], [ok_p], "well 0: rate, bhp_limit and z_ref must be finite"),
            ([tp_well(2, 0, 1.0, 1.0, 0.0, 0, 1)], [ok_p], "well 0: kind = 2"),
            ([ok_w], [tp_perf(cell, 0.0, 0.0)], "well 0, perforation 0: WI = 0"),
            ([ok_w], [tp_perf(cell, float("inf"), 0.0)], "well 0, perforation 0: WI and z must be finite"),
            ([ok_w], [tp_perf(3, 1.0, 0.0)], "well 0, perforation 0: cell 3 lies outside the box"),
            ([ok_w], [tp_perf(h.ntot - 1, 1.0, 0.0)], "lies outside the box"),
            ([tp_well(0, 0, 1.0, 1.0, 0.0, 0, 2)], [ok_p], "outside the array of 1"),
            ([ok_w, tp_well(1, 0, 1.0, 1.0, 0.0, 1, 1)], [ok_p, ok_p], "well 1, perforation 0: cell %d is already perforated by well 0" % cell),
            ([tp_well(0, 0, 1.0, 1.0, 0.0, 0, 2)], [ok_p, ok_p], "well 0, perforation 1: cell %d is already perforated by well 0" % cell)):
        assert call(wells, perfs) != 0 and msg in err(), (msg, err())
    assert h.lib.tp_set_well_control(h.ctx, 0, C.c_double(1.0), C.c_double(1.0), 0) != 0 and "the context has 0 wells" in err()
    assert _bits(h) == base                                   # a refused call leaves the context as it was
    with pytest.raises(ValueError, match="already perforated by well 'P'"):
        h.set_wells([spec["wells"][0], dict(spec["wells"][1], cells=spec["wells"][0]["cells"][:spec["wells"][1]["cells"].size])])
    h.close()


def test_two_slabs_are_refused():
    from thermalporous_amd.engine import HipEngine, load_library, tp_perf, tp_well
    spec, u, *_ = _case("2ph_3d_6x5x4")
    lib = load_library()
    grp = C.c_void_p()
    assert lib.tp_local_group_create(2, C.byref(grp)) == 0
    try:
        with pytest.raises(NotImplementedError, match="nranks = 2"):
            HipEngine(spec, _opts(2), rank=0, nranks=2, local_group=grp)
        # and the library itself: a context of a two-slab grid refuses tp_set_wells whatever the host checked
        bare = dict(spec)
        del bare["wells"]
        out = {}

        def make(rank):
            out[rank] = HipEngine(bare, _opts(2), rank=rank, nranks=2, local_group=grp)
        ts = [threading.Thread(target=make, args=(r,)) for r in range(2)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        h = out[0]
        wa, pa = (tp_well*1)(tp_well(0, 0, 1.0, 1.0, 0.0, 0, 1)), (tp_perf*1)(tp_perf(h.np_, 1.0, 0.0))
        assert lib.tp_set_wells(h.ctx, 1, wa, 1, pa) != 0
        assert "nranks = 2" in lib.tp_last_error().decode()
        for e in out.values():
            e.close()
    finally:
        lib.tp_local_group_destroy(grp)
