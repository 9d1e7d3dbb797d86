"""amg_gs_levels / amg_gs_sweeps (red-black Gauss-Seidel on the top levels of the scalar AMG cycle) on the host: the tests'
reference (amg_gs_ref.GsSemiAMG) is the Gauss-Seidel sweep (D + L)^-1 in red-then-black ordering with the operator assembled
densely, and is SemiAMG bit for bit when off; the keys are accepted and off by default; what they exclude is refused naming both
options; the C struct carries the fields where the header says and the header declares the new query; the FGMRES counts of the
reference keep the conditions DESIGN.md 4.5 states.  No GPU."""
import os
import re

import numpy as np
import pytest

import cases
import oracle.linalg as la
from amg_gs_ref import GsSemiAMG, oracle_engine, red_mask
from oracle.engine import OracleEngine
from oracle.linalg import SemiAMG, spmv_scalar
from thermalporous_amd.engine import API_SYMBOLS, DEFAULT_OPTS, EngineError, HipEngine, check_amg_gs_options, \
    resolve_ilu_options, tp_options
from thermalporous_amd.homogeneousgeo import HomogeneousGeo
from thermalporous_amd.physicalparameters import PhysicalParameters
from thermalporous_amd.solver_options import _flatten, engine_options
from thermalporous_amd.twophase import TwoPhase
from thermalporous_amd.wellcase import WellCase

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "thermalporous_hip.h")
KEYS = ("amg_gs_levels", "amg_gs_sweeps")


def operator(n, seed=0):
    """A diagonally dominant 7-point operator on the box n = (n0, n1, n2) with zero couplings across the boundary."""
    n0, n1, n2 = n
    rng = np.random.default_rng(seed)
    A = np.zeros((7, n2, n1, n0))
    A[1:] = -rng.uniform(0.1, 1.0, (6, n2, n1, n0))*np.array([30.0, 30.0, 1.0, 1.0, 3.0, 3.0])[:, None, None, None]
    A[1][..., 0] = A[2][..., -1] = 0.0
    A[3][:, 0] = A[4][:, -1] = 0.0
    A[5][0] = A[6][-1] = 0.0
    A[0] = -A[1:].sum(axis=0) + rng.uniform(0.01, 0.1, (n2, n1, n0))
    return A


def dense(A):
    """The operator as a dense matrix over the flattened cells, column by column from the stencil mat-vec."""
    shape = A[0].shape
    n = A[0].size
    M = np.zeros((n, n))
    for c in range(n):
        e = np.zeros(n)
        e[c] = 1.0
        M[:, c] = spmv_scalar(A, e.reshape(shape)).reshape(-1)
    return M


def small_amg(n, A):
    """GsSemiAMG on a box far below the tail threshold, with level 0 made a GS level by hand (the sweeps do not depend on size)."""
    amg = GsSemiAMG(n, (30.0, 1.0, 3.0), gs_levels=1, gs_sweeps=1, omega=0.9, nu=2, full_levels=3).setup(A)
    assert not amg.is_gs(0)                            # (the level rule keeps such a box in the tail)
    return amg


@pytest.mark.parametrize("n", [(5, 4, 3), (1, 7, 6), (4, 1, 3)], ids=str)
def test_reference_sweep_is_the_dense_gauss_seidel_in_red_black_order(n):
    A = operator(n)
    amg = small_amg(n, A)
    rng = np.random.default_rng(1)
    b, x = rng.standard_normal(A[0].shape), rng.standard_normal(A[0].shape)
    red = red_mask(A[0].shape).reshape(-1)
    order = np.concatenate([np.flatnonzero(red), np.flatnonzero(~red)])          # red cells first, then black
    M = dense(A)[np.ix_(order, order)]
    DL = np.tril(M)
    want = np.empty(A[0].size)
    want[order] = x.reshape(-1)[order] + np.linalg.solve(DL, b.reshape(-1)[order] - M @ x.reshape(-1)[order])
    got = amg.forward(0, b, x)
    assert np.linalg.norm(got.reshape(-1) - want)/np.linalg.norm(want) <= 1e-12
    # cells of one colour do not couple: the red-red and black-black blocks of the operator are diagonal
    nr = int(red.sum())
    assert np.count_nonzero(M[:nr, :nr] - np.diag(np.diag(M[:nr, :nr]))) == 0
    assert np.count_nonzero(M[nr:, nr:] - np.diag(np.diag(M[nr:, nr:]))) == 0
    # after the red half-sweep the residual at the red cells is zero to rounding, and the black cells are untouched
    xr = amg.half(0, 0, b, x)
    r = (b - spmv_scalar(A, xr)).reshape(-1)
    scale = np.abs(dense(A)) @ np.abs(xr.reshape(-1)) + np.abs(b.reshape(-1))
    assert np.all(np.abs(r[red]) <= 1e-13*scale[red])
    assert np.array_equal(xr.reshape(-1)[~red], x.reshape(-1)[~red])
    # the backward sweep is the same with the colours exchanged
    xb = amg.half(0, 1, b, x)
    assert np.array_equal(amg.backward(0, b, x), amg.half(0, 0, b, xb))
    assert np.array_equal(xb.reshape(-1)[red], x.reshape(-1)[red])


def test_colour_is_the_index_sum_not_the_linear_index():
    m = red_mask((3, 3, 5))                            # n0 = 5, n0 n1 = 15: both odd
    assert m[0, 0, 0] and not m[0, 0, 1] and not m[0, 1, 0] and not m[1, 0, 0] and m[1, 1, 0]
    lin = (np.arange(m.size) % 2 == 0).reshape(m.shape)
    assert np.array_equal(m, lin)                      # every extent odd: the two agree ...
    m = red_mask((3, 4, 6))
    lin = (np.arange(m.size) % 2 == 0).reshape(m.shape)
    assert not np.array_equal(m, lin)                  # ... an even n0 and they do not
    assert m.sum() == m.size//2


def test_rule_tail_levels_are_never_gs():
    A = operator((9, 14, 8))                           # 1008 cells: wholly inside the tail
    amg = GsSemiAMG((9, 14, 8), (30.0, 1.0, 3.0), gs_levels=3, full_levels=3).setup(A)
    assert amg.n_gs_levels() == 0
    b = np.random.default_rng(2).standard_normal(A[0].shape)
    assert np.array_equal(amg.vcycle(b), SemiAMG.vcycle(amg, b))
    A = operator((10, 22, 12))                         # 2640 / 1320 / 660: two levels above the tail
    amg = GsSemiAMG((10, 22, 12), (30.0, 1.0, 3.0), gs_levels=3, full_levels=3).setup(A)
    assert [amg.is_gs(l) for l in range(4)] == [True, True, False, False]
    sizes = [l[0].size for l in amg.levels[:3]]
    assert sizes[:2] == [2640, 1320] and sizes[2] <= 1024
    amg.gs_levels = 1
    assert amg.n_gs_levels() == 1
    amg = GsSemiAMG((1, 40, 33), (0.0, 1.0, 3.0), gs_levels=1, full_levels=3).setup(operator((1, 40, 33)))
    assert amg.n_gs_levels() == 1                      # (no n0 >= 2 clause, unlike the line levels)


def set_up(e, spec, u0, u, pc):
    e.set_old(u0)
    e.set_dt(8640.0)
    e.set_state(u)
    out = e.jacobian(want_schur=pc == "cptr")
    J, Sm = out if pc == "cptr" else (out, None)
    e.pc.setup(J, Sm)
    return J


@pytest.mark.parametrize("pc", ["cpr", "cptr"])
def test_off_is_semiamg_bit_for_bit(pc):
    spec, u0, *_ = cases.c4_spe10_3d(Nx=12, Ny=22, Nz=10, nphase=2)
    opts = dict(pc=pc)
    engs = [OracleEngine(spec, opts), oracle_engine(spec, dict(opts, amg_gs_levels=0)), oracle_engine(spec, dict(opts, amg_gs_levels=2))]
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    x = np.random.default_rng(3).standard_normal(u.shape)
    ys = []
    for e in engs:
        set_up(e, spec, u0, u, pc)
        ys.append(e.pc.apply(x))
    assert isinstance(engs[1].pc.amg_p, GsSemiAMG) and engs[1].pc.amg_p.n_gs_levels() == 0
    assert np.array_equal(ys[0], ys[1])
    assert engs[2].pc.amg_p.n_gs_levels() == 2 and not np.array_equal(ys[0], ys[2])


# The reference's FGMRES counts (cptr, dt 8640, perturbed_state(seed=5, amp=0.3), rhs default_rng(13), default options), as
# conditions: one Gauss-Seidel sweep per leg streams about the bytes of the two Jacobi sweeps it replaces and must not cost more
# than two iterations; two sweeps per leg must buy iterations.  Measured: 12x22x10  19 / 20 / 16,  13x21x11  24 / 25 / 21.
@pytest.fixture(scope="module", params=[(12, 22, 10), (13, 21, 11)], ids=str)
def counts(request):
    Nx, Ny, Nz = request.param
    spec, u0, *_ = cases.c4_spe10_3d(Nx=Nx, Ny=Ny, Nz=Nz, nphase=2)
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    b = np.random.default_rng(13).standard_normal(u.shape)
    its = {}
    for key, extra in (("off", {}), ("g1", dict(amg_gs_levels=3)), ("g2", dict(amg_gs_levels=3, amg_gs_sweeps=2))):
        o = oracle_engine(spec, dict(pc="cptr", **extra))
        J = set_up(o, spec, u0, u, "cptr")
        _, it, reason, _ = la.fgmres(lambda v: la.spmv_block(J, v), o.pc.apply, b, rtol=o.opts["ksp_rtol"], atol=o.opts["ksp_atol"],
                                     restart=o.opts["ksp_restart"], maxit=o.opts["ksp_max_it"])
        assert reason > 0, (key, it, reason)
        assert o.pc.amg_p.n_gs_levels() == (0 if key == "off" else 2)          # (level 2 is the tail: L = 3 gives two GS levels)
        its[key] = it
    print("%dx%dx%d: FGMRES iterations off %d, L=3 g=1 %d, L=3 g=2 %d" % (Nx, Ny, Nz, its["off"], its["g1"], its["g2"]))
    return its


def test_counts_one_sweep_costs_at_most_two_iterations(counts):
    assert counts["g1"] <= counts["off"] + 2, counts


def test_counts_two_sweeps_need_strictly_fewer_iterations(counts):
    assert counts["g2"] < counts["off"], counts


def preset(name):
    p = PhysicalParameters()
    p.S_o = 0.9
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    c = WellCase(p, g, well_case="test0", constant_rate=True)
    m = TwoPhase(g, c, p, solver_parameters=name, filename=None, verbosity=False, _engine_factory=OracleEngine)
    return _flatten(dict(m.solver_parameters)), m.name, m.decoup


def test_keys_are_accepted_and_off_by_default():
    sp, model, decoup = preset("pc_cptr")
    assert DEFAULT_OPTS["amg_gs_levels"] == 0 and DEFAULT_OPTS["amg_gs_sweeps"] == 1
    off = engine_options(sp, model, decoup)
    assert off["amg_gs_levels"] == 0 and off["amg_gs_sweeps"] == 1
    on = engine_options({**sp, "amg_gs_levels": 2, "amg_gs_sweeps": 3}, model, decoup)
    assert on["amg_gs_levels"] == 2 and on["amg_gs_sweeps"] == 3
    assert {k: v for k, v in on.items() if k not in KEYS} == {k: v for k, v in off.items() if k not in KEYS}
    o = HipEngine._make_options(resolve_ilu_options(dict(DEFAULT_OPTS, amg_gs_levels=2, amg_gs_sweeps=3), (8, 9, 14)))
    assert (o.amg_gs_levels, o.amg_gs_sweeps) == (2, 3)
    o = HipEngine._make_options(resolve_ilu_options(dict(DEFAULT_OPTS), (8, 9, 14)))
    assert (o.amg_gs_levels, o.amg_gs_sweeps) == (0, 1)


def test_struct_fields_and_export_exist():
    names = [f[0] for f in tp_options._fields_]
    i = names.index("ilu_whole")
    assert names[i:i + 4] == ["ilu_whole", "amg_gs_levels", "amg_gs_sweeps", "ilu_block"]
    assert "tp_amg_gs_info" in API_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"int32_t\s+amg_gs_levels\s*;", text) and re.search(r"int32_t\s+amg_gs_sweeps\s*;", text)
    order = [text.index(s) for s in ("int32_t ilu_whole;", "int32_t amg_gs_levels;", "int32_t amg_gs_sweeps;", "int32_t ilu_block[3];")]
    assert order == sorted(order)
    assert re.search(r"int\s+tp_amg_gs_info\s*\(\s*tp_ctx\s*\*\s*ctx\s*,\s*int32_t\s+which\s*,\s*int64_t\s+out\[4\]\s*\)\s*;", text)


def test_ranges_are_value_errors():
    sp, model, decoup = preset("pc_cptr")
    with pytest.raises(ValueError) as e:
        engine_options({**sp, "amg_gs_levels": 4}, model, decoup)
    assert "amg_gs_levels" in str(e.value) and "amg_full_levels" in str(e.value)
    engine_options({**sp, "amg_gs_levels": 4, "amg_full_levels": 4}, model, decoup)
    for bad in (dict(amg_gs_levels=-1), dict(amg_gs_levels=1.5), dict(amg_gs_levels=True), dict(amg_gs_levels=1, amg_gs_sweeps=0),
                dict(amg_gs_levels=1, amg_gs_sweeps=5), dict(amg_gs_levels=4)):
        with pytest.raises(ValueError):
            engine_options({**sp, **bad}, model, decoup)
        with pytest.raises(ValueError):
            check_amg_gs_options(dict(DEFAULT_OPTS, **bad))
    for g in (1, 2, 3, 4):
        check_amg_gs_options(dict(DEFAULT_OPTS, amg_gs_levels=3, amg_gs_sweeps=g))


def test_a_sweep_count_that_would_be_ignored_is_refused():
    sp, model, decoup = preset("pc_cptr")
    with pytest.raises(ValueError) as e:
        engine_options({**sp, "amg_gs_sweeps": 2}, model, decoup)
    assert "amg_gs_sweeps" in str(e.value) and "amg_gs_levels" in str(e.value)
    with pytest.raises(ValueError):
        check_amg_gs_options(dict(DEFAULT_OPTS, amg_gs_sweeps=2))
    engine_options({**sp, "amg_gs_sweeps": 1}, model, decoup)
    engine_options({**sp, "amg_gs_sweeps": 2, "amg_gs_levels": 1}, model, decoup)


def test_solver_parameters_refuse_amg_single_and_the_line_levels():
    sp, model, decoup = preset("pc_cptr")
    for other, kw in (("amg_single", dict(amg_single=True)), ("amg_line_levels", dict(amg_line_levels=1))):
        with pytest.raises(NotImplementedError) as e:
            engine_options({**sp, "amg_gs_levels": 1, **kw}, model, decoup)
        assert "amg_gs_levels" in str(e.value) and other in str(e.value)
        engine_options({**sp, **kw}, model, decoup)


def test_solver_parameters_refuse_the_system_amg():
    sp, model, decoup = preset("pc_cptramg")
    assert engine_options(sp, model, decoup)["pc"] == "cptramg"
    with pytest.raises(NotImplementedError) as e:
        engine_options({**sp, "amg_gs_levels": 1}, model, decoup)
    assert "amg_gs_levels" in str(e.value) and "cptramg" in str(e.value) and "pc_kind 3" in str(e.value)


@pytest.mark.parametrize("other,kw,nranks", [("amg_line_levels", dict(amg_line_levels=1), 1), ("amg_single", dict(amg_single=True), 1),
                                             ("cptramg", dict(pc="cptramg"), 1),
                                             ("schur_selfp", dict(pc="fieldsplit_cd", schur_selfp=True), 1), ("nranks", {}, 2)])
def test_engine_options_refuse_the_unsupported_combinations(other, kw, nranks):
    with pytest.raises(EngineError) as e:
        check_amg_gs_options(dict(DEFAULT_OPTS, amg_gs_levels=1, **kw), nranks)
    assert "amg_gs_levels" in str(e.value) and other in str(e.value)
    check_amg_gs_options(dict(DEFAULT_OPTS, **kw), nranks)               # each alone stays legal
