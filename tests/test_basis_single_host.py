"""The opt-in fp32 storage of the FGMRES bases (ksp_basis_single, tp_options.ksp_basis_single) on the host: the option's
plumbing -- engine keys, solver_parameters spelling, refusal with BiCGStab naming both keys, the range of ksp_single_floor, the
two fields added to the C struct, the exports in the engine's symbol list -- and the numpy reference the GPU tests compare
with (tests/basis_single_ref.py): every input is clear of the thresholds it meets, the summation-order floor is what the
module records, the iteration cost stays under the caps, the true residual is below the tolerance.  No GPU."""
import os
import re

import numpy as np
import pytest

import basis_single_ref as R
from thermalporous_amd.engine import API_SYMBOLS, DEFAULT_OPTS, HipEngine, check_ksp_basis_options, tp_options
from thermalporous_amd.solver_options import _flatten, engine_options
from test_bcgs_host import preset

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "thermalporous_hip.h")
_CACHE = {}
INPUTS = R.PARITY + [R.LONG]


def problem(p):
    name, shape, opts, dt, seed, kw = p
    if name not in _CACHE:
        spec, u0, u, o, J, F = R.oracle_problem(shape, opts, seed=seed, dt=dt)
        _CACHE[name] = (o, J, F)
    return _CACHE[name]


def floor_of(p):
    """summation_floor of an input at its own tolerance, computed once and shared."""
    key = ("floor", p[0])
    if key not in _CACHE:
        o, J, F = problem(p)
        _CACHE[key] = R.summation_floor(o, J, F, **R.solver_kw(p[5])[0])
    return _CACHE[key]


# ---- option plumbing -----------------------------------------------------------------------------------------------------------
def test_defaults_and_struct_fields():
    assert DEFAULT_OPTS["ksp_basis_single"] is False and DEFAULT_OPTS["ksp_single_floor"] == 1e-7
    names = [f[0] for f in tp_options._fields_]
    i = names.index("ksp_basis_single")            # (the struct's tail -- ksp_kind and the four s1_* fields -- keeps its place)
    assert names[i:i + 3] == ["ksp_basis_single", "ksp_single_floor", "ksp_kind"] and names[i - 1] == "amg_line_levels"
    hdr = open(HEADER).read()
    body = hdr[hdr.index("typedef struct tp_options {"):hdr.index("} tp_options;")]
    fields = re.findall(r"^\s*(?:int32_t|double)\s+([^;]+);", body, flags=re.M)
    fields = [f.strip() for f in fields]
    j = fields.index("ksp_basis_single")
    assert fields[j:j + 3] == ["ksp_basis_single", "ksp_single_floor", "ksp_kind"]
    o = HipEngine._make_options({**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8)})
    assert (o.ksp_basis_single, o.ksp_single_floor) == (0, 1e-7)
    o = HipEngine._make_options({**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8), "ksp_basis_single": True, "ksp_single_floor": 1e-6})
    assert (o.ksp_basis_single, o.ksp_single_floor) == (1, 1e-6)
    for sym in ("tp_ksp_basis_info", "tp_fvec_create_batch", "tp_fvec_store", "tp_fvec_get", "tp_fvec_dot_batch", "tp_fvec_axpy_batch"):
        assert sym in API_SYMBOLS and re.search(r"\bint %s\(" % sym, hdr)


@pytest.mark.parametrize("theta", [0.0, 2.0**-24, 1.0, 2.0, -1e-7, float("nan"), True, "1e-7", np.float32(1.0)])
def test_floor_out_of_range_is_a_value_error(theta):
    with pytest.raises(ValueError, match="ksp_single_floor"):
        check_ksp_basis_options({**DEFAULT_OPTS, "ksp_basis_single": True, "ksp_single_floor": theta})
    with pytest.raises(ValueError, match="ksp_single_floor"):          # checked whether or not the option is on
        check_ksp_basis_options({**DEFAULT_OPTS, "ksp_single_floor": theta})


def test_floor_in_range_and_bcgs_refusal():
    for theta in (1e-7, 1e-6, 0.5, 2.0**-23, np.float32(1e-6), np.float64(1e-7)):
        check_ksp_basis_options({**DEFAULT_OPTS, "ksp_basis_single": True, "ksp_single_floor": theta})
    check_ksp_basis_options({**DEFAULT_OPTS, "ksp": "bcgs"})           # BiCGStab alone stays legal
    with pytest.raises(NotImplementedError, match="ksp_basis_single.*bcgs"):
        check_ksp_basis_options({**DEFAULT_OPTS, "ksp_basis_single": True, "ksp": "bcgs"})


@pytest.mark.parametrize("name,two", [("pc_cpr", False), ("pc_cptr", True), ("pc_bilu", True)])
def test_solver_parameters_spelling(name, two):
    sp, mname, decoup, vector = preset(name, two)
    eo = lambda d: engine_options(d, mname, decoup, vector=vector)
    base = eo(sp)
    assert base["ksp_basis_single"] is False and base["ksp_single_floor"] == 1e-7
    on = eo({**sp, "ksp_basis_single": True, "ksp_single_floor": 1e-6})
    assert on["ksp_basis_single"] is True and on["ksp_single_floor"] == 1e-6
    rest = lambda o: {k: v for k, v in o.items() if k not in ("ksp_basis_single", "ksp_single_floor")}
    assert rest(on) == rest(base)
    with pytest.raises(NotImplementedError, match="ksp_basis_single.*fbcgs"):
        eo({**sp, "ksp_basis_single": True, "ksp_type": "fbcgs"})
    with pytest.raises(ValueError, match="ksp_single_floor"):
        eo({**sp, "ksp_basis_single": True, "ksp_single_floor": 1.0})


def test_engine_constructor_and_set_options_call_the_check():
    import inspect
    from thermalporous_amd.engine import check_options
    src = inspect.getsource(HipEngine.__init__) + inspect.getsource(HipEngine.set_options)
    assert src.count("check_options(") == 2 and inspect.getsource(check_options).count("check_ksp_basis_options(o)") == 1


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_without_rounding_is_gmres():
    """single = False on a dense system: the residual history decreases and x solves the system; single = True reaches the same
    solution to the tolerance, through the floor and a second cycle."""
    rng = np.random.default_rng(3)
    n = 40
    A = np.eye(n) + 0.3*rng.standard_normal((n, n))/np.sqrt(n)
    M = np.linalg.inv(A + 0.05*rng.standard_normal((n, n))/np.sqrt(n))
    b = rng.standard_normal(n)
    xs = np.linalg.solve(A, b)
    x, its, reason, hist, ncyc, orth = R.fgmres_ref(lambda v: A @ v, lambda v: M @ v, b, rtol=1e-12, single=False)
    assert reason == 2 and ncyc == 1 and np.linalg.norm(x - xs) <= 1e-10*np.linalg.norm(xs)
    assert all(hist[i + 1] <= hist[i]*(1 + 1e-12) for i in range(its))
    info = {}
    x, its1, reason, hist, ncyc, orth = R.fgmres_ref(lambda v: A @ v, lambda v: M @ v, b, rtol=1e-12, info=info)
    assert reason == 2 and ncyc >= 2 and np.linalg.norm(b - A @ x) <= 1e-12*np.linalg.norm(b) and info["rnorm"] <= 1e-12*np.linalg.norm(b)
    assert info["rnorm"] == info["cycles"][-1]["beta"] and np.linalg.norm(x - xs) <= 1e-10*np.linalg.norm(xs)
    # every cycle but the last stopped at its floor theta beta, not at tol
    assert all(c["stop"] == R.THETA*c["beta0"] for c in info["cycles"][:-1])
    # limits: b = 0, NaN, maxit
    assert R.fgmres_ref(lambda v: A @ v, lambda v: M @ v, 0*b)[1:3] == (0, 2)
    bn = b.copy()
    bn[3] = np.nan
    assert R.fgmres_ref(lambda v: A @ v, lambda v: M @ v, bn)[1:3] == (0, -9)
    out = R.fgmres_ref(lambda v: A @ v, lambda v: M @ v, b, rtol=1e-12, maxit=2, info=info)
    assert out[1:3] == (2, -3) and info["rnorm"] == info["cycles"][-1]["beta"] > 1e-12*np.linalg.norm(b)


@pytest.mark.parametrize("p", INPUTS, ids=[p[0] for p in INPUTS])
def test_inputs_are_clear_of_their_thresholds(p):
    fl, fw, rv, ifw, irv = floor_of(p)
    rtol = R.solver_kw(p[5])[0]["rtol"]
    tol = rtol*fw[3][0]
    factor = R.LONG_CLEAR if p is R.LONG else 2.0
    print(p[0], "its", fw[1], rv[1], "cycles", fw[4], rv[4], "orth %.1e" % fw[5], "floor %.2e" % fl,
          [("%.3g" % (c["stop"]/tol), ["%.3g" % (r/c["stop"]) for r in c["res"][-2:]], "%.3g" % (c["beta"]/tol)) for c in ifw["cycles"]])
    assert fw[2] == rv[2] == 2 and fw[1] == rv[1] and fw[4] == rv[4] >= 2
    assert R.clear_of_thresholds(ifw, tol, factor) and R.clear_of_thresholds(irv, tol, factor)
    assert ifw["rnorm"] <= tol and irv["rnorm"] <= tol
    if p[0] == "c4_cptr_restart5":
        assert len(ifw["cycles"][0]["res"]) == 5 and ifw["cycles"][0]["res"][-1] > 2*ifw["cycles"][0]["stop"]
    if p is R.LONG:
        assert fw[1] > 50 and len(ifw["cycles"][0]["res"]) == 30


def test_summation_floor_is_the_recorded_one():
    worst = max((floor_of(p)[0], p[0]) for p in INPUTS)
    print("floor", worst)
    assert worst[0] <= R.PARITY_FLOOR and worst[0] >= R.PARITY_FLOOR/2          # (re-measured: neither above nor far below)
    assert 10*R.PARITY_FLOOR <= R.PARITY_TOL <= 10.2*R.PARITY_FLOOR


@pytest.mark.parametrize("p", INPUTS, ids=[p[0] for p in INPUTS])
def test_iteration_cost_stays_under_the_caps(p):
    """rtol 1e-7: the fp64 count, in as many cycles as the fp64 solve takes (one, unless ksp_restart binds); 1e-8: at most 3
    more; 1e-10: at most 4 more.  The true residual is below the tolerance at each."""
    import oracle.linalg as la
    o, J, F = problem(p)
    restart = R.solver_kw(p[5])[0]["restart"]
    for rtol, cap in R.CAPS.items():
        d = R.solve_ref(o, J, F, rtol=rtol, restart=restart, single=False)
        s = R.solve_ref(o, J, F, rtol=rtol, restart=restart)
        tr = np.linalg.norm((F - la.spmv_block(J, s[0])).ravel())
        print(p[0], rtol, "fp32 basis", s[1], "cycles", s[4], "fp64", d[1], "cycles", d[4], "true/tol %.3f" % (tr/(rtol*s[3][0])))
        assert d[2] == s[2] == 2 and s[1] - d[1] <= cap, (rtol, s[1], d[1])
        if rtol == 1e-7:
            assert s[4] == d[4] and (restart < 200 or s[4] == 1)
        assert tr <= rtol*s[3][0]


def test_tight_tolerance_needs_the_second_cycle():
    name, rtol = R.TIGHT
    p = [q for q in R.PARITY if q[0] == name][0]
    o, J, F = problem(p)
    info = {}
    x, its, reason, hist, ncyc, orth = R.solve_ref(o, J, F, rtol=rtol, info=info)
    assert reason == 2 and ncyc >= 2 and info["rnorm"] <= rtol*hist[0]
    # without the floor the single cycle's recurrence residual goes below the tolerance while the true residual does not
    x1, its1, _, hist1, ncyc1, _ = R.solve_ref(o, J, F, rtol=rtol, theta=1e-300, maxit=its)
    import oracle.linalg as la
    tr1 = np.linalg.norm((F - la.spmv_block(J, x1)).ravel())
    print("tight", name, "its", its, "cycles", ncyc, "no floor: recurrence/tol %.2e true/tol %.2e" % (min(hist1)/(rtol*hist[0]), tr1/(rtol*hist[0])))
    assert tr1 > rtol*hist[0]


def test_one_long_cycle_of_a_slow_solve_crawls():
    """The limit of the method that DESIGN.md 4.6b records: the floor only helps if a cycle reaches it.  The 58-iteration input
    under ksp_restart 200 (one long cycle) loses the orthogonality of its rounded basis before it reaches theta beta and takes
    more than twice the fp64 iterations at rtol 1e-7; under FGMRES(30) it takes the fp64 count.  It still converges on a true
    residual: the option never reports a solve it has not finished."""
    import oracle.linalg as la
    o, J, F = problem(R.LONG)
    d = R.solve_ref(o, J, F, rtol=1e-7, restart=200, single=False)
    info = {}
    s = R.solve_ref(o, J, F, rtol=1e-7, restart=200, info=info)
    s30, d30 = R.solve_ref(o, J, F, rtol=1e-7, restart=30), R.solve_ref(o, J, F, rtol=1e-7, restart=30, single=False)
    print("restart 200: fp32 basis", s[1], "fp64", d[1], "orth %.2f" % s[5], "; restart 30:", s30[1], d30[1])
    assert d[2] == s[2] == 2 and s[1] > 2*d[1] and s[5] > 0.5
    assert np.linalg.norm((F - la.spmv_block(J, s[0])).ravel()) <= 1e-7*s[3][0] and info["rnorm"] <= 1e-7*s[3][0]
    assert s30[2] == 2 and s30[1] == d30[1]
