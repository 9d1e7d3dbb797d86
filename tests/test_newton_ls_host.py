"""The opt-in backtracking line search, everything that needs no GPU: the options translation and its refusals, the chooser of the
next trial length, the numpy reference tests/newton_ls_ref.py on the inputs the GPU tests compare against (and the two conditions
those inputs must meet), and the host time loop on an oracle engine that runs the reference."""
import math

import numpy as np
import pytest

import cases
import newton_ls_ref as R
from thermalporous_amd import engine as E
from thermalporous_amd import exceptions
from thermalporous_amd.solver_options import engine_options
from thermalporous_amd.twophase import TwoPhase

_CACHE = {}


def ref(name):
    """The reference results on a named input, computed once and shared (never modified)."""
    if name not in _CACHE:
        if name == "D":
            _CACHE[name] = R.run_ref_D(3)
        elif name == "E":
            _CACHE[name] = R.run_ref("c3", R.A_OPTS, 0.1, dict(ls_max_it=1))
        elif name == "F":
            _CACHE[name] = R.run_ref("c3", R.F_OPTS, 0.1, dict(ls_max_change=R.F_CAP))
        else:
            _, case, opts, dt, ls = [p for p in R.PARITY + [R.C_INPUT] if p[0] == name][0]
            floor, a, b = R.sensitivity_floor(case, opts, dt, ls)
            _CACHE[name] = (floor, a, b, R.run_ref(case, opts, dt, {}, linesearch="basic")[2])
    return _CACHE[name]


def cptr_parameters():
    spec, u0, p, g, c = cases.c3_spe10_2d(6, 8, 2)
    from oracle.engine import OracleEngine
    m = TwoPhase(g, c, p, end=0.01, maxdt=0.01, solver_parameters="pc_cptr", filename=None, verbosity=False, _engine_factory=OracleEngine)
    return dict(m.solver_parameters)


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_petsc_keys_translate_and_every_refusal_raises():
    d = cptr_parameters()
    o = engine_options(d, "Two-phase")
    assert o["linesearch"] == "basic" and o["ls_order"] == 3 and o["ls_max_change"] is None
    o = engine_options({**d, "snes_linesearch_type": "basic"}, "Two-phase")
    assert o["linesearch"] == "basic"
    o = engine_options({**d, "snes_linesearch_type": "bt"}, "Two-phase")          # (raises without the feature)
    assert o["linesearch"] == "bt" and (o["ls_order"], o["ls_alpha"], o["ls_max_it"], o["ls_maxstep"], o["ls_minlambda"]) == (3, 1e-4, 40, 1e8, 1e-12)
    o = engine_options({**d, "snes_linesearch_type": "bt", "snes_linesearch_order": 2, "snes_linesearch_alpha": 1e-3,
                        "snes_linesearch_max_it": 7, "snes_linesearch_maxstep": 50.0, "snes_linesearch_minlambda": 1e-6,
                        "ls_max_change": (0.0, 0.0, 0.2)}, "Two-phase")
    assert (o["ls_order"], o["ls_alpha"], o["ls_max_it"], o["ls_maxstep"], o["ls_minlambda"]) == (2, 1e-3, 7, 50.0, 1e-6)
    assert o["ls_max_change"] == (0.0, 0.0, 0.2)
    assert engine_options({**d, "linesearch": "bt", "ls_order": 2}, "Two-phase")["ls_order"] == 2          # build keys
    for other in ("l2", "cp", "nleqerr"):
        with pytest.raises(NotImplementedError):
            engine_options({**d, "snes_linesearch_type": other}, "Two-phase")
    for k, v in (("snes_linesearch_order", 2), ("snes_linesearch_alpha", 1e-3), ("snes_linesearch_max_it", 5),
                 ("snes_linesearch_maxstep", 10.0), ("snes_linesearch_minlambda", 1e-8)):
        with pytest.raises(NotImplementedError):
            engine_options({**d, k: v}, "Two-phase")                                  # without bt
        with pytest.raises(NotImplementedError):
            engine_options({**d, "snes_linesearch_type": "basic", k: v}, "Two-phase")
    with pytest.raises(ValueError):
        engine_options({**d, "ls_order": 2}, "Two-phase")                             # a bt build key under basic
    with pytest.raises(ValueError):
        engine_options({**d, "ls_max_change": (0.0, 0.0, 0.1)}, "Two-phase")
    with pytest.raises(ValueError):
        engine_options({**d, "linesearch": "basic", "snes_linesearch_type": "bt"}, "Two-phase")       # configured twice, differently
    with pytest.raises(KeyError):
        engine_options({**d, "snes_linesearch_type": "bt", "snes_linesearch_damping": 0.5}, "Two-phase")


@pytest.mark.parametrize("bad", [dict(ls_order=1), dict(ls_order=4), dict(ls_order=True), dict(ls_alpha=0.0), dict(ls_alpha=0.5),
                                 dict(ls_alpha=-1e-4), dict(ls_max_it=0), dict(ls_max_it=2.5), dict(ls_maxstep=0.0), dict(ls_maxstep=-1.0),
                                 dict(ls_minlambda=-1e-3), dict(ls_minlambda=1.0), dict(ls_max_change=(1.0, 2.0)),
                                 dict(ls_max_change=(1.0, float("nan"), 0.0))])
def test_check_linesearch_options_ranges(bad):
    E.check_linesearch_options({**E.DEFAULT_OPTS, "linesearch": "bt"})
    with pytest.raises(ValueError):
        E.check_linesearch_options({**E.DEFAULT_OPTS, "linesearch": "bt", **bad})


def test_check_linesearch_options_kind_and_defaults_under_basic():
    E.check_linesearch_options(dict(E.DEFAULT_OPTS))
    E.check_linesearch_options({**E.DEFAULT_OPTS, "ls_max_change": (0.0, -1.0, 0.0)})       # no cap at all: nothing to ignore
    with pytest.raises(NotImplementedError):
        E.check_linesearch_options({**E.DEFAULT_OPTS, "linesearch": "l2"})
    for k, v in (("ls_order", 2), ("ls_alpha", 1e-3), ("ls_max_it", 10), ("ls_maxstep", 1.0), ("ls_minlambda", 1e-6),
                 ("ls_max_change", (0.0, 0.0, 0.1))):
        with pytest.raises(ValueError):
            E.check_linesearch_options({**E.DEFAULT_OPTS, k: v})


def test_options_are_packed_into_tp_options():
    names = [f[0] for f in E.tp_options._fields_]
    i = names.index("ls_kind")                # (between ilu_single and amg_line_levels: the fields behind keep the order earlier tests pin)
    assert names[i:i + 7] == ["ls_kind", "ls_order", "ls_max_it", "ls_alpha", "ls_maxstep", "ls_minlambda", "ls_max_change"]
    assert names[i - 1] == "ilu_single" and names[i + 7] == "amg_line_levels" and names[-1] == "s1_atol"
    o = E.resolve_ilu_options(dict(E.DEFAULT_OPTS), (12, 16, 1))
    t = E.HipEngine._make_options(o)
    assert (t.ls_kind, t.ls_order, t.ls_max_it, t.ls_alpha, t.ls_maxstep, t.ls_minlambda) == (0, 3, 40, 1e-4, 1e8, 1e-12)
    assert list(t.ls_max_change) == [0.0, 0.0, 0.0]
    t = E.HipEngine._make_options({**o, "linesearch": "bt", "ls_order": 2, "ls_max_it": 9, "ls_alpha": 0.01, "ls_maxstep": 3.0,
                                   "ls_minlambda": 1e-5, "ls_max_change": (1.0, 2.0, 0.25)})
    assert (t.ls_kind, t.ls_order, t.ls_max_it, t.ls_alpha, t.ls_maxstep, t.ls_minlambda) == (1, 2, 9, 0.01, 3.0, 1e-5)
    assert list(t.ls_max_change) == [1.0, 2.0, 0.25]
    for name in ("tp_ls_info", "tp_ls_history", "tp_ls_step_stats", "tp_ls_trial"):
        assert name in E.API_SYMBOLS


# ---- the chooser -------------------------------------------------------------------------------------------------------------
def test_chooser_quadratic_value_and_clamps():
    f0, g0 = 2.0, -4.0                                       # ||F0||^2 = 4
    # quadratic model m(l) = f0 + g0 l + c l^2 through (1, f): c = f - f0 - g0, minimiser -g0 / (2 c)
    for f, want in ((3.0, 0.4), (6.0, 0.25), (10.5, 0.16)):
        assert R.next_lambda(2, g0, f0, [(1.0, 2.0*f)]) == pytest.approx(want, rel=1e-15)
    # the same from lambda = 0.5: minimiser -g0 l^2 / (2 (f - f0 - g0 l))
    assert R.next_lambda(2, g0, f0, [(0.5, 2.0*3.0)]) == pytest.approx(4*0.25/(2*(3.0 - 2.0 + 2.0)), rel=1e-15)
    assert R.next_lambda(3, g0, f0, [(1.0, 6.0)]) == R.next_lambda(2, g0, f0, [(1.0, 6.0)])      # order 3 with one trial: quadratic
    assert R.next_lambda(2, g0, f0, [(1.0, 2.0*1e6)]) == 0.1                                     # lower clamp
    assert R.next_lambda(2, g0, f0, [(1.0, 2.0*(2.0 - 4e-4 + 1e-9))]) == 0.5                     # barely rejected: upper clamp
    assert R.next_lambda(2, g0, f0, [(0.3, 2.0*1e6)]) == 0.1*0.3
    assert R.next_lambda(2, g0, f0, [(1.0, float("inf"))]) == 0.1                                # (finite is the caller's test)


def test_chooser_cubic_recovers_the_minimiser_of_a_cubic_model():
    # f(l) = f0 + g0 l + b l^2 + a l^3 with its local minimiser inside the clamp window of the last trial
    f0, g0, a, b = 2.0, -4.0, 20.0, 1.0
    f = lambda l: f0 + g0*l + b*l*l + a*l*l*l
    lmin = (-b + math.sqrt(b*b - 3*a*g0))/(3*a)             # 0.2419...
    got = R.next_lambda(3, g0, f0, [(1.0, 2*f(1.0)), (0.5, 2*f(0.5))])
    assert 0.05 <= lmin <= 0.25 and got == pytest.approx(lmin, rel=1e-12)
    # a = 0: the cubic degenerates to the quadratic minimiser
    f = lambda l: f0 + g0*l + 10.0*l*l
    assert R.next_lambda(3, g0, f0, [(1.0, 2*f(1.0)), (0.5, 2*f(0.5))]) == pytest.approx(0.2, rel=1e-12)
    # clamps apply to the cubic too
    f = lambda l: f0 + g0*l + 1e4*l*l*l
    assert R.next_lambda(3, g0, f0, [(1.0, 2*f(1.0)), (0.5, 2*f(0.5))]) == 0.05


def test_chooser_negative_discriminant_halves():
    # two trials whose cubic has b^2 - 3 a g0 < 0 (a < 0 steep enough): no real stationary point
    f0, g0, a, b = 2.0, -4.0, -30.0, 1.0
    assert b*b - 3*a*g0 < 0
    f = lambda l: f0 + g0*l + b*l*l + a*l*l*l
    assert R.next_lambda(3, g0, f0, [(1.0, 2*f(1.0)), (0.4, 2*f(0.4))]) == 0.2


def test_nonfinite_trials_halve_and_reset_the_history():
    """Input D: a non-finite residual halves lambda exactly and forgets the finite trials before it."""
    spec, u0, first, d = ref("D")
    assert first["reason"] == -5 and first["nits"] == 1 and np.isfinite(first["u"]).all()
    for k, v in R.D_EXPECT.items():
        assert d[k] == v, (k, d[k])
    assert d["nits"] == 2 and d["margin"] >= R.MARGIN_MIN
    _, _, _, d2 = R.run_ref_D(2)
    assert d2["lam"] == d["lam"] and d2["nonfinite"] == d["nonfinite"]        # no finite rejected trial: the order cannot matter


# ---- the reference on the inputs of the GPU comparison ------------------------------------------------------------------------
def test_parity_inputs_meet_both_conditions_and_basic_fails_where_bt_converges():
    worst = 0.0
    for name, case, opts, dt, ls in R.PARITY:
        floor, a, b, basic = ref(name)
        (reason, nits, trials), (breason, bnits) = R.EXPECT[name]
        print("%-9s basic %d after %d; bt %d in %d its, %d evaluations, lits %d; margin %.4f; floor %.3e" %
              (name, basic["reason"], basic["nits"], a["reason"], a["nits"], a["evaluations"], a["lits"], a["margin"], floor))
        print("   lambda", a["lam"])
        assert (basic["reason"], basic["nits"]) == (breason, bnits), name
        assert (a["reason"], a["nits"], a["trials"]) == (reason, nits, trials), name
        assert a["evaluations"] == sum(trials) and not a["nonfinite"]
        assert a["fnorm"] <= opts.get("snes_rtol", 1e-8)*a["fnorm0"]
        assert a["margin"] >= R.MARGIN_MIN, (name, a["margin"])
        assert floor < R.FLOOR_MAX, (name, floor)
        worst = max(worst, floor)
    print("floor %.3e  tolerance %.3e" % (worst, R.PARITY_TOL))
    assert 10*worst <= R.PARITY_TOL <= 10.2*R.PARITY_FLOOR and worst <= 1.01*R.PARITY_FLOOR
    # the two orders agree until two finite rejected trials exist: from the third lambda on they differ
    l2, l3 = ref("A_order2")[1]["lam"], ref("A_order3")[1]["lam"]
    assert l2[:2] == l3[:2] and l2[0] == pytest.approx(0.1964, abs=5e-5) and l2[1] == pytest.approx(0.2692, abs=5e-5)
    assert l2[2] == pytest.approx(0.0558, abs=5e-5) and l3[2] == pytest.approx(0.0517, abs=5e-5) and l2[3] == pytest.approx(0.0227, abs=5e-5)
    assert l2[4:] == l3[4:] == [1.0, 1.0]


def test_full_steps_reproduce_basic_bitwise():
    """Input C: every first trial is accepted, and the iterates are those of the basic solver, bit for bit."""
    floor, a, b, basic = ref("C")
    assert a["reason"] == basic["reason"] == 3 and a["nits"] == basic["nits"] == 3
    assert a["lam"] == [1.0]*3 and a["trials"] == [1]*3 and a["evaluations"] == 3
    assert np.array_equal(a["u"], basic["u"]) and a["hist"] == basic["hist"]
    _, _, a30 = R.run_ref("c1", R.C_OPTS, 30.0, {})
    _, _, b30 = R.run_ref("c1", R.C_OPTS, 30.0, {}, linesearch="basic")
    assert a30["lam"] == [1.0]*5 and np.array_equal(a30["u"], b30["u"])


def test_failed_search_restores_the_state():
    """Input E: ls_max_it 1 on A, whose first trial is rejected."""
    spec, u0, e = ref("E")
    assert e["reason"] == R.SNES_DIVERGED_LINE_SEARCH and e["nits"] == 0 and e["evaluations"] == 1
    assert np.array_equal(e["u"], u0) and e["fnorm"] == e["fnorm0"] and e["lam"] == []
    # minlambda: the same input with a floor above the second trial length
    _, _, m = R.run_ref("c3", R.A_OPTS, 0.1, dict(ls_minlambda=0.5))
    assert m["reason"] == -6 and m["evaluations"] == 1 and np.array_equal(m["u"], u0)


def test_first_trial_rule():
    """Input F: the S_o cap halves the first step; maxstep acts on ||dx||."""
    spec, u0, f = ref("F")
    reason, nits, trials = R.F_EXPECT
    assert (f["reason"], f["nits"], f["trials"]) == (reason, nits, trials)
    assert f["first"][0] == pytest.approx(0.5, rel=1e-9) and f["lam"][0] == f["first"][0]
    assert all(l <= 1.0 for l in f["first"]) and f["margin"] >= R.MARGIN_MIN
    floor = R.sensitivity_floor("c3", R.F_OPTS, 0.1, dict(ls_max_change=R.F_CAP))[0]
    print("F: margin %.4f floor %.3e" % (f["margin"], floor))
    assert floor <= R.PARITY_FLOOR                         # (its history is compared at the same tolerance)
    # caps on fields whose step is small do not bind; a cap <= 0 is off
    _, _, g = R.run_ref("c3", R.A_OPTS, 0.1, dict(ls_max_change=(1e6, 1e6, -1.0)))
    assert g["lam"] == ref("A_order3")[1]["lam"]
    # maxstep: ||dx|| of the first iteration is 113.0: maxstep 11.3 gives lambda = 0.1
    _, _, s = R.run_ref("c3", {**R.A_OPTS, "snes_max_it": 1}, 0.1, dict(ls_maxstep=11.301546632808706))
    assert s["first"][0] == pytest.approx(0.1, rel=1e-9)


# ---- the host time loop ----------------------------------------------------------------------------------------------------------
def first_step(linesearch):
    spec, u0, p, g, c = cases.c3_spe10_2d(12, 16, 2)
    d = cptr_parameters()
    d.update({"snes_linesearch_type": linesearch, "ksp_rtol": 1e-10})
    m = TwoPhase(g, c, p, end=1.0, maxdt=0.1, small_dt_start=False, solver_parameters=d, filename=None, verbosity=False,
                 _engine_factory=R.LsOracleEngine)
    m.start()
    m.step()
    return m


def test_cold_first_time_step_needs_no_dt_halving_with_bt():
    bt = first_step("bt")
    assert bt.engine.opts["linesearch"] == "bt" and bt.failed_solves == 0 and bt.dt_vec == [0.1*86400.0]
    assert bt.engine.last["ls_trials"] > bt.nits_vec[0]                 # (it did backtrack)
    basic = first_step("basic")
    assert basic.failed_solves >= 1 and basic.dt_vec[0] < 0.1*86400.0


def test_failed_search_is_a_convergence_error_and_the_loop_halves_dt():
    """reason -6 is raised like any other divergence; the time loop halves dt and goes on."""
    spec, u0, p, g, c = cases.c3_spe10_2d(12, 16, 2)
    d = cptr_parameters()
    d.update({"snes_linesearch_type": "bt", "snes_linesearch_max_it": 1, "ksp_rtol": 1e-10})
    m = TwoPhase(g, c, p, end=1.0, maxdt=0.1, small_dt_start=False, solver_parameters=d, filename=None, verbosity=False,
                 _engine_factory=R.LsOracleEngine)
    m.start()
    with pytest.raises(exceptions.ConvergenceError):
        m.solver.solve()
    assert m.engine.last["reason"] == -6
    m.start()
    m.step()
    assert m.failed_solves >= 1 and m.dt_vec[0] == 0.1*86400.0/2**m.failed_solves
