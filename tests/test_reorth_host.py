"""Gram-Schmidt refinement of the outer FGMRES (ksp_reorth): what can be checked without a GPU -- the option
plumbing, and the numpy reference tests/reorth_ref.py on the very inputs the GPU tests use (tests/test_gpu_reorth.py): that
the reference itself separates one pass from two, the criterion's edge cases, and the summation-order floor behind the
tolerance of the GPU comparison."""
import ctypes as C
import os

import numpy as np
import pytest

import reorth_ref as RR
from optpack import differing_fields
from thermalporous_amd.engine import (API_SYMBOLS, DEFAULT_OPTS, HipEngine, check_ksp_reorth_options, tp_options)
from thermalporous_amd.solver_options import engine_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thermalporous_hip.h")


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_defaults_struct_fields_and_exports():
    assert DEFAULT_OPTS["ksp_reorth"] == "never" and DEFAULT_OPTS["ksp_reorth_eta"] == 2.0**-0.5
    names = [f[0] for f in tp_options._fields_]
    i = names.index("ksp_reorth")
    assert names[i:i + 2] == ["ksp_reorth", "ksp_reorth_eta"]
    assert dict(tp_options._fields_)["ksp_reorth"] is C.c_int32 and dict(tp_options._fields_)["ksp_reorth_eta"] is C.c_double
    assert tp_options.ksp_reorth_eta.offset % C.sizeof(C.c_double) == 0
    assert "tp_ksp_reorth_info" in API_SYMBOLS and "tp_vec_orth_step" in API_SYMBOLS
    text = open(HEADER).read()
    assert "int tp_ksp_reorth_info(tp_ctx *ctx, int64_t out[4]);" in text and "int tp_vec_orth_step(" in text
    base = dict(DEFAULT_OPTS, ilu_tile=(1 << 30, 8, 8))
    o = HipEngine._make_options(base)
    assert (o.ksp_reorth, o.ksp_reorth_eta) == (0, 2.0**-0.5)
    for mode, code in (("never", 0), ("ifneeded", 1), ("always", 2)):
        o = HipEngine._make_options(dict(base, ksp_reorth=mode, ksp_reorth_eta=0.25))
        assert (o.ksp_reorth, o.ksp_reorth_eta) == (code, 0.25)
    # every other field is what it was without the keys
    a, b = HipEngine._make_options(base), HipEngine._make_options(dict(base, ksp_reorth="always"))
    assert differing_fields(a, b) <= {"ksp_reorth"}


SP = {"snes_type": "newtonls", "ksp_type": "fgmres", "mat_type": "aij", "pc_type": "bjacobi", "sub_pc_type": "ilu"}


@pytest.mark.parametrize("petsc,mode", [("refine_never", "never"), ("refine_ifneeded", "ifneeded"), ("refine_always", "always")])
def test_petsc_spelling_maps_onto_the_engine_key(petsc, mode):
    o = engine_options({**SP, "ksp_gmres_cgs_refinement_type": petsc}, "Two-phase")
    assert o["ksp_reorth"] == mode and o["ksp_reorth_eta"] == 2.0**-0.5
    assert engine_options(SP, "Two-phase")["ksp_reorth"] == "never"
    # the build keys pass through, alone or agreeing with the PETSc key
    o = engine_options({**SP, "ksp_reorth": mode, "ksp_reorth_eta": 0.5}, "Two-phase")
    assert (o["ksp_reorth"], o["ksp_reorth_eta"]) == (mode, 0.5)
    assert engine_options({**SP, "ksp_reorth": mode, "ksp_gmres_cgs_refinement_type": petsc}, "Two-phase")["ksp_reorth"] == mode


def test_stated_twice_and_differently_raises():
    with pytest.raises(ValueError, match="twice"):
        engine_options({**SP, "ksp_reorth": "always", "ksp_gmres_cgs_refinement_type": "refine_never"}, "Two-phase")
    with pytest.raises(ValueError, match="twice"):
        engine_options({**SP, "ksp_reorth": "never", "ksp_gmres_cgs_refinement_type": "refine_ifneeded"}, "Two-phase")
    with pytest.raises(NotImplementedError):
        engine_options({**SP, "ksp_gmres_cgs_refinement_type": "refine_sometimes"}, "Two-phase")


@pytest.mark.parametrize("eta", [0.0, 1.0, -0.5, 1.5, float("nan"), "0.5", True, None])
def test_eta_outside_the_open_interval_raises_whatever_the_mode(eta):
    for mode in RR.MODES:
        with pytest.raises(ValueError, match="ksp_reorth_eta"):
            check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp_reorth=mode, ksp_reorth_eta=eta))
    with pytest.raises(ValueError, match="ksp_reorth_eta"):
        engine_options({**SP, "ksp_reorth_eta": eta}, "Two-phase")


def test_unknown_mode_raises():
    with pytest.raises(ValueError, match="ksp_reorth"):
        check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp_reorth="sometimes"))


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_refused_combinations_name_both_keys(mode):
    with pytest.raises(NotImplementedError, match=r"ksp_reorth.*bcgs"):
        check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp_reorth=mode, ksp="bcgs"))
    with pytest.raises(NotImplementedError, match=r"ksp_reorth.*ksp_basis_single.*2\^-24"):
        check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp_reorth=mode, ksp_basis_single=True))
    petsc = "refine_" + mode
    with pytest.raises(NotImplementedError, match=r"ksp_reorth.*bcgs"):
        engine_options({**SP, "ksp_type": "fbcgs", "ksp_gmres_cgs_refinement_type": petsc}, "Two-phase")
    with pytest.raises(NotImplementedError, match=r"ksp_reorth.*ksp_basis_single"):
        engine_options({**SP, "ksp_basis_single": True, "ksp_gmres_cgs_refinement_type": petsc}, "Two-phase")
    # "never" goes with both
    check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp="bcgs"))
    check_ksp_reorth_options(dict(DEFAULT_OPTS, ksp_basis_single=True))
    assert engine_options({**SP, "ksp_type": "fbcgs", "ksp_gmres_cgs_refinement_type": "refine_never"}, "Two-phase")["ksp"] == "bcgs"


def test_modified_gram_schmidt_key_is_still_not_consumed():
    with pytest.raises(KeyError):
        engine_options({**SP, "ksp_gmres_modifiedgramschmidt": True}, "Two-phase")


# ---- the reference on the GPU tests' inputs -----------------------------------------------------------------------------------
def test_vector_shapes_are_those_of_the_grids():
    import cases
    for name, (builder, kw) in RR.SHAPES.items():
        spec, *_ = getattr(cases, builder)(**kw)
        assert (int(spec["nphase"]) + 1,) + tuple(spec["phi"].shape) == RR.VSHAPE[name], (name, spec["phi"].shape)
    assert np.prod(RR.VSHAPE["g2d"][1:]) < 256 and np.prod(RR.VSHAPE["g3d"]) % (256*8) != 0


def _figures():
    out = {}
    for delta in RR.DELTAS:
        one, two = [], []
        for shape in RR.SHAPES:
            for k in RR.KS:
                V, w = RR.near_dependent(shape, k, delta)
                # the inputs are what they claim to be: orthonormal to rounding, ||w||^2 = 1 + delta^2
                gram = max(abs(RR.dot_forward(V[i], V[j]) - (i == j)) for i in range(k) for j in range(k))
                assert gram < 1e-14 and abs(RR.dot_forward(w, w) - 1.0 - delta*delta) < 1e-14
                h1, n1, r1, w1 = RR.orth_step(V, w, "never")
                h2, n2, r2, w2 = RR.orth_step(V, w, "always")
                hi, ni, ri, wi = RR.orth_step(V, w, "ifneeded")
                assert (r1, r2, ri) == (False, True, True)                  # delta < eta: the default criterion fires
                assert np.array_equal(hi, h2) and ni == n2 and np.array_equal(wi, w2)
                assert abs(np.sqrt(n2) - delta) <= 1e-7*delta + 4e-16
                one.append(RR.orth_figure(V, w1))
                two.append(RR.orth_figure(V, w2))
        out[delta] = (min(one), max(one), max(two))
    return out


def test_reference_separates_one_pass_from_two():
    """One pass leaves the new vector orthogonal to the basis to ~ eps / delta only; the second pass brings it to ~ eps.  At
    delta = 1e-8 the two differ by at least reorth_ref.SEPARATION = 1e4: the condition the GPU test reuses, shown here for the
    reference alone, with the measured figures kept as constants in reorth_ref.py."""
    eps = np.finfo(float).eps
    fig = _figures()
    for delta, (lo, hi, two) in fig.items():
        print("delta %g: one pass %.3e .. %.3e (eps/delta %.3e), two passes <= %.3e" % (delta, lo, hi, eps/delta, two))
        assert 0.1*eps/delta <= hi <= 10*eps/delta                      # "about eps / delta"
        assert two <= 16*eps
        for got, rec in ((lo, RR.ONE_PASS_FIGURE[delta][0]), (hi, RR.ONE_PASS_FIGURE[delta][1]), (two, RR.TWO_PASS_FIGURE[delta])):
            assert rec/1.01 <= got <= 1.01*rec, (delta, got, rec)
    lo, hi, two = fig[1e-8]
    assert lo >= RR.SEPARATION*two


def test_summation_order_floor_is_what_the_tolerance_was_derived_from():
    """reorth_ref.STEP_TOL = 10 x the largest deviation between the forward and the reversed sums of the reference step over
    every shape, k and mode, per delta (the project's convention for sums taken in another order: tests/bcgs_ref.py)."""
    for delta in RR.DELTAS:
        worst = max(RR.step_floor(shape, k, delta) for shape in RR.SHAPES for k in RR.KS)
        print("delta %g: floor %.3e tolerance %.3e" % (delta, worst, RR.STEP_TOL[delta]))
        assert 0.9*RR.STEP_FLOOR[delta] <= worst <= RR.STEP_FLOOR[delta]
        assert 10*worst <= RR.STEP_TOL[delta] <= 10.01*RR.STEP_FLOOR[delta]


def test_criterion_edge_cases():
    V, w = RR.near_dependent("g2d", 5, 1e-4)
    # exactly orthogonal w: h = 0 exactly (a vector with disjoint support), no refinement at any eta
    sup = [np.zeros_like(w) for _ in range(2)]
    sup[0].flat[3], sup[1].flat[7] = 1.0, 1.0
    u = np.zeros_like(w)
    u.flat[20:30] = 1.0
    for eta in (1e-12, RR.ETA, 1.0 - 1e-12):
        h, n, ran, out = RR.orth_step(sup, u, "ifneeded", eta)
        assert not ran and not h.any() and n == 10.0 and np.array_equal(out, u)
    # ... and one orthogonal to rounding only: still none at the default eta
    h, n, ran, _ = RR.orth_step(V, RR.orth_step(V, w, "always")[3], "ifneeded")
    assert not ran
    # w in span(V): n1 ~ 0 (or exactly 0), refine, nothing divides
    a = np.arange(1.0, 6.0)
    ws = sum(a[i]*V[i] for i in range(5))
    with np.errstate(all="raise"):
        h, n, ran, _ = RR.orth_step(V, ws, "ifneeded")
        assert ran and n < 1e-28 and np.allclose(h, a, rtol=1e-14)
        h, n, ran, _ = RR.orth_step(sup, 3.0*sup[0], "ifneeded")
        assert ran and n == 0.0 and list(h) == [3.0, 0.0]
        # w = 0: nothing to refine
        h, n, ran, _ = RR.orth_step(sup, np.zeros_like(w), "ifneeded")
        assert not ran and n == 0.0
    assert RR.criterion([3.0, 0.0], 0.0, RR.ETA) and not RR.criterion([0.0], 0.0, RR.ETA)
    # NaN in w: no refinement, and the NaN propagates as in the one-pass step
    wn = w.copy()
    wn.flat[11] = np.nan
    h, n, ran, out = RR.orth_step(V, wn, "ifneeded")
    h1, n1, _, out1 = RR.orth_step(V, wn, "never")
    assert not ran and np.isnan(n) and np.isnan(h).all() and np.array_equal(h, h1, equal_nan=True) and np.array_equal(out, out1, equal_nan=True)
    assert not RR.criterion([np.inf], 1.0, RR.ETA) and not RR.criterion([1.0], np.inf, RR.ETA) and not RR.criterion([1.0], np.nan, RR.ETA)
    # "always" refines whatever the sums are
    assert RR.orth_step(V, wn, "always")[2]


def test_fgmres_reference_modes_agree_on_a_small_system():
    """fgmres_ref on a dense, well-conditioned system: every mode converges to the same solution; "ifneeded" with a tiny eta is
    "never" bit for bit, and with eta close to 1 it is "always"."""
    rng = np.random.default_rng(3)
    n = 40
    A = np.eye(n) + 0.3*rng.standard_normal((n, n))/np.sqrt(n)
    b = rng.standard_normal(n)
    res = {}
    for mode, eta in (("never", RR.ETA), ("always", RR.ETA), ("ifneeded", 1e-12), ("ifneeded", 1.0 - 1e-12)):
        info = {}
        x, its, reason, hist = RR.fgmres_ref(lambda v: A @ v, lambda v: v.copy(), b, rtol=1e-10, mode=mode, eta=eta, info=info)
        assert reason == 2 and np.linalg.norm(A @ x - b) <= 1e-9*np.linalg.norm(b)
        res[(mode, eta)] = (x, its, hist, info)
    assert not any(res[("ifneeded", 1e-12)][3]["fired"]) and all(res[("always", RR.ETA)][3]["fired"])
    assert np.array_equal(res[("ifneeded", 1e-12)][0], res[("never", RR.ETA)][0]) and res[("ifneeded", 1e-12)][2] == res[("never", RR.ETA)][2]
    assert all(res[("ifneeded", 1.0 - 1e-12)][3]["fired"])
    assert np.array_equal(res[("ifneeded", 1.0 - 1e-12)][0], res[("always", RR.ETA)][0])
    assert abs(res[("always", RR.ETA)][1] - res[("never", RR.ETA)][1]) <= 1


def test_fgmres_floor_on_the_parity_systems_is_what_the_tolerance_was_derived_from():
    """Every system of bcgs_ref.PARITY under "always" and "ifneeded": the reference converges in both summation orders after the
    same number of iterations and with the same criteria fired; the largest deviation between the two orders is the floor
    behind reorth_ref.FGMRES_TOL = 10 x floor."""
    import bcgs_ref as R
    worst = 0.0
    for name, shape, opts, dt, seed in R.PARITY:
        spec, u0, u, o, J, F = R.oracle_problem(shape, opts, seed=seed, dt=dt)
        for mode in ("always", "ifneeded"):
            floor, fw, rv, info = RR.fgmres_floor(o, J, F, mode)
            print("%-16s %-8s its %2d / %2d  second passes %2d  floor %.3e" % (name, mode, fw[1], rv[1], sum(info["fired"]), floor))
            assert fw[2] == rv[2] == 2 and fw[1] == rv[1], (name, mode)
            assert mode != "always" or all(info["fired"])
            worst = max(worst, floor)
    print("floor %.3e  tolerance %.3e" % (worst, RR.FGMRES_TOL))
    assert worst <= 1.01*RR.FGMRES_FLOOR and 10*worst <= RR.FGMRES_TOL <= 10.2*RR.FGMRES_FLOOR
