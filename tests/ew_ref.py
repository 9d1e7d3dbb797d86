"""Eisenstat-Walker inexact Newton in numpy: the reference of the GPU driver (newton() in thermalporous_amd/csrc/tp_solver.hip,
tp_options.ksp_ew; the chooser is thermalporous_amd/csrc/tp_ew.hpp), built on the oracle's residual, Jacobian and linear solve.

The tolerance eta_k of linear solve k = 0, 1, ... of one Newton solve, with ||F_k|| the residual norm where system k is formed
and rho_k the residual norm the Krylov solver returned for it:

    k == 0:     eta = rtol0
    version 1:  eta = | ||F_k|| - rho_{k-1} | / ||F_{k-1}|| ;          s = pow(eta_{k-1}, alpha2)
    version 2:  eta = gamma pow(||F_k|| / ||F_{k-1}||, alpha) ;        s = gamma pow(eta_{k-1}, alpha)
    k > 0:      if s > threshold: eta = max(eta, s)                    (safeguard)
    always:     eta = min(eta, rtolmax); eta = max(eta, ksp_rtol)      (cap, then floor: ksp_rtol stays, PETSc overwrites it)

Solve k stops at max(eta_k ||F_k||, ksp_atol).  next_rtol is written operation by operation as the C++ writes it, and both call
libm's pow: the same inputs give the same bits.  The GPU's inputs differ by the summation order of its norms and by its Krylov
solve (+-1 iteration).

newton_ew_ref runs tests/newton_ls_ref.py:newton_ls_ref -- `basic` and `bt` alike -- on a stand-in engine whose linear_solve
chooses eta from the right-hand side it is handed (||F_k|| = ||b||, which is the norm newton_ls_ref itself keeps) and overrides
engine.opts["ksp_rtol"] for that one solve.
"""
import math

import numpy as np

import newton_ls_ref as L

DAY = 86400.0
ALPHA = (1.0 + math.sqrt(5.0))/2.0
DEFAULTS = dict(rtol0=0.3, rtolmax=0.9, gamma=1.0, alpha=ALPHA, alpha2=ALPHA, threshold=0.1)
# the branches one choice took (tp_ew.hpp: EW_*)
FIRST, SAFE_TESTED, SAFE_RAISED, CAPPED, FLOORED = 1, 2, 4, 8, 16


def next_rtol(version, k, fnorm, fnorm_last, lresid_last, rtol_last, ksp_rtol, rtol0=0.3, rtolmax=0.9, gamma=1.0, alpha=ALPHA,
              alpha2=ALPHA, threshold=0.1):
    """(eta_k, flags): the chooser.  fnorm_last, lresid_last, rtol_last are not read for k == 0."""
    fl = 0
    if k == 0:
        eta = rtol0
        fl |= FIRST
    else:
        if version == 1:
            eta = abs(fnorm - lresid_last)/fnorm_last
            s = math.pow(rtol_last, alpha2)
        else:
            eta = gamma*math.pow(fnorm/fnorm_last, alpha)
            s = gamma*math.pow(rtol_last, alpha)
        if s > threshold:
            fl |= SAFE_TESTED
            if s > eta:
                eta = s
                fl |= SAFE_RAISED
    if not eta <= rtolmax:
        eta = rtolmax
        fl |= CAPPED
    if eta < ksp_rtol:
        eta = ksp_rtol
        fl |= FLOORED
    return eta, fl


def ew_params(opts):
    """The chooser's keyword arguments from engine options (ew_rtol0 ... ew_threshold; missing keys at their defaults)."""
    return {k: float(opts.get("ew_" + k, d)) for k, d in DEFAULTS.items()}


def ew_version(opts):
    v = opts.get("ksp_ew", False)
    return 2 if v is True else int(v or 0)


class _EwSolves:
    """Stand-in engine for newton_ls_ref: the oracle engine's problem, options and state, and a linear_solve that runs under
    the Eisenstat-Walker tolerance.  eta_scale multiplies the tolerance each solve RUNS at (the sensitivity run halves it); the
    chooser keeps seeing its own eta_{k-1}."""

    def __init__(self, engine, version, params, eta_scale):
        self.engine, self.version, self.params, self.eta_scale = engine, version, params, eta_scale
        self.opts, self.prob, self.u = engine.opts, engine.prob, engine.u
        self.rtol, self.fnorm, self.lresid, self.kits, self.kreason, self.flags = [], [], [], [], [], []

    def linear_solve(self, J, Sm, F):
        fnorm = math.sqrt(L._sumsq(F))
        k = len(self.rtol)
        last = (self.fnorm[-1], self.lresid[-1], self.rtol[-1]) if k else (0.0, 0.0, 0.0)
        floor = self.opts["ksp_rtol"]
        eta, fl = next_rtol(self.version, k, fnorm, last[0], last[1], last[2], floor, **self.params)
        self.opts["ksp_rtol"] = eta*self.eta_scale
        try:
            dx, kits, kreason, hist = self.engine.linear_solve(J, Sm, F)
        finally:
            self.opts["ksp_rtol"] = floor
        self.rtol.append(eta); self.fnorm.append(fnorm); self.lresid.append(float(hist[-1]))
        self.kits.append(int(kits)); self.kreason.append(int(kreason)); self.flags.append(fl)
        return dx, kits, kreason, hist


def newton_ew_ref(engine, version=2, eta_scale=1.0, params=None, **ls):
    """One nonlinear solve from engine.u under Eisenstat-Walker `version` (0: every solve at ksp_rtol, the plain newton_ls_ref).
    ls: the line-search arguments of newton_ls_ref (linesearch="basic" unless given).  Returns newton_ls_ref's dict plus, per
    linear solve, ew = dict(rtol, fnorm, lresid, kits, kreason, flags) and safeguarded = how often the safeguard raised eta."""
    ls = {"linesearch": "basic", **ls}
    if not version:
        r = L.newton_ls_ref(engine, **ls)
        r.update(ew=dict(rtol=[], fnorm=[], lresid=[], kits=[], kreason=[], flags=[]), safeguarded=0)
        return r
    st = _EwSolves(engine, version, dict(DEFAULTS, **(params or {})), eta_scale)
    r = L.newton_ls_ref(st, **ls)
    r["ew"] = dict(rtol=st.rtol, fnorm=st.fnorm, lresid=st.lresid, kits=st.kits, kreason=st.kreason, flags=st.flags)
    r["safeguarded"] = sum(1 for f in st.flags if f & SAFE_RAISED)
    return r


def make_ew_oracle_engine():
    OracleEngine = L._oracle_engine()

    class EwOracleEngine(OracleEngine):
        """OracleEngine whose newton_solve honours the engine options ksp_ew / ew_* and linesearch / ls_*: the CPU stand-in of
        the GPU engine for the host time loop (_engine_factory)."""

        def newton_solve(self):
            r = newton_ew_ref(self, version=ew_version(self.opts), params=ew_params(self.opts), **L._ls_kwargs(self.opts))
            self.u = r["u"]
            self.last = dict(nits=r["nits"], lits=r["lits"], reason=r["reason"], fnorm=r["fnorm"], fnorm0=r["fnorm0"],
                             history=[r["fnorm0"]] + r["hist"], ls_trials=r["evaluations"], ew_rtol=list(r["ew"]["rtol"]))
            return self.last
    return EwOracleEngine


def __getattr__(name):              # built on first use: importing this module does not import the oracle
    if name == "EwOracleEngine":
        cls = make_ew_oracle_engine()
        globals()["EwOracleEngine"] = cls
        return cls
    raise AttributeError(name)


# ---- the inputs of tests/test_ew_host.py and tests/test_gpu_ew.py ---------------------------------------------------------------
# The ramp: eight time steps from the cold uniform state, the old state set to the converged state after each step.
RAMP_DT = (0.001, 0.002, 0.004, 0.008, 0.016, 0.03, 0.03, 0.03)            # days
RAMP_OPTS = dict(pc="cptr", ksp_rtol=1e-8)
C3_OPTS = dict(pc="cptr", ksp_rtol=1e-8)                                   # c3_spe10_2d(12, 16): the first two ramp steps


def ramp_case():
    import cases
    return cases.c4_spe10_3d(8, 10, 6)


def c3_case():
    import cases
    return cases.c3_spe10_2d(12, 16)


def run_ramp(engine, u0, dts, solve):
    """The ramp on any engine (oracle or GPU): state = old state = u0, then per dt: set_dt, solve(engine) -> dict with nits, lits,
    reason; old <- state.  Stops at the first step that does not converge.  Returns the list of per-step dicts."""
    engine.set_state(u0)
    engine.set_old(u0)
    out = []
    for dt in dts:
        engine.set_dt(dt*DAY)
        r = solve(engine)
        out.append(r)
        if r["reason"] <= 0:
            break
        engine.set_old(None)
    return out


def ref_ramp(version, eta_scale=1.0, case=ramp_case, opts=RAMP_OPTS, dts=RAMP_DT, params=None, **ls):
    """The reference on the ramp: (per-step results of newton_ew_ref, final state)."""
    spec, u0, *_ = case()
    eng = L._oracle_engine()(spec, opts)

    def solve(e):
        r = newton_ew_ref(e, version=version, eta_scale=eta_scale, params=params, **ls)
        e.u = r["u"]
        return r
    steps = run_ramp(eng, u0, dts, solve)
    return steps, eng.get_state()


def state_diff(a, b):
    """Per-field difference in the norms of tests/test_gpu_parity.py: relative 2-norm for p and T, max abs for S_o."""
    a, b = np.asarray(a), np.asarray(b)
    d = [float(np.linalg.norm((a[f] - b[f]).ravel())/max(np.linalg.norm(b[f].ravel()), 1e-300)) for f in range(2)]
    if a.shape[0] > 2:
        d.append(float(np.abs(a[2] - b[2]).max()))
    return d


# what the reference gives on the ramp: Newton iterations per step (every step converges with reason 3); Krylov totals 191 (fixed),
# 92 (version 1), 94 (version 2); the safeguard raises eta_1 of every step (0.3^alpha = 0.143 > 0.1)
EXPECT_NITS = {"fixed": [4, 3, 3, 3, 3, 3, 3, 3], "v1": [4, 4, 4, 4, 4, 4, 4, 4], "v2": [4, 4, 4, 4, 5, 5, 4, 5]}
C3_EXPECT_NITS = [4, 5]                 # version 2 on c3's two steps; eta_1 of the second step is 0.397 > rtol0 (the residual grew)
# The bt input: input A of newton_ls_ref (c3 12 x 16 cold at dt 0.1 d, four shortened steps) at snes_rtol 1e-10.  A as it stands
# (snes_rtol 1e-6) and at 1e-8 was measured and REPLACED: under Eisenstat-Walker its last linear solves run at eta 0.15 .. 0.9, the
# solve stops wherever the residual first passes snes_rtol ||F_0||, and the final pressure then moves by 2.3e-8 (1e-6) or 8.5e-10
# (1e-8) when every eta is halved -- above the ramp's floor; at 1e-10 the halved run still ends early, on snes_stol, with the same
# 8.5e-10.  With snes_rtol 1e-10 and snes_stol 0 every run ends on the residual, in the quadratic regime.
# Input B (c4 at dt 0.02 d) moves by 7e-7 and was not used.
BT_OPTS = dict(L.A_OPTS, snes_rtol=1e-10, snes_stol=0.0)
BT_DT = 0.1
BT_EXPECT_TRIALS = [2, 2, 3, 4, 4, 1, 1, 1, 1, 1, 1, 1]           # version 2; 12 iterations, the smallest Armijo margin 0.031

# Sensitivity floor of the ramp's final state (floor 1): per field, the larger of |EW reference - fixed reference| and |EW reference -
# the EW reference with every eta halved|, over versions 1 and 2; the GPU tolerance is 10 x the floor (the project's habit,
# newton_ls_ref.PARITY_TOL) and may not exceed the 1e-8 of the existing Newton parity tests.  tests/test_ew_host.py re-measures it;
# profiles/ew_parity.txt holds the figures.
# measured (p, T, S_o): version 1 against fixed 4.21e-11, 3.48e-14, 5.48e-10, against halved 2.57e-12, 1.04e-14, 7.27e-10;
#                        version 2 against fixed 6.34e-11, 1.10e-13, 5.48e-10, against halved 4.44e-11, 1.00e-13, 6.21e-12
FLOOR1 = (6.4e-11, 1.2e-13, 7.3e-10)
PARITY_TOL = tuple(10*f for f in FLOOR1)
