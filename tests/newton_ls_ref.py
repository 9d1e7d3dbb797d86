"""Newton with the Armijo backtracking line search in numpy: the reference of the GPU driver (newton() / ls_backtrack in
thermalporous_amd/csrc/tp_solver.hip, tp_options.ls_kind = 1), built on the oracle's residual, Jacobian and linear solve.

One Newton iteration from iterate u0 with F0 = F(u0), f0 = ||F0||^2 / 2 and the Krylov correction dx:

    ynorm = ||dx||, m_f = max|dx_f|;  lambda = min(1, maxstep/ynorm, min_f max_change[f]/m_f)     (caps <= 0: off)
    slope g0 = -||F0||^2          (exact for an exact linear solve, within ksp_rtol otherwise; no mat-vec is spent on it)
    trial t = 1, 2, ...:  u = u0 - lambda dx;  phi = ||F(u)||^2
       accept if phi is finite and phi <= (1 - 2 alpha lambda) ||F0||^2
       t == max_it: the search failed
       phi not finite: lambda <- lambda/2 and the interpolation history is forgotten
       else lambda <- next_lambda(...): minimiser of the quadratic (order 2, or one finite rejected trial) or of the
            Dennis-Schnabel cubic (order 3, two finite rejected trials; lambda/2 on a negative discriminant), clamped to
            [0.1, 0.5] lambda
       lambda < minlambda (absolute): the search failed
    convergence tests as the basic solver's, with snorm = lambda ynorm
    failed search: u <- u0, reason -6 (SNES_DIVERGED_LINE_SEARCH), fnorm that of u0

Every scalar decision is written operation by operation as the C++ writes it, so the two choosers return the same bits from
the same inputs; the GPU's inputs differ by the summation order of its norms and by its Krylov solve (+-1 iteration).
"""
import math

import numpy as np

SNES_DIVERGED_LINE_SEARCH = -6
DAY = 86400.0


def next_lambda(order, g0, f0, hist):
    """The next trial length after a finite rejected trial.  hist: the finite rejected trials [(lambda, phi = ||F||^2), ...]
    since the start or the last non-finite trial, the current one last; f = phi/2."""
    lam, phi = hist[-1]
    f = 0.5*phi
    if order == 2 or len(hist) < 2:
        nl = -g0*lam*lam/(2.0*(f - f0 - g0*lam))
    else:
        lam_p, phi_p = hist[-2]
        fp = 0.5*phi_p
        t1 = f - f0 - lam*g0
        t2 = fp - f0 - lam_p*g0
        a = (t1/(lam*lam) - t2/(lam_p*lam_p))/(lam - lam_p)
        b = (-lam_p*t1/(lam*lam) + lam*t2/(lam_p*lam_p))/(lam - lam_p)
        d = b*b - 3.0*a*g0
        if d < 0.0:
            nl = 0.5*lam
        elif a == 0.0:
            nl = -g0/(2.0*b)
        else:
            nl = (-b + math.sqrt(d))/(3.0*a)
    if not nl >= 0.1*lam:
        nl = 0.1*lam
    if nl > 0.5*lam:
        nl = 0.5*lam
    return nl


def _sumsq(a):
    return float(np.sum(a.ravel()*a.ravel()))


def newton_ls_ref(engine, linesearch="bt", order=3, alpha=1e-4, max_it=40, maxstep=1e8, minlambda=1e-12, max_change=None,
                  ksp_rtol_factor=1.0):
    """One nonlinear solve from engine.u.  ksp_rtol_factor scales the oracle's ksp_rtol (the sensitivity floor solves every
    linear system 100 times tighter).  Returns a dict: reason, nits, lits, fnorm0, fnorm, lam / trials / hist (per
    iteration: accepted lambda, trials, ||F|| after it), first (first trial length of every search), evaluations, nonfinite
    [(iteration, lambda), ...], margin (smallest |phi / ((1 - 2 alpha lambda) ||F0||^2) - 1| over the finite trials), u."""
    o = dict(engine.opts)
    prob = engine.prob
    want_schur = o["pc"] in ("cptr", "fieldsplit_cd")
    rtol0 = engine.opts["ksp_rtol"]
    u = engine.u.copy()
    res = dict(lam=[], trials=[], hist=[], first=[], nonfinite=[], evaluations=0, margin=float("inf"))
    with np.errstate(all="ignore"):
        F = prob.residual(u)
        fnorm = math.sqrt(_sumsq(F))
        fnorm0 = fnorm
        nits = lits = reason = 0
        if not np.isfinite(fnorm):
            reason = -4
        elif fnorm < o["snes_atol"]:
            reason = 2
        while reason == 0:
            if nits >= o["snes_max_it"]:
                reason = -5
                break
            out = prob.jacobian(u, want_schur=want_schur)
            J, Sm = out if want_schur else (out, None)
            engine.opts["ksp_rtol"] = rtol0*ksp_rtol_factor
            try:
                dx, kits, kreason, _ = engine.linear_solve(J, Sm, F)
            finally:
                engine.opts["ksp_rtol"] = rtol0
            lits += kits
            if kreason < 0:
                reason = -3
                break
            if linesearch == "basic":
                u = u - dx
                F = prob.residual(u)
                fnorm = math.sqrt(_sumsq(F))
                nits += 1
                res["hist"].append(fnorm)
                snorm, xnorm = math.sqrt(_sumsq(dx)), math.sqrt(_sumsq(u))
                if not np.isfinite(fnorm):
                    reason = -4
                elif fnorm < o["snes_atol"]:
                    reason = 2
                elif fnorm <= o["snes_rtol"]*fnorm0:
                    reason = 3
                elif snorm < o["snes_stol"]*xnorm:
                    reason = 4
                continue
            ynorm = math.sqrt(_sumsq(dx))
            lam = 1.0
            if maxstep/ynorm < lam:
                lam = maxstep/ynorm
            for f in range(dx.shape[0]):
                cap = max_change[f] if max_change is not None else 0.0
                if cap > 0.0:
                    m = float(np.max(np.abs(dx[f])))
                    if cap/m < lam:
                        lam = cap/m
            res["first"].append(lam)
            ff = fnorm*fnorm
            f0, g0 = 0.5*ff, -ff
            hist = []
            ok = False
            t = 0
            while np.isfinite(ynorm):
                t += 1
                ut = u - lam*dx
                Ft = prob.residual(ut)
                phi = _sumsq(Ft)
                res["evaluations"] += 1
                finite = bool(np.isfinite(phi))
                if finite:
                    res["margin"] = min(res["margin"], abs(phi/((1.0 - 2.0*alpha*lam)*ff) - 1.0))
                else:
                    res["nonfinite"].append((nits, lam))
                if finite and phi <= (1.0 - 2.0*alpha*lam)*ff:
                    ok = True
                    break
                if t >= max_it:
                    break
                if not finite:
                    lam = 0.5*lam
                    hist = []
                else:
                    hist = (hist + [(lam, phi)])[-2:]
                    lam = next_lambda(order, g0, f0, hist)
                if lam < minlambda:
                    break
            if not ok:
                reason = SNES_DIVERGED_LINE_SEARCH
                break
            u, F = ut, Ft
            fnorm = math.sqrt(phi)
            nits += 1
            res["lam"].append(lam)
            res["trials"].append(t)
            res["hist"].append(fnorm)
            snorm, xnorm = lam*ynorm, math.sqrt(_sumsq(u))
            if fnorm < o["snes_atol"]:
                reason = 2
            elif fnorm <= o["snes_rtol"]*fnorm0:
                reason = 3
            elif snorm < o["snes_stol"]*xnorm:
                reason = 4
    res.update(reason=reason, nits=nits, lits=lits, fnorm0=fnorm0, fnorm=fnorm, u=u)
    return res


def _ls_kwargs(opts):
    """The search's arguments from engine options (the keys of thermalporous_amd.engine.DEFAULT_OPTS)."""
    return dict(linesearch=opts.get("linesearch", "basic"), order=opts.get("ls_order", 3), alpha=opts.get("ls_alpha", 1e-4),
                max_it=opts.get("ls_max_it", 40), maxstep=opts.get("ls_maxstep", 1e8), minlambda=opts.get("ls_minlambda", 1e-12),
                max_change=opts.get("ls_max_change"))


def _oracle_engine():
    from oracle.engine import OracleEngine
    return OracleEngine


def make_ls_oracle_engine():
    OracleEngine = _oracle_engine()

    class LsOracleEngine(OracleEngine):
        """OracleEngine whose newton_solve honours the engine options linesearch / ls_*: the CPU stand-in of the GPU engine for
        the host time loop (_engine_factory)."""

        def newton_solve(self):
            r = newton_ls_ref(self, **_ls_kwargs(self.opts))
            self.u = r["u"]
            self.last = dict(nits=r["nits"], lits=r["lits"], reason=r["reason"], fnorm=r["fnorm"], fnorm0=r["fnorm0"],
                             history=[r["fnorm0"]] + r["hist"], ls_trials=r["evaluations"])
            return self.last
    return LsOracleEngine


def __getattr__(name):              # LsOracleEngine is built on first use: importing this module does not import the oracle
    if name == "LsOracleEngine":
        cls = make_ls_oracle_engine()
        globals()["LsOracleEngine"] = cls
        return cls
    raise AttributeError(name)


# ---- the inputs of tests/test_newton_ls_host.py and tests/test_gpu_newton_ls.py -----------------------------------------------
# All cold: state = old state = the case's uniform initial state.
def _builders():
    import cases
    return {"c3": lambda: cases.c3_spe10_2d(12, 16, 2), "c4": lambda: cases.c4_spe10_3d(8, 10, 6), "c1": lambda: cases.c1_homogeneous(10, 2)}


# Two inputs were REPLACED after measuring them on the reference, because they miss the sensitivity condition below:
#   A as first proposed (snes_rtol 1e-8) converges in 7 iterations, 14 evaluations, and its 7th ||F|| (5e-9 .. 7e-9 against
#     ||F0|| = 5e5) is the rounding noise of the residual evaluation: it changes by 9 % (order 2) and 1 % (order 3) when the linear
#     systems are solved 100 times tighter.  A here stops one iteration earlier (snes_rtol 1e-6: 6 iterations, 13 evaluations,
#     the same lambdas), where the last ||F|| changes by 1.3e-7.
#   B as first proposed (dt 0.1 d, ksp_rtol 1e-7): the oracle's linear solve does not reach 1e-9 (nor 1e-10) in 600 iterations
#     at that time step, so its floor cannot be measured.  B here is the same grid at dt 0.02 d and ksp_rtol 1e-9: basic fails
#     (-3 after 7 iterations), bt converges in 13 iterations, 20 evaluations.
A_OPTS = dict(pc="cptr", snes_max_it=25, ksp_rtol=1e-10, snes_rtol=1e-6)
B_OPTS = dict(pc="cptr", snes_max_it=25, ksp_rtol=1e-9)
C_OPTS = dict(pc="cpr")
# (name, case, engine options, dt in days, search options): the parity inputs
PARITY = [("A_order2", "c3", A_OPTS, 0.1, dict(ls_order=2)), ("A_order3", "c3", A_OPTS, 0.1, dict(ls_order=3)),
          ("B", "c4", B_OPTS, 0.02, dict(ls_order=3))]
# what the reference gives on them: (reason, nits, trials per iteration) under bt, (reason, nits) under basic
EXPECT = {"A_order2": ((3, 6, [2, 2, 3, 4, 1, 1]), (-3, 21)), "A_order3": ((3, 6, [2, 2, 3, 4, 1, 1]), (-3, 21)),
          "B": ((3, 13, [1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1]), (-3, 7))}
C_INPUT = ("C", "c1", C_OPTS, 1.0, dict(ls_order=3))
D_DT = 1.0                          # input D: A's case at dt 1 d, one basic iteration, then bt with snes_max_it 2
# Every finite Armijo decision of a parity input lies at least this far (relative) from its threshold
MARGIN_MIN = 1e-3
# Sensitivity floor of the parity inputs: the largest relative change of an accepted lambda or a history ||F|| when the reference
# solves every linear system to ksp_rtol/100 (sensitivity_floor below); the tolerance of the GPU comparison is 10 x the floor,
# as bcgs_ref.PARITY_TOL is (profiles/newton_ls_parity.txt; tests/test_newton_ls_host.py re-measures it)
FLOOR_MAX = 1e-4
# measured: A_order2 1.33e-7, A_order3 2.2e-8, B 2.874e-5 (its 12th ||F||, 1.49e2 after 1.97e4: the linear residual left at
# ksp_rtol 1e-9 shows once the nonlinear residual has dropped by two orders in one step)
PARITY_FLOOR = 2.874e-5
PARITY_TOL = 2.9e-4
# smallest decision margins measured: A_order2 0.0552, A_order3 0.0632, B 0.190, D 0.114, F 0.0995
# input F: A (order 3) with a cap on the change of S_o of half the first iteration's max|dx_S| = 0.03330182051959105 (measured
# on the reference): the first trial length is 0.5, the search then takes 7 iterations and 10 evaluations.  It stops at
# snes_rtol 1e-5: at 1e-6 it needs an 8th iteration whose ||F|| = 8.6e-8 is rounding noise (it changes by 1.2 % with the linear
# systems solved 100 times tighter; the 7 before it change by at most 3.5e-9)
F_CAP = (0.0, 0.0, 0.5*0.03330182051959105)
F_OPTS = dict(A_OPTS, snes_rtol=1e-5)
F_EXPECT = (3, 7, [1, 1, 1, 2, 3, 1, 1])
# input D: one basic iteration ends with reason -5 at a finite state; the bt solve from there (snes_max_it 2) ends with -5 after
# lambda = 0.5 and 0.0625 exactly, 7 evaluations, 5 of them non-finite (iteration 0 at lambda 1; iteration 1 at 1, 0.5, 0.25, 0.125)
D_EXPECT = dict(reason=-5, lam=[0.5, 0.0625], trials=[2, 5], evaluations=7,
                nonfinite=[(0, 1.0), (1, 1.0), (1, 0.5), (1, 0.25), (1, 0.125)])


def cold_engine(case, opts, dt_days, cls=None):
    """An oracle engine on `case` at its uniform initial state (= old state) with time step dt: (spec, u0, engine)."""
    spec, u0, *_ = _builders()[case]()
    eng = (cls or _oracle_engine())(spec, opts)
    eng.set_state(u0)
    eng.set_old(u0)
    eng.set_dt(dt_days*DAY)
    return spec, u0, eng


def run_ref(case, opts, dt_days, ls, linesearch="bt", ksp_rtol_factor=1.0):
    spec, u0, eng = cold_engine(case, opts, dt_days)
    kw = _ls_kwargs({"linesearch": linesearch, **ls})
    return spec, u0, newton_ls_ref(eng, ksp_rtol_factor=ksp_rtol_factor, **kw)


def run_ref_D(order=3):
    """Input D: (spec, u0, u1 = the state after one basic iteration, result of the bt solve with snes_max_it 2 from u1)."""
    spec, u0, eng = cold_engine("c3", {**A_OPTS, "snes_max_it": 1}, D_DT)
    first = newton_ls_ref(eng, linesearch="basic")
    eng.u = first["u"]
    eng.opts["snes_max_it"] = 2
    return spec, u0, first, newton_ls_ref(eng, linesearch="bt", order=order)


def sensitivity_floor(case, opts, dt_days, ls):
    """(floor, result at ksp_rtol, result at ksp_rtol/100)."""
    _, _, a = run_ref(case, opts, dt_days, ls)
    _, _, b = run_ref(case, opts, dt_days, ls, ksp_rtol_factor=0.01)
    if a["trials"] != b["trials"] or a["reason"] != b["reason"]:
        return float("inf"), a, b
    dev = [abs(x - y)/abs(x) for x, y in zip(a["lam"], b["lam"])] + [abs(x - y)/abs(x) for x, y in zip(a["hist"], b["hist"])]
    return max(dev), a, b
