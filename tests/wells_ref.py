"""Inputs and independent checks for the completed wells.  The reference itself is ``oracle.tpfa.Problem`` with
``spec["wells"]`` (or its ``wells`` argument), the wells being its component ``oracle.wells.Wells``."""
import numpy as np

from oracle.tpfa import Problem
from oracle.wells import solve_bhp  # noqa: F401  (tests take it from here)


def solve_bhp_brute(kind, a, th, Q):
    """The rate-mode bhp by trying every prefix of the perforations sorted by threshold: the open set is the m perforations
    with the most favourable thresholds, for the one m whose bhp shuts exactly the others."""
    sgn = 1.0 if kind == "prod" else -1.0
    order = np.argsort(-sgn*th, kind="stable")
    found = []
    for m in range(1, len(a) + 1):
        sel = order[:m]
        sa = a[sel].sum()
        if not sa > 0.0:
            continue
        bhp = (np.sum(a[sel]*th[sel]) - sgn*Q)/sa
        opn = sgn*(th - bhp) > 0.0
        if opn.sum() == m and opn[sel].all():
            found.append((bhp, opn))
    return found


def wells_problem(spec, hs=None, boundary=None, satfn=None, wells=None):
    """The reference with wells over the grid / sides / saturation functions asked for (spec's own keys when None)."""
    return Problem(spec, hs=hs, boundary=boundary, satfn=satfn, wells=wells)


def wells_oracle(spec, opts, wells=None):
    """An OracleEngine on the problem with wells (its linear solves apply J + sum_w c_w b_w^T while the preconditioner is set up
    on J alone) that honours the engine options linesearch ("bt") and ksp ("bcgs")."""
    from newton_ls_ref import make_ls_oracle_engine

    class WellsOracle(make_ls_oracle_engine()):
        def linear_solve(self, J, Sm, F):
            o = self.opts
            if o.get("ksp", "fgmres") != "bcgs":
                return super().linear_solve(J, Sm, F)
            from bcgs_ref import bcgs_ref
            self.pc.setup(J, Sm)
            return bcgs_ref(self.operator(J), self.pc.apply, F, rtol=o["ksp_rtol"], atol=o["ksp_atol"], maxit=o["ksp_max_it"])

        def well_info(self):
            return self.prob.well_state(self.u)

        def set_well_control(self, i, rate=None, bhp=None, shut=None):
            w = self.prob.wells[i]
            w.update({k: v for k, v in (("rate", rate), ("bhp", bhp), ("shut", shut)) if v is not None})
    return WellsOracle(spec if wells is None else dict(spec, wells=wells), opts)


# ---- wells for the tests ------------------------------------------------------------------------------------------------------
def peaceman(Ka, Kb, Da, Db, L, rw=0.1, skin=0.0):
    ro = 0.28*np.sqrt(np.sqrt(Kb/Ka)*Da**2 + np.sqrt(Ka/Kb)*Db**2)/((Kb/Ka)**0.25 + (Ka/Kb)**0.25)
    return 2.0*np.pi*L*np.sqrt(Ka*Kb)/(np.log(ro/rw) + skin)


def line_cells(spec, axis, fixed, lo=0, hi=None):
    """Flat internal cells of the line along internal axis `axis` at the other two indices `fixed` (ascending axis order)."""
    n = tuple(int(v) for v in spec["n"])
    hi = n[axis] if hi is None else hi
    others = [d for d in range(3) if d != axis]
    out = []
    for i in range(lo, hi):
        idx = [0, 0, 0]
        idx[axis] = i
        idx[others[0]], idx[others[1]] = fixed
        out.append(idx[0] + n[0]*(idx[1] + n[1]*idx[2]))
    return np.array(out, dtype=np.int64)


def make_well(spec, name, kind, cells, axis, rate, bhp, hs=None, radius=None):
    """A spec["wells"] entry on `cells` (a line along internal `axis`): WI from the cells' own widths and permeabilities across
    the axis, elevations from the centres along the gravity axis."""
    n = tuple(int(v) for v in spec["n"])
    cells = np.asarray(cells, dtype=np.int64)
    idx = [cells % n[0], (cells//n[0]) % n[1], cells//(n[0]*n[1])]
    w = [np.asarray(hs[d], dtype=float) if hs is not None else np.full(n[d], float(spec["h"][d])) for d in range(3)]
    ca, cb = [d for d in range(3) if d != axis]
    K = [np.asarray(k, dtype=float).reshape(-1) for k in spec["K"]]
    Ka, Kb = K[ca][cells], K[cb][cells]
    if spec["dim"] == 2:                  # unit thickness: the one cross permeability in both cross directions
        Ka = Kb = K[ca if ca < 2 else cb][cells]
    if radius is None:                    # (a graded grid of the tests has cells a few centimetres wide: a thinner bore there)
        radius = 0.1 if hs is None else 1e-3
    WI = peaceman(Ka, Kb, w[ca][idx[ca]], w[cb][idx[cb]], w[axis][idx[axis]], radius)
    assert np.all(WI > 0.0), "Peaceman's radius of a perforated cell is not larger than the well's"
    g = int(spec["gaxis"])
    z = (np.cumsum(w[g]) - 0.5*w[g])[idx[g]] if g >= 0 else np.zeros(cells.size)
    return {"name": name, "kind": kind, "rate": float(rate), "bhp": float(bhp), "z_ref": float(z.max()), "shut": False,
            "cells": cells, "WI": WI, "z": z}


def tune_wells(prob, u, wells, plan):
    """Sets rate and bhp limit of every well from the thresholds at u so that the well ends in the planned state.  plan[name]:
    ("rate", f): a rate that puts the bhp the fraction f of the threshold spread beyond the all-open mean (f > 0 closes the
    perforations on the wrong side: two or more rounds), the limit far away; ("bhp", f): the same rate with the limit placed
    the fraction f of the spread inside the thresholds, so that the rate-mode bhp violates it."""
    prob.well.wells = [dict(w) for w in wells]
    for w in prob.wells:
        w["rate"], w["bhp"] = 1.0, (0.0 if w["kind"] == "prod" else 1e3)
    prob.set_old(u)
    st = prob.well_state(u)
    out = []
    for w, s in zip(wells, st):
        a, th = np.real(s["a"]), np.real(s["th"])
        sgn = 1.0 if w["kind"] == "prod" else -1.0
        spread = max(th.max() - th.min(), 0.2)
        mode, f = plan[w["name"]]
        mean = np.sum(a*th)/np.sum(a)
        Q = f*spread*np.sum(a)                        # all-open bhp = mean -+ f spread
        w = dict(w, rate=float(Q))
        if mode == "rate":
            w["bhp"] = float(mean - sgn*100.0)
        else:
            w["bhp"] = float(mean - sgn*0.25*f*spread)
        out.append(w)
    prob.well.wells = [dict(w) for w in out]
    prob.set_old(u)
    return out
