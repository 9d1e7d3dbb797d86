"""CPU reference of the completed wells: ``WellsMixin`` adds them to the oracle's residual, written in numpy
from the definition and not through the library.

A well (an entry of ``spec["wells"]``: kind, rate Q, bhp limit, z_ref, and per perforation the flat internal cell, WI and the
elevation z) has, with u_k the state of its k-th perforated cell,
    a_k = WI_k lambda_k(u_k),   theta_k = p_k - rho_w g (z_ref - z_k),   q_k = -a_k (theta_k - bhp) where open, else 0,
open meaning theta_k > bhp for a producer and theta_k < bhp for an injector.  In rate mode bhp solves sum_k q_k = -+Q by
active-set rounds (``solve_bhp``); in BHP mode (the limit violated, or nothing mobile open) bhp is the limit.  rho_w is frozen
over a time step: ``set_old`` computes it.  A perforation adds G(u_k) q_k, what a source entry of its kind adds for the rate q_k
with weight 1.

Every decision (open / closed, the mode) is taken on real parts, so a complex perturbation differentiates the branch in force.
``jacobian`` freezes the wells' bhp at its real value and lets the class behind it in the MRO do what it does (its own formulas,
or the complex step of ``residual`` for the saturation-function classes), then adds the wells' part of the diagonal blocks and of
S~ by complex steps of their contribution; the factors c = dR/dbhp and b = dbhp/du are complex steps too.  The exact Jacobian is
J + sum_w c_w b_w^T, which ``rank1`` applies; a well of one perforation has its c b^T folded into the diagonal block and zero
factors, as the library does it."""
import numpy as np

from oracle import closures as cl
from oracle import linalg as la
from oracle.tpfa import Problem

HSTEP = 1e-30


def solve_bhp(kind, a, th, Q, limit):
    """Active-set rounds on (possibly complex) a, theta.  Returns bhp, mode ("rate" | "bhp"), the open mask, the rounds and
    sum_open a.  Start with all open; bhp = (sum_open a theta -+ Q)/sum_open a; close what it shuts; repeat until no change."""
    sgn = 1.0 if kind == "prod" else -1.0
    a, th = np.asarray(a), np.asarray(th)
    opn = np.ones(a.shape, dtype=bool)
    rounds, mode, bhp, sa = 0, "bhp", limit, 0.0
    while True:
        sa = np.sum(a[opn])
        rounds += 1
        if not (sa.real > 0.0):
            mode = "bhp"
            break
        bhp = (np.sum(a[opn]*th[opn]) - sgn*Q)/sa
        new = opn & (sgn*(th.real - bhp.real) > 0.0)
        mode = "rate"
        if new.sum() == opn.sum():
            break
        opn = new
    if mode == "rate" and (bhp.real < limit if kind == "prod" else bhp.real > limit):
        mode = "bhp"
    if mode == "bhp":
        bhp = limit + 0.0*np.sum(th)*0.0
        opn = sgn*(th.real - limit) > 0.0
        sa = np.sum(a[opn]) if opn.any() else 0.0
    return bhp, mode, opn, rounds, sa


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


class WellsMixin:
    """The wells, for any of Problem, BcProblem, GradedProblem and the saturation-function classes behind it in the MRO."""

    def __init__(self, spec, *args, wells=None, **kw):
        super().__init__(spec, *args, **kw)
        self.wells = [dict(w) for w in (spec.get("wells") or [] if wells is None else wells)]
        for w in self.wells:
            w["cells"] = np.asarray(w["cells"], dtype=np.int64)
            w["WI"], w["z"] = np.asarray(w["WI"], dtype=float), np.asarray(w["z"], dtype=float)
            if w.get("z_ref") is None:
                w["z_ref"] = float(w["z"].max())
        self.rho_w = [0.0]*len(self.wells)
        self._frozen = None
        self.last_wells = []
        self.last_factors = []

    # ---------------------------------------------------------------- closures of one well's perforations
    def _mob(self, S):
        if hasattr(self, "sat"):
            from satfn_ref import curves
            kr_o, kr_w, _ = curves(self.sat, S)
            return kr_o, kr_w
        return S, 1.0 - S

    def _lam_G(self, kind, p, T, S, Tx):
        """lambda and G (b rows) at the perforated cells; fw, fo: the phase split of the rate."""
        prm = self.prm
        API, Ti = prm["API"], prm["T_inj"]
        mo = cl.oil_mu(T, API)[0]
        one = 1.0 + 0.0*p
        if self.nph == 1:
            lam = 1.0/mo
            if kind == "prod":
                ro = cl.oil_rho(p, T, API)[0]
                return lam, [self.w0*ro, ro*prm["c_v_o"]*Tx], 0.0*one, one
            roi = cl.oil_rho(p, Ti + 0.0*T, API)[0]
            return lam, [self.w0*roi, roi*(prm["c_v_o"]*Ti)], 0.0*one, one
        mw = cl.water_mu(T)[0]
        cw, co = prm["c_v_w"], prm["c_v_o"]
        if kind == "prod":
            kr_o, kr_w = self._mob(S)
            lo, lw = kr_o/mo, kr_w/mw
            lam = lo + lw
            safe = np.where(lam.real > 0.0, lam, 1.0)
            gw, go = lw/safe, lo/safe
            ro, rw = cl.oil_rho(p, T, API)[0], cl.water_rho(p, T)[0]
            m = rw*gw*cw + ro*go*co
            dead = ~(lam.real > 0.0)
            G = [np.where(dead, 0.0, self.w0*m), np.where(dead, 0.0, m*Tx), np.where(dead, 0.0, self.w2*ro*go)]
            return np.where(dead, 0.0, lam), G, gw, go
        rwi = cl.water_rho(p, Ti + 0.0*T)[0]
        return 1.0/mw, [self.w0*cw*rwi, rwi*(cw*Ti), 0.0*one], one, 0.0*one

    def _head(self, i):
        w = self.wells[i]
        if self.gaxis < 0:
            return 0.0*w["z"]
        return self.rho_w[i]*self.prm["g"]*(w["z_ref"] - w["z"])

    def set_old(self, u_old):
        super().set_old(u_old)
        u = self.as_fields(np.asarray(u_old, dtype=float))
        p, T, S = (None if x is None else x.reshape(-1) for x in self.split(u))
        prm = self.prm
        for i, w in enumerate(self.wells):
            c = w["cells"]
            if w["kind"] == "inj":
                k = int(np.argmin(np.abs(w["z"] - w["z_ref"])))
                pd = p[c[k]]
                self.rho_w[i] = float(cl.water_rho(pd, prm["T_inj"])[0] if self.nph == 2 else cl.oil_rho(pd, prm["T_inj"], prm["API"])[0])
                continue
            pc, Tc = p[c], T[c]
            mo = cl.oil_mu(Tc, prm["API"])[0]
            ro = cl.oil_rho(pc, Tc, prm["API"])[0]
            if self.nph == 1:
                num, den = np.sum(w["WI"]*ro/mo), np.sum(w["WI"]/mo)
            else:
                kr_o, kr_w = self._mob(S[c])
                lo, lw = kr_o/mo, kr_w/cl.water_mu(Tc)[0]
                num = np.sum(w["WI"]*(lo*ro + lw*cl.water_rho(pc, Tc)[0]))
                den = np.sum(w["WI"]*(lo + lw))
            self.rho_w[i] = float(num/den) if den > 0.0 else 0.0

    # ---------------------------------------------------------------- the wells' part of the residual
    def _wells_R(self, u, frozen=None, Tx=None, dbhp=0.0, record=False):
        """What the wells add to R at u (zeros elsewhere).  frozen: per well (bhp, mode, open, sa) to use instead of solving;
        dbhp: added to every rate-mode bhp (the complex step for c)."""
        u = self.as_fields(u)
        p, T, S = (None if x is None else x.reshape(-1) for x in self.split(u))
        if Tx is None:
            Tx = getattr(self, "_Tx", None)
        Txf = T if Tx is None else np.asarray(Tx).reshape(-1)
        out = np.zeros((self.b, p.size), dtype=np.result_type(u.dtype, Txf.dtype, type(dbhp)))
        rec = []
        for i, w in enumerate(self.wells):
            c = w["cells"]
            if w.get("shut") or not w["rate"] > 0.0:
                rec.append(dict(bhp=w["bhp"], mode="shut", open=np.zeros(c.size, bool), rounds=0, sa=0.0, q=np.zeros(c.size),
                                qw=np.zeros(c.size), qo=np.zeros(c.size), a=np.zeros(c.size), th=np.zeros(c.size)))
                continue
            Sc = None if S is None else S[c]
            lam, G, fw, fo = self._lam_G(w["kind"], p[c], T[c], Sc, Txf[c])
            a = w["WI"]*lam
            th = p[c] - self._head(i)
            if frozen is not None:
                bhp, mode, opn, sa = frozen[i]
                rounds = 0
            else:
                bhp, mode, opn, rounds, sa = solve_bhp(w["kind"], a, th, w["rate"], w["bhp"])
            if mode == "rate":
                bhp = bhp + dbhp
            q = np.where(opn, -a*(th - bhp), 0.0)
            for r in range(self.b):
                out[r, c] -= G[r]*q
            rec.append(dict(bhp=bhp, mode=mode, open=opn, rounds=rounds, sa=sa, q=q, qw=fw*q, qo=fo*q, a=a, th=th))
        if record:
            self.last_wells = rec
        return out.reshape((self.b,) + self.shape)

    def well_state(self, u):
        """Per well at the real state u: bhp, mode, open, rounds, sa, q, qw, qo, a, th."""
        self._wells_R(np.asarray(u, dtype=float), record=True)
        return self.last_wells

    def kink_margin(self, u):
        """The smallest |theta_k - bhp| over the perforations of the active wells, relative to the drawdown scale (the largest
        |theta_k - bhp| of the same well)."""
        m = np.inf
        for st in self.well_state(u):
            if st["mode"] == "shut":
                continue
            d = np.abs(st["th"] - st["bhp"])
            m = min(m, float(d.min()/d.max()))
        return m

    def residual(self, u):
        u = self.as_fields(u)
        R = super().residual(u)
        W = self._wells_R(u, frozen=self._frozen, record=not np.iscomplexobj(u) and self._frozen is None)
        if np.iscomplexobj(W) and not np.iscomplexobj(R):
            R = R.astype(complex)
        return R + W

    # ---------------------------------------------------------------- Jacobian: diagonal part and the rank-1 factors
    def jacobian(self, u, want_schur=False):
        u = self.as_fields(np.asarray(u, dtype=float))
        states = self.well_state(u)
        frozen = [(float(np.real(s["bhp"])), s["mode"], s["open"], float(np.real(s["sa"]))) for s in states]
        via_residual = hasattr(self, "schur_complex_step")          # the saturation-function classes differentiate residual()
        self._frozen = frozen
        try:
            out = super().jacobian(u, want_schur=want_schur)
        finally:
            self._frozen = None
        J, Sm = out if want_schur else (out, None)
        b = self.b
        cells = np.concatenate([w["cells"] for w in self.wells]) if self.wells else np.zeros(0, np.int64)
        if not via_residual and cells.size:
            Jd = J[0].reshape(b, b, -1)
            for col in range(b):
                uc = u.astype(complex)
                uc[col].reshape(-1)[cells] += 1j*HSTEP
                d = self._wells_R(uc, frozen=frozen).imag.reshape(b, -1)/HSTEP
                for r in range(b):
                    Jd[r, col, cells] += d[r, cells]
            if want_schur:
                Tx = u[1].astype(complex)
                Tx.reshape(-1)[cells] += 1j*HSTEP
                d = self._wells_R(u.astype(complex), frozen=frozen, Tx=Tx).imag.reshape(b, -1)/HSTEP
                Sm[0].reshape(-1)[cells] += d[1, cells]
        # factors
        self.last_factors = []
        p, T, S = (None if x is None else x.reshape(-1) for x in self.split(u))
        dR = self._wells_R(u.astype(complex), frozen=frozen, dbhp=1j*HSTEP).imag.reshape(b, -1)/HSTEP
        for i, (w, st) in enumerate(zip(self.wells, states)):
            c = w["cells"]
            cf, bf = np.zeros((b, c.size)), np.zeros((b, c.size))
            if st["mode"] == "rate":
                cf = dR[:, c].copy()
                opn = st["open"]
                sgn = 1.0 if w["kind"] == "prod" else -1.0
                for j in np.nonzero(opn)[0]:
                    for col in range(b):
                        pc, Tc = p[c].astype(complex), T[c].astype(complex)
                        Sc = None if S is None else S[c].astype(complex)
                        [pc, Tc, Sc][col][j] += 1j*HSTEP
                        lam = self._lam_G(w["kind"], pc, Tc, Sc, Tc)[0]
                        a = w["WI"]*lam
                        th = pc - self._head(i)
                        bhp = (np.sum(a[opn]*th[opn]) - sgn*w["rate"])/np.sum(a[opn])
                        bf[col, j] = bhp.imag/HSTEP
                if c.size == 1:                                     # one perforation: c b^T is a diagonal block
                    Jd = J[0].reshape(b, b, -1)
                    Jd[:, :, c[0]] += np.outer(cf[:, 0], bf[:, 0])
                    cf, bf = 0.0*cf, 0.0*bf
            self.last_factors.append((cf, bf))
        return (J, Sm) if want_schur else J

    def rank1(self, x):
        """sum_w c_w (b_w . x) as a vector shaped like x, with the factors of the last jacobian() call."""
        y = np.zeros_like(x)
        xf, yf = x.reshape(self.b, -1), y.reshape(self.b, -1)
        for w, (cf, bf) in zip(self.wells, self.last_factors):
            c = w["cells"]
            yf[:, c] += cf*np.sum(bf*xf[:, c])
        return y

    def dense_jacobian(self, u):
        """dF/du, every entry, by a complex step per unknown of the residual with NOTHING frozen: (b, ncell, b, ncell)."""
        u = self.as_fields(np.asarray(u, dtype=float))
        n = int(np.prod(self.shape))
        D = np.zeros((self.b, n, self.b, n))
        for col in range(self.b):
            for j in range(n):
                uc = u.astype(complex)
                uc[col].reshape(-1)[j] += 1j*HSTEP
                D[:, :, col, j] = self.residual(uc).imag.reshape(self.b, n)/HSTEP
        return D


class WellsProblem(WellsMixin, Problem):
    pass


def wells_problem(spec, hs=None, boundary=None, satfn=None, wells=None):
    """The reference with wells over the grid / sides / saturation functions asked for (spec's own keys when None)."""
    hs = spec.get("hs") if hs is None else hs
    boundary = spec.get("boundary") if boundary is None else boundary
    satfn = spec.get("satfn") if satfn is None else satfn
    if hs is not None and boundary and satfn is None:
        from graded_ref import GradedBcProblem
        return type("WellsGradedBcProblem", (WellsMixin, GradedBcProblem), {})(spec, boundary, hs, wells=wells)
    if satfn is not None and hs is not None and not boundary:
        from satfn_ref import SatfnGradedProblem
        return type("WellsSatfnGradedProblem", (WellsMixin, SatfnGradedProblem), {})(spec, hs, satfn=satfn, wells=wells)
    if satfn is not None and boundary and hs is None:
        from satfn_ref import SatfnBcProblem
        return type("WellsSatfnBcProblem", (WellsMixin, SatfnBcProblem), {})(spec, boundary, satfn=satfn, wells=wells)
    if satfn is not None and hs is None and not boundary:
        from satfn_ref import SatfnProblem
        return type("WellsSatfnProblem", (WellsMixin, SatfnProblem), {})(spec, satfn=satfn, wells=wells)
    if hs is not None and not boundary:
        from graded_ref import GradedProblem
        return type("WellsGradedProblem", (WellsMixin, GradedProblem), {})(spec, hs, wells=wells)
    if boundary and hs is None:
        from bc_ref import BcProblem
        return type("WellsBcProblem", (WellsMixin, BcProblem), {})(spec, boundary, wells=wells)
    if hs is None and not boundary and satfn is None:
        return WellsProblem(spec, wells=wells)
    from satfn_ref import SatfnGradedBcProblem
    return type("WellsSatfnGradedBcProblem", (WellsMixin, SatfnGradedBcProblem), {})(spec, boundary, hs, satfn=satfn, wells=wells)


def wells_oracle(spec, opts, wells=None):
    """An OracleEngine whose problem carries the wells and whose linear solves apply J + sum_w c_w b_w^T while the
    preconditioner is set up on J alone.  Honours the engine options linesearch ("bt") and ksp ("bcgs")."""
    from newton_ls_ref import make_ls_oracle_engine

    class WellsOracle(make_ls_oracle_engine()):
        def linear_solve(self, J, Sm, F):
            o = self.opts
            self.pc.setup(J, Sm)
            op = lambda x: la.spmv_block(J, x) + self.prob.rank1(x)
            if o.get("ksp", "fgmres") == "bcgs":
                from bcgs_ref import bcgs_ref
                return bcgs_ref(op, self.pc.apply, F, rtol=o["ksp_rtol"], atol=o["ksp_atol"], maxit=o["ksp_max_it"])
            return la.fgmres(op, self.pc.apply, F, rtol=o["ksp_rtol"], atol=o["ksp_atol"], restart=o["ksp_restart"], maxit=o["ksp_max_it"])

        def set_old(self, u=None):
            self.prob.set_old(self.u if u is None else np.array(u, dtype=float))

        def well_info(self):
            return self.prob.well_state(self.u)

        def set_well_control(self, i, rate=None, bhp=None, shut=None):
            w = self.prob.wells[i]
            w.update({k: v for k, v in (("rate", rate), ("bhp", bhp), ("shut", shut)) if v is not None})
    o = WellsOracle(spec, opts)
    o.prob = wells_problem(spec, wells=wells)
    o.pc = la.TwoStagePC(o.prob, o.opts)
    return o


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
    prob.wells = [dict(w) for w in wells]
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
    prob.wells = [dict(w) for w in out]
    prob.set_old(u)
    return out
