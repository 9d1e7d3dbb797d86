"""Completed wells of the oracle's TPFA problem (test infrastructure): the component ``Wells`` that a
``oracle.tpfa.Problem`` owns, written in numpy from the definition and not through the library.

A well (an entry of ``spec["wells"]``: kind, rate Q, bhp limit, z_ref, and per perforation the flat internal cell, WI and the
elevation z) has, with u_k the state of its k-th perforated cell,
    a_k = WI_k lambda_k(u_k),   theta_k = p_k - rho_w g (z_ref - z_k),   q_k = -a_k (theta_k - bhp) where open, else 0,
open meaning theta_k > bhp for a producer and theta_k < bhp for an injector.  In rate mode bhp solves sum_k q_k = -+Q by
active-set rounds (``solve_bhp``); in BHP mode (the limit violated, or nothing mobile open) bhp is the limit.  rho_w is frozen
over a time step: ``set_old`` computes it.  A perforation adds G(u_k) q_k, what a source entry of its kind adds for the rate q_k
with weight 1.  Mobilities are the problem's (``relperm``).

Every decision (open / closed, the mode) is taken on real parts, so a complex perturbation differentiates the branch in force.
The problem's ``jacobian`` freezes the wells' bhp at its real value (``frozen_at``) and forms J by its own route; the wells' part
of the diagonal blocks and of S~ comes from complex steps of their contribution (``add_diagonal``; the complex step of
residual() carries it already), and so do the factors c = dR/dbhp and b = dbhp/du (``set_factors``).  The exact Jacobian is
J + sum_w c_w b_w^T, which ``rank1`` applies; a well of one perforation has its c b^T folded into the diagonal block and zero
factors, as the library does it.  Without wells the component adds nothing."""
import contextlib

import numpy as np

from . import closures as cl

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


class Wells:
    def __init__(self, prob, wells):
        self.P = prob
        self.wells = [dict(w) for w in wells]
        for w in self.wells:
            w["cells"] = np.asarray(w["cells"], dtype=np.int64)
            w["WI"], w["z"] = np.asarray(w["WI"], dtype=float), np.asarray(w["z"], dtype=float)
            if w.get("z_ref") is None:
                w["z_ref"] = float(w["z"].max())
        self.rho_w = [0.0]*len(self.wells)
        self._frozen = None               # per well (bhp, mode, open, sa) while the problem's jacobian() runs
        self._states = None
        self.last_wells = []
        self.last_factors = []

    # ---------------------------------------------------------------- closures of one well's perforations
    def _lam_G(self, kind, p, T, S, Tx):
        """lambda and G (b rows) at the perforated cells; fw, fo: the phase split of the rate."""
        P = self.P
        prm = P.prm
        API, Ti = prm["API"], prm["T_inj"]
        mo = cl.oil_mu(T, API)[0]
        one = 1.0 + 0.0*p
        if P.nph == 1:
            lam = 1.0/mo
            if kind == "prod":
                ro = cl.oil_rho(p, T, API)[0]
                return lam, [P.w0*ro, ro*prm["c_v_o"]*Tx], 0.0*one, one
            roi = cl.oil_rho(p, Ti + 0.0*T, API)[0]
            return lam, [P.w0*roi, roi*(prm["c_v_o"]*Ti)], 0.0*one, one
        mw = cl.water_mu(T)[0]
        cw, co = prm["c_v_w"], prm["c_v_o"]
        if kind == "prod":
            kr_o, kr_w = P.relperm(S)
            lo, lw = kr_o/mo, kr_w/mw
            lam = lo + lw
            safe = np.where(lam.real > 0.0, lam, 1.0)
            gw, go = lw/safe, lo/safe
            ro, rw = cl.oil_rho(p, T, API)[0], cl.water_rho(p, T)[0]
            m = rw*gw*cw + ro*go*co
            dead = ~(lam.real > 0.0)
            G = [np.where(dead, 0.0, P.w0*m), np.where(dead, 0.0, m*Tx), np.where(dead, 0.0, P.w2*ro*go)]
            return np.where(dead, 0.0, lam), G, gw, go
        rwi = cl.water_rho(p, Ti + 0.0*T)[0]
        return 1.0/mw, [P.w0*cw*rwi, rwi*(cw*Ti), 0.0*one], one, 0.0*one

    def _head(self, i):
        w = self.wells[i]
        if self.P.gaxis < 0:
            return 0.0*w["z"]
        return self.rho_w[i]*self.P.prm["g"]*(w["z_ref"] - w["z"])

    def _flat(self, u):
        return (None if x is None else x.reshape(-1) for x in self.P.split(u))

    def set_old(self, u_old):
        P = self.P
        p, T, S = self._flat(P.as_fields(np.asarray(u_old, dtype=float)))
        prm = P.prm
        for i, w in enumerate(self.wells):
            c = w["cells"]
            if w["kind"] == "inj":
                k = int(np.argmin(np.abs(w["z"] - w["z_ref"])))
                pd = p[c[k]]
                self.rho_w[i] = float(cl.water_rho(pd, prm["T_inj"])[0] if P.nph == 2 else cl.oil_rho(pd, prm["T_inj"], prm["API"])[0])
                continue
            pc, Tc = p[c], T[c]
            mo = cl.oil_mu(Tc, prm["API"])[0]
            ro = cl.oil_rho(pc, Tc, prm["API"])[0]
            if P.nph == 1:
                num, den = np.sum(w["WI"]*ro/mo), np.sum(w["WI"]/mo)
            else:
                kr_o, kr_w = P.relperm(S[c])
                lo, lw = kr_o/mo, kr_w/cl.water_mu(Tc)[0]
                num = np.sum(w["WI"]*(lo*ro + lw*cl.water_rho(pc, Tc)[0]))
                den = np.sum(w["WI"]*(lo + lw))
            self.rho_w[i] = float(num/den) if den > 0.0 else 0.0

    # ---------------------------------------------------------------- the wells' part of the residual
    def _wells_R(self, u, frozen=None, Tx=None, dbhp=0.0, record=False):
        """What the wells add to R at u (zeros elsewhere).  frozen: per well (bhp, mode, open, sa) to use instead of solving;
        dbhp: added to every rate-mode bhp (the complex step for c)."""
        P = self.P
        u = P.as_fields(u)
        p, T, S = self._flat(u)
        if Tx is None:
            Tx = P._Tx
        Txf = T if Tx is None else np.asarray(Tx).reshape(-1)
        out = np.zeros((P.b, p.size), dtype=np.result_type(u.dtype, Txf.dtype, type(dbhp)))
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
            for r in range(P.b):
                out[r, c] -= G[r]*q
            rec.append(dict(bhp=bhp, mode=mode, open=opn, rounds=rounds, sa=sa, q=q, qw=fw*q, qo=fo*q, a=a, th=th))
        if record:
            self.last_wells = rec
        return out.reshape((P.b,) + P.shape)

    def add_to(self, R, u):
        """R plus the wells' part at u (R itself without wells)."""
        if not self.wells:
            return R
        W = self._wells_R(u, frozen=self._frozen, record=not np.iscomplexobj(u) and self._frozen is None)
        if np.iscomplexobj(W) and not np.iscomplexobj(R):
            R = R.astype(complex)
        return R + W

    def state(self, u):
        """Per well at the real state u: bhp, mode, open, rounds, sa, q, qw, qo, a, th."""
        self._wells_R(np.asarray(u, dtype=float), record=True)
        return self.last_wells

    def kink_margin(self, u):
        """The smallest |theta_k - bhp| over the perforations of the active wells, relative to the drawdown scale (the largest
        |theta_k - bhp| of the same well)."""
        m = np.inf
        for st in self.state(u):
            if st["mode"] == "shut":
                continue
            d = np.abs(st["th"] - st["bhp"])
            m = min(m, float(d.min()/d.max()))
        return m

    # ---------------------------------------------------------------- Jacobian: diagonal part and the rank-1 factors
    @contextlib.contextmanager
    def frozen_at(self, u):
        """While it holds, residual() takes every well's bhp, mode and open set as they are at the real state u."""
        self._states = self.state(u)
        self._frozen = [(float(np.real(s["bhp"])), s["mode"], s["open"], float(np.real(s["sa"]))) for s in self._states]
        try:
            yield
        finally:
            self._frozen = None

    def add_diagonal(self, u, J, Sm):
        """The wells' part of the diagonal blocks of J (and of S~, if not None) by complex steps of their contribution."""
        b = self.P.b
        cells = np.concatenate([w["cells"] for w in self.wells]) if self.wells else np.zeros(0, np.int64)
        if not cells.size:
            return
        Jd = J[0].reshape(b, b, -1)
        for col in range(b):
            uc = u.astype(complex)
            uc[col].reshape(-1)[cells] += 1j*HSTEP
            d = self._wells_R(uc, frozen=self._frozen).imag.reshape(b, -1)/HSTEP
            for r in range(b):
                Jd[r, col, cells] += d[r, cells]
        if Sm is not None:
            Tx = u[1].astype(complex)
            Tx.reshape(-1)[cells] += 1j*HSTEP
            d = self._wells_R(u.astype(complex), frozen=self._frozen, Tx=Tx).imag.reshape(b, -1)/HSTEP
            Sm[0].reshape(-1)[cells] += d[1, cells]

    def set_factors(self, u, J):
        """last_factors: per well (c, b), each (b, perforations); a one-perforation well's c b^T goes into J's diagonal block."""
        b = self.P.b
        self.last_factors = []
        if not self.wells:
            return
        p, T, S = self._flat(u)
        dR = self._wells_R(u.astype(complex), frozen=self._frozen, dbhp=1j*HSTEP).imag.reshape(b, -1)/HSTEP
        for i, (w, st) in enumerate(zip(self.wells, self._states)):
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

    def rank1(self, x):
        """sum_w c_w (b_w . x) as a vector shaped like x, with the factors of the last jacobian() call (zeros without wells)."""
        y = np.zeros_like(x)
        xf, yf = x.reshape(self.P.b, -1), y.reshape(self.P.b, -1)
        for w, (cf, bf) in zip(self.wells, self.last_factors):
            c = w["cells"]
            yf[:, c] += cf*np.sum(bf*xf[:, c])
        return y
