"""CPU reference of the saturation functions: ``SatfnProblem`` restates the oracle's two-phase residual with
Corey / Brooks-Corey relative permeabilities and a capillary pressure, in numpy from the definitions and not through the library
or through thermalporous_amd.physicalparameters.

With D = 1 - Sr_o - Sr_w, Se_o = (S_o - Sr_o)/D, Se_w = (1 - S_o - Sr_w)/D:
  kr_o = kro_max Se_o^n_o inside 0 < Se_o < 1, 0 at and below 0, kro_max at and above 1 (kr_w alike on Se_w); "brooks_corey" is
  "corey" with both exponents (2 + 3 lmbda)/lmbda; "linear" is S_o and 1 - S_o.
  p_c = p_ct (1 - min(max(Se_w, 0), 1)) ("linear") or p_ct s^(-1/lmbda), s = min(max(Se_w, pc_se_min), 1) ("brooks_corey").
  p_w = p - p_c(S_o): water density at (p_w, T) in the accumulation (new and old), the water mobility and the gravity head; the
  water driving force Phi_w = p_w+ - p_w- - gam (rho_w+ + rho_w-).  Oil, kT, the rock term, the weights and the tie rules: the
  oracle's.  Wells: drawdown and densities at p; the producers' total mobility and split by kr_a(S_o)/mu_a.

Every branch (clamps, upwinding, rate caps) is taken on the real part, so a complex perturbation differentiates the branch in
force.  The Jacobian is the complex step of residual() over the 7-colouring (i0 + 2 i1 + 3 i2) mod 7 (the oracle's
jacobian_complex_step); nothing here carries a derivative by hand.  S~, the temperature convection-diffusion operator, is the
derivative of the energy row with respect to the temperature that enters it EXPLICITLY -- the T of (e0 + rock) T, the upwind T of
the advected heat, the T+ - T- of the conduction, the T of the producers' and heaters' terms -- with densities, mobilities, fluxes
and conductivities held: residual() takes that temperature from ``self._Tx`` when it is set, and S~ is its complex step.

``SatfnBcProblem``, ``SatfnGradedProblem`` and ``SatfnGradedBcProblem`` compose the same overrides with tests/bc_ref.py and
tests/graded_ref.py."""
import numpy as np

from bc_ref import BcProblem
from graded_ref import GradedBcProblem, GradedProblem
from oracle import closures as cl
from oracle import linalg as la
from oracle.tpfa import HEATER, INJ, PROD, Problem, _hi, _lo, harmonic

DEFAULT = {"relperm": "linear", "capillary": None, "Sr_o": 0.0, "Sr_w": 0.0, "n_o": 2.0, "n_w": 2.0, "kro_max": 1.0,
           "krw_max": 1.0, "lmbda": 2.0, "p_ct": 0.0, "pc_se_min": 0.05}

M1 = dict(relperm="corey", Sr_o=0.2, Sr_w=0.15, n_o=2.0, n_w=3.0, kro_max=0.9, krw_max=0.4)
M2 = dict(relperm="brooks_corey", lmbda=2.0, Sr_o=0.2, Sr_w=0.15, capillary="linear", p_ct=0.05)
M3 = dict(M1, capillary="brooks_corey", p_ct=0.01, lmbda=2.0, pc_se_min=0.05)
DEGENERATE = dict(relperm="corey", Sr_o=0.0, Sr_w=0.0, n_o=1.0, n_w=1.0, kro_max=1.0, krw_max=1.0)
MODELS = {"M1": M1, "M2": M2, "M3": M3}


def _inside(x, lo=0.0):
    return (x.real > lo) & (x.real < 1.0)


def curves(sat, S):
    """kr_o, kr_w, p_c at S_o = S (real or complex arrays), branches on the real part."""
    sat = {**DEFAULT, **sat}
    S = np.asarray(S)
    D = 1.0 - sat["Sr_o"] - sat["Sr_w"]
    Se_o = (S - sat["Sr_o"])/D
    Se_w = ((1.0 - sat["Sr_w"]) - S)/D                  # (this order: S_o = 1 - Sr_w is the end exactly, as S_o = Sr_o is)
    if sat["relperm"] == "linear":
        kr_o, kr_w = S + 0.0, 1.0 - S
    else:
        n_o, n_w = sat["n_o"], sat["n_w"]
        if sat["relperm"] == "brooks_corey":
            n_o = n_w = (2.0 + 3.0*sat["lmbda"])/sat["lmbda"]
        z = 0.0*S
        io, iw = _inside(Se_o), _inside(Se_w)
        kr_o = np.where(io, sat["kro_max"]*np.where(io, Se_o, 0.5)**n_o, np.where(Se_o.real >= 1.0, sat["kro_max"] + z, z))
        kr_w = np.where(iw, sat["krw_max"]*np.where(iw, Se_w, 0.5)**n_w, np.where(Se_w.real >= 1.0, sat["krw_max"] + z, z))
    z = 0.0*S
    if sat["capillary"] is None:
        pc = z
    elif sat["capillary"] == "linear":
        iw = _inside(Se_w)
        pc = np.where(iw, sat["p_ct"]*(1.0 - Se_w), np.where(Se_w.real >= 1.0, z, sat["p_ct"] + z))
    else:
        smin, e = sat["pc_se_min"], -1.0/sat["lmbda"]
        iw = _inside(Se_w, smin)
        pc = np.where(iw, sat["p_ct"]*np.where(iw, Se_w, 0.5)**e, np.where(Se_w.real >= 1.0, sat["p_ct"] + z, sat["p_ct"]*smin**e + z))
    return kr_o, kr_w, pc


class SatfnMixin:
    """The overrides, for any of Problem, BcProblem and GradedProblem behind it in the MRO."""

    def __init__(self, spec, *args, satfn=None, **kw):
        super().__init__(spec, *args, **kw)
        assert self.nph == 2, "saturation functions need the two-phase model"
        self.sat = {**DEFAULT, **(spec.get("satfn") or {} if satfn is None else satfn)}
        self._Tx = None                   # the explicit temperature of the energy row, when it is differentiated alone (S~)

    # ---------------------------------------------------------------- closures
    def props(self, p, T, S):
        prm = self.prm
        kr_o, kr_w, pc = curves(self.sat, S)
        ro = cl.oil_rho(p, T, prm["API"])[0]
        mo = cl.oil_mu(T, prm["API"])[0]
        rw = cl.water_rho(p - pc, T)[0]                   # water at its own pressure p_w = p - p_c(S_o)
        mw = cl.water_mu(T)[0]
        phi = self.phi
        return {"ro": (ro,), "rw": (rw,), "Lo": (kr_o*ro/mo,), "Lw": (kr_w*rw/mw,), "pc": pc, "mu": (mo, None, mw, None),
                "kT": (phi*(S*prm["ko"] + (1 - S)*prm["kw"]) + (1 - phi)*prm["kr"], phi*(prm["ko"] - prm["kw"]))}

    def _explicit_T(self, T):
        return T if self._Tx is None else self._Tx

    def accum(self, p, T, S, pr=None):
        prm = self.prm
        pr = pr or self.props(p, T, S)
        phi = self.phi
        rock = (1 - phi)*prm["rho_r"]*prm["c_r"]
        Tx = self._explicit_T(T)
        Mw = phi*pr["rw"][0]*(1.0 - S)                    # rho_w(p - p_c(S_o), T)
        Mo = phi*pr["ro"][0]*S
        e0 = prm["c_v_w"]*Mw + prm["c_v_o"]*Mo
        return np.array([e0, e0*Tx + rock*Tx, Mo])

    def set_old(self, u_old):
        keep, self._Tx = self._Tx, None
        super().set_old(u_old)
        self._Tx = keep

    # ---------------------------------------------------------------- faces
    def _phase_pressure(self, rk, p, pr):
        return p - pr["pc"] if rk == "rw" else p

    def _conduct(self, a, kT, T):
        lo, hi = _lo(a), _hi(a)
        if hasattr(self, "_conduction"):                  # graded: two half cells in series
            return self._conduction(a, kT)[0]*(T[lo] - T[hi])
        return harmonic(kT[lo], kT[hi])*self.G[a]*(T[lo] - T[hi])

    def _face_flux(self, a, p, T, pr):
        lo, hi = _lo(a), _hi(a)
        TK = self.TK[a][lo]
        Tx = self._explicit_T(T)
        f = [0.0]*self.b
        for (Lk, rk, ce, c0, to2) in self.phases():
            Phi = self._phi_face(a, self._phase_pressure(rk, p, pr), pr[rk][0])
            up = Phi.real > 0.0                           # strict: ties -> '-' side
            L = np.where(up, pr[Lk][0][lo], pr[Lk][0][hi])
            Tu = np.where(up, Tx[lo], Tx[hi])
            F = TK*L*Phi
            f[0] = f[0] + self.w0*c0*F
            f[1] = f[1] + ce*Tu*F
            if to2:
                f[2] = f[2] + self.w2*F
        f[1] = f[1] + self._conduct(a, pr["kT"][0], Tx)
        return f

    # ---------------------------------------------------------------- sources
    def source_terms(self, p, T, S, return_rates=False):
        prm = self.prm
        e = self.src
        kind, wt, bhp, qmax, WI, const = (e[k] for k in ("kind", "wt", "bhp", "max_rate", "WI", "const"))
        API = prm["API"]
        is_prod, is_inj = kind == PROD, kind == INJ
        Tx = T if self._Tx is None else self._Tx.reshape(-1)[e["cell"]]
        mo = cl.oil_mu(T, API)[0]
        ro = cl.oil_rho(p, T, API)[0]                     # wells: densities at p, drawdown on p (wellcase.py:204-235)
        mw = cl.water_mu(T)[0]
        rw = cl.water_rho(p, T)[0]
        kr_o, kr_w, _ = curves(self.sat, S)
        dd_raw = bhp - p
        dd = np.where(is_prod, np.where(dd_raw.real >= 0.0, 0.0, dd_raw), np.where(dd_raw.real <= 0.0, 0.0, dd_raw))

        def cap(rate):
            rate = np.where(np.abs(rate.real) - np.abs(qmax) >= 0.0, qmax, rate)
            return np.where(const != 0, qmax, rate)
        lam_o, lam_w = kr_o/mo, kr_w/mw
        lam_t = lam_o + lam_w
        rate_p = cap(WI*lam_t*dd)
        safe = np.where(lam_t.real > 0.0, lam_t, 1.0)     # (both phases immobile: no split; S_o in [Sr_o, 1 - Sr_w] never is)
        qw = lam_w/safe*rate_p
        qo = lam_o/safe*rate_p
        rate_i = cap(WI/mw*dd)
        rw_inj = cl.water_rho(p, prm["T_inj"] + 0*T)[0]
        cw, co = prm["c_v_w"], prm["c_v_o"]
        out = np.zeros((self.b, len(kind)), dtype=np.result_type(p, T, S, Tx))
        out[0] = self.w0*np.where(is_prod, cw*rw*qw + co*ro*qo, np.where(is_inj, cw*rw_inj*rate_i, 0.0))*wt
        out[2] = self.w2*np.where(is_prod, ro*qo, 0.0)*wt
        out[1] = np.where(is_prod, (rw*qw*cw + ro*qo*co)*Tx,
                          np.where(is_inj, rw_inj*rate_i*cw*prm["T_inj"], prm["U"]*(prm["T_inj"] - Tx)))*wt
        if return_rates:
            return out, {"rate": np.where(is_prod, rate_p, np.where(is_inj, rate_i, 0.0)),
                         "water_rate": np.where(is_prod, qw, 0.0), "oil_rate": np.where(is_prod, qo, 0.0)}
        return out

    # ---------------------------------------------------------------- Jacobian and S~ by complex step
    def _colour_slots(self):
        n0, n1, n2 = self.n
        i2, i1, i0 = np.meshgrid(np.arange(n2), np.arange(n1), np.arange(n0), indexing="ij")
        col = (i0 + 2*i1 + 3*i2) % 7
        offs = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
        masks = []
        for (d0, d1, d2) in offs:
            j0, j1, j2 = i0 + d0, i1 + d1, i2 + d2
            ok = (j0 >= 0) & (j0 < n0) & (j1 >= 0) & (j1 < n1) & (j2 >= 0) & (j2 < n2)
            masks.append((ok, (j0 + 2*j1 + 3*j2) % 7))
        return col, masks

    def schur_complex_step(self, u):
        u = self.as_fields(u).astype(float)
        col, masks = self._colour_slots()
        Sm = np.zeros((7,) + self.shape)
        hstep = 1e-30
        uc = u.astype(complex)
        try:
            for k in range(7):
                self._Tx = uc[1].copy()
                self._Tx[col == k] += 1j*hstep
                dR = self.residual(uc)[1].imag/hstep
                for s, (ok, cj) in enumerate(masks):
                    m = ok & (cj == k)
                    Sm[s][m] = dR[m]
        finally:
            self._Tx = None
        return Sm

    def jacobian(self, u, want_schur=False):
        J = self.jacobian_complex_step(u)
        return (J, self.schur_complex_step(u)) if want_schur else J


class SatfnProblem(SatfnMixin, Problem):
    pass


class SatfnGradedProblem(SatfnMixin, GradedProblem):
    def __init__(self, spec, hs=None, satfn=None):
        super().__init__(spec, hs, satfn=satfn)


class SatfnSidesMixin(SatfnMixin):
    """The boundary face under saturation functions, for BcProblem or GradedBcProblem behind it: whatever ``_side`` gives as the
    face's geometry, the phase pressures go through p_c and the water density is taken at p_w on both sides of the face."""

    def _bc_flux(self, side, u):
        a, d, sl, sub, (pP, TP, prP), (pM, TM, prM), TK, gam, Ga = self._side(side, u)
        if self._Tx is not None:                            # the cell's explicit temperature; the ghost's is data
            if d:
                TP = self._Tx[sl]
            else:
                TM = self._Tx[sl]
        f = [0.0]*self.b
        phis = []
        for (Lk, rk, ce, c0, to2) in self.phases():
            Phi = self._phase_pressure(rk, pP, prP) - self._phase_pressure(rk, pM, prM) - gam*(prP[rk][0] + prM[rk][0])
            phis.append(np.array(Phi.real))
            up = Phi.real > 0.0
            L = np.where(up, prP[Lk][0], prM[Lk][0])
            Tu = np.where(up, TP, TM)
            F = TK*L*Phi
            f[0] = f[0] + self.w0*c0*F
            f[1] = f[1] + ce*Tu*F
            if to2:
                f[2] = f[2] + self.w2*F
        f[1] = f[1] + harmonic(prP["kT"][0], prM["kT"][0])*Ga*(TP - TM)
        return d, sl, f, phis


class SatfnBcProblem(SatfnSidesMixin, BcProblem):
    def __init__(self, spec, boundary=None, satfn=None):
        super().__init__(spec, boundary, satfn=satfn)


class SatfnGradedBcProblem(SatfnSidesMixin, GradedBcProblem):
    """All three at once: GradedBcProblem._side gives the boundary cell's own width and face area (gam = g h/4, Ga = 2A/h, T^K =
    2 K A/h).  With c_P = c_M = h/(4A) the series conduction k_P k_M/(c_P k_M + c_M k_P) is harmonic(k_P, k_M) Ga, so the flux
    body above carries over unchanged; the interior faces are SatfnGradedProblem's."""

    def __init__(self, spec, boundary=None, hs=None, satfn=None):
        super().__init__(spec, boundary, hs, satfn=satfn)


def satfn_oracle(spec, opts, satfn=None):
    """An OracleEngine whose problem is a SatfnProblem (its preconditioner rebuilt on the new problem)."""
    from oracle.engine import OracleEngine
    o = OracleEngine(spec, opts)
    o.prob = SatfnProblem(spec, satfn=satfn)
    o.pc = la.TwoStagePC(o.prob, o.opts)
    return o


def satfn_graded_bc_oracle(spec, opts):
    """An OracleEngine whose problem is a SatfnGradedBcProblem on spec's own widths, sides and curves."""
    from oracle.engine import OracleEngine
    o = OracleEngine(spec, opts)
    o.prob = SatfnGradedBcProblem(spec)
    o.pc = la.TwoStagePC(o.prob, o.opts)
    return o


# ---- the capillary-gravity column --------------------------------------------------------------------------------------------
COLUMN_SAT = dict(relperm="corey", Sr_o=0.2, Sr_w=0.15, capillary="linear", p_ct=0.05)


def capillary_gravity_column(nz=8, dz=2.5, se_w_bottom=0.9, sat=None):
    """A two-phase z column 1 x 1 x nz of height dz per cell, API 40 (at the default API 10 oil is as dense as water and nothing
    segregates), no sources, at capillary-gravity equilibrium: from a bottom cell with Se_w = se_w_bottom, every next cell up
    solves the 2 x 2 system Phi_o = 0, Phi_w = 0 of the face below it for (p, S_o) by Newton with complex-step derivatives of
    this module's closures.  Returns spec (with "satfn"), u, and per phase (water, oil) and interior face the scale T^K L rho g dz
    of the flux that phase's gravity head alone would drive, the properties those of the lower cell."""
    import cases
    from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo
    from thermalporous_amd.physicalparameters import PhysicalParameters
    from thermalporous_amd.problem import build_spec
    sat = {**DEFAULT, **(COLUMN_SAT if sat is None else sat)}
    prm = PhysicalParameters()
    prm.API = 40.0
    prm.S_o = 0.5
    geo = HomogeneousBoxGeo(1, 1, nz, prm, Length=5.0, Length_y=5.0, Length_z=nz*dz)
    spec = build_spec(geo, None, prm, 2)
    spec["sources"] = None
    spec["satfn"] = sat
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (nz, 1, 1)
    g, API = spec["prm"]["g"], spec["prm"]["API"]
    gam = 0.5*g*float(spec["h"][0])
    T = 320.0
    D = 1.0 - sat["Sr_o"] - sat["Sr_w"]

    def rho(p, S):
        pc = curves(sat, S)[2]
        return cl.oil_rho(p, T, API)[0], cl.water_rho(p - pc, T)[0], pc

    u = cases.uniform_state(spec, spec["prm"]["p_ref"], T, 1.0 - sat["Sr_w"] - se_w_bottom*D)
    for i in range(1, nz):
        pP, SP = u[0, 0, 0, i - 1], u[2, 0, 0, i - 1]
        roP, rwP, pcP = rho(pP, SP)

        def F(x):
            roM, rwM, pcM = rho(x[0], x[1])
            return np.array([pP - x[0] - gam*(roP + roM), (pP - pcP) - (x[0] - pcM) - gam*(rwP + rwM)])
        x = np.array([pP - 2.0*gam*roP, SP], dtype=float)
        for _ in range(50):
            f = F(x)
            Jm = np.zeros((2, 2))
            for k in range(2):
                xc = x.astype(complex)
                xc[k] += 1e-30j
                Jm[:, k] = F(xc).imag/1e-30
            dx = np.linalg.solve(Jm, f.real)
            x = x - dx
            if np.abs(dx).max() < 1e-15*np.abs(x).max():
                break
        u[0, 0, 0, i], u[2, 0, 0, i] = x
    P = SatfnProblem(spec)
    pr = P.props(u[0], u[1], u[2])
    lo = (0, 0, slice(None, -1))
    scale = [P.TK[0][lo]*pr[Lk][0][lo]*pr[rk][0][lo]*g*float(spec["h"][0]) for Lk, rk in (("Lw", "rw"), ("Lo", "ro"))]
    return spec, u, np.asarray(scale, dtype=float).reshape(2, -1)


def column_face_fluxes(P, R):
    """(water, oil) mass flux through every interior face of a source-free column from its residual with old = state: the rows are
    R_2 = w2 (F_o,i - F_o,i-1) and R_0 = w0 (c_w dF_w + c_o dF_o)."""
    R = np.asarray(R).reshape(3, -1)
    Fo = np.cumsum(R[2])[:-1]/P.w2
    Fw = (np.cumsum(R[0])[:-1]/P.w0 - P.prm["c_v_o"]*Fo)/P.prm["c_v_w"]
    return np.array([Fw, Fo])
