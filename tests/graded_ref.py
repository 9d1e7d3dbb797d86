"""CPU reference of the graded tensor-product grid: ``GradedProblem`` restates the oracle's residual, Jacobian
and S~ with one width per cell index along each internal axis, in numpy from the definitions and not through the library.

Widths ``hs[a][i]`` (``spec["hs"]`` or the ``hs`` argument; internal axis order), cell volume V_c = hs[0][i0] hs[1][i1] hs[2][i2].
A face along a between the cells P (lower index, '+') and M: area A = V_P/h_a[i_P], half distances d = h_a/2, c = d/A on each
side.  T^K = K_P K_M/(c_P K_M + c_M K_P) (0 where the denominator is not positive), Phi = p_P - p_M - g (d_P + d_M)/2 (rho_P +
rho_M) on the gravity axis, conduction H (T_P - T_M) with H = k_P k_M/D, D = c_P k_M + c_M k_P, dH/dk_P = c_P k_M^2/D^2,
dH/dk_M = c_M k_P^2/D^2.  Accumulation takes V_c/dt per cell.  Upwinding, tie rule, weights, closures and sources: the oracle's.

``G[a]``: the coarsening strengths the library takes for amg_T with spacing -- the mean face area (product of the other two
axes' mean widths) times the mean of 1/(d_P + d_M) over the axis's interior faces -- so that the oracle's TwoStagePC coarsens
as the GPU does.

``GradedBcProblem`` adds BcProblem's Dirichlet sides under the boundary-face rule: K_M = K_P and both half distances h_a/4 of
the boundary cell, i.e. T^K = 2 K A/h, Ga = 2A/h and gam = g h/4 with the cell's own width and face area."""
import copy

import numpy as np

from bc_ref import BcProblem, side_slice
from oracle import linalg as la
from oracle.tpfa import Problem, _hi, _lo


def random_widths(n, lengths, seed=0):
    """Per axis n[a] widths drawn from a seeded uniform(0.4, 2.5) and rescaled to sum to lengths[a]."""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(3):
        w = rng.uniform(0.4, 2.5, int(n[a]))
        out.append(w*(float(lengths[a])/w.sum()))
    return tuple(out)


def equal_widths(spec):
    return tuple(np.full(int(spec["n"][a]), float(spec["h"][a])) for a in range(3))


def spec_lengths(spec):
    return tuple(float(spec["h"][a])*int(spec["n"][a]) for a in range(3))


def series(cP, cM, kP, kM):
    """k_P k_M/(c_P k_M + c_M k_P), 0 where the denominator is not positive; and the denominator."""
    D = cP*kM + cM*kP
    with np.errstate(divide="ignore", invalid="ignore"):
        H = np.where(D.real > 0.0, kP*kM/np.where(D == 0, 1.0, D), 0.0)
    return H, D


class GradedProblem(Problem):
    def __init__(self, spec, hs=None):
        super().__init__(spec)
        hs = spec["hs"] if hs is None else hs
        self.hs = tuple(np.asarray(hs[a], dtype=float).reshape(-1).copy() for a in range(3))
        assert all(self.hs[a].size == self.n[a] and (self.hs[a] > 0).all() for a in range(3))
        h0, h1, h2 = self.hs
        self.Vc = h2[:, None, None]*h1[None, :, None]*h0[None, None, :]           # (n2, n1, n0)
        self.V = None                                                             # (nothing may read one volume for all cells)
        # per axis: the cell's width as an array over the cells, the face area, c = (h/2)/A per cell
        self.ha, self.Aa, self.ca = [], [], []
        for a in range(3):
            sh = [1, 1, 1]
            sh[2 - a] = self.n[a]
            ha = np.broadcast_to(self.hs[a].reshape(sh), self.shape)
            A = self.Vc/ha
            self.ha.append(ha)
            self.Aa.append(A)
            self.ca.append(0.5*ha/A)
        self.TK, self.G = [], []
        for a in range(3):
            t = np.zeros(self.shape)
            if self.n[a] > 1:
                lo, hi = _lo(a), _hi(a)
                t[lo] = series(self.ca[a][lo], self.ca[a][hi], self.K[a][lo], self.K[a][hi])[0]
            self.TK.append(t)
            self.G.append(self.mean_strength(a))

    def mean_strength(self, a):
        """Mean of A/(d_P + d_M) over the interior faces of axis a, formed as the library forms it."""
        if self.n[a] <= 1:
            return 0.0
        area = 1.0
        for o in range(3):
            if o != a:
                area *= float(np.sum(self.hs[o]))/self.hs[o].size
        w = self.hs[a]
        inv = float(np.sum(1.0/(0.5*(w[:-1] + w[1:]))))
        return area*inv/(w.size - 1)

    # ------------------------------------------------------------------ residual
    def residual(self, u):
        u = self.as_fields(u)
        p, T, S = self.split(u)
        pr = self.props(p, T, S)
        w = [self.w0, 1.0, self.w2]
        R = (self.accum(p, T, S, pr) - self.old)*(self.Vc/self.dt)
        R = R.astype(u.dtype, copy=False)
        for q in range(self.b):
            R[q] = R[q]*w[q]
        for a in range(3):
            if self.n[a] == 1:
                continue
            f = self._face_flux(a, p, T, pr)
            lo, hi = _lo(a), _hi(a)
            for q in range(self.b):
                R[q][lo] += f[q]
                R[q][hi] -= f[q]
        if self.src is not None:
            c = self.src["cell"]
            pc, Tc = p.reshape(-1)[c], T.reshape(-1)[c]
            Sc = S.reshape(-1)[c] if S is not None else None
            s = self.source_terms(pc, Tc, Sc)
            Rf = R.reshape(self.b, -1)
            for q in range(self.b):
                np.subtract.at(Rf[q], c, s[q])
        return R

    def _gam_face(self, a):
        """g (d_P + d_M)/2 per face of axis a (0 off the gravity axis)."""
        lo, hi = _lo(a), _hi(a)
        if a != self.gaxis:
            return np.zeros(self.ha[a][lo].shape)
        return self.prm["g"]*0.25*(self.ha[a][lo] + self.ha[a][hi])

    def _phi_face(self, a, p, rho):
        lo, hi = _lo(a), _hi(a)
        return p[lo] - p[hi] - self._gam_face(a)*(rho[lo] + rho[hi])

    def _conduction(self, a, kT):
        lo, hi = _lo(a), _hi(a)
        return series(self.ca[a][lo], self.ca[a][hi], kT[lo], kT[hi])

    def _face_flux(self, a, p, T, pr):
        lo, hi = _lo(a), _hi(a)
        TK = self.TK[a][lo]
        f = [0.0]*self.b
        for (Lk, rk, ce, c0, to2) in self.phases():
            Phi = self._phi_face(a, p, pr[rk][0])
            up = Phi.real > 0.0                       # strict: ties -> '-' side
            L = np.where(up, pr[Lk][0][lo], pr[Lk][0][hi])
            Tu = np.where(up, T[lo], T[hi])
            F = TK*L*Phi
            f[0] = f[0] + self.w0*c0*F
            f[1] = f[1] + ce*Tu*F
            if to2:
                f[2] = f[2] + self.w2*F
        H, _ = self._conduction(a, pr["kT"][0])
        f[1] = f[1] + H*(T[lo] - T[hi])
        return f

    # ------------------------------------------------------------------ Jacobian (analytic)
    def jacobian(self, u, want_schur=False):
        u = self.as_fields(u)
        p, T, S = self.split(u)
        pr = self.props(p, T, S)
        b, prm = self.b, self.prm
        J = np.zeros((7, b, b) + self.shape)
        Sm = np.zeros((7,) + self.shape) if want_schur else None
        w = [self.w0, 1.0, self.w2]
        Vdt = self.Vc/self.dt
        phi = self.phi
        rock = (1 - phi)*prm["rho_r"]*prm["c_r"]
        ro, ro_p, ro_T = pr["ro"]
        if self.nph == 2:
            rw, rw_p, rw_T = pr["rw"]
            cw, co = prm["c_v_w"], prm["c_v_o"]
            Mw = (phi*rw*(1 - S), phi*rw_p*(1 - S), phi*rw_T*(1 - S), -phi*rw)
            Mo = (phi*ro*S, phi*ro_p*S, phi*ro_T*S, phi*ro)
            for c in range(3):
                e0 = cw*Mw[c + 1] + co*Mo[c + 1]
                J[0, 0, c] += w[0]*e0*Vdt
                J[0, 1, c] += e0*T*Vdt
                J[0, 2, c] += w[2]*Mo[c + 1]*Vdt
            J[0, 1, 1] += (cw*Mw[0] + co*Mo[0] + rock)*Vdt
            if want_schur:
                Sm[0] += (phi*co*S*ro + phi*cw*(1 - S)*rw + rock)*Vdt
        else:
            cv = prm["c_v_o"]
            Mo = (phi*ro, phi*ro_p, phi*ro_T)
            for c in range(2):
                J[0, 0, c] += w[0]*Mo[c + 1]*Vdt
                J[0, 1, c] += cv*Mo[c + 1]*T*Vdt
            J[0, 1, 1] += (cv*Mo[0] + rock)*Vdt
            if want_schur:
                Sm[0] += (phi*cv*ro + rock)*Vdt
        for a in range(3):
            if self.n[a] == 1:
                continue
            lo, hi = _lo(a), _hi(a)
            TK = self.TK[a][lo]
            fs = (b, b) + TK.shape
            dP, dM = np.zeros(fs), np.zeros(fs)
            sP, sM = np.zeros(TK.shape), np.zeros(TK.shape)
            gam = self._gam_face(a)
            for (Lk, rk, ce, c0, to2) in self.phases():
                rho = pr[rk]
                Phi = self._phi_face(a, p, rho[0])
                up = Phi > 0.0
                Lt = pr[Lk]
                L = np.where(up, Lt[0][lo], Lt[0][hi])
                Tu = np.where(up, T[lo], T[hi])
                F = TK*L*Phi
                dPhiP = [1.0 - gam*rho[1][lo], -gam*rho[2][lo], 0.0]
                dPhiM = [-1.0 - gam*rho[1][hi], -gam*rho[2][hi], 0.0]
                for c in range(b):
                    dLP = np.where(up, np.broadcast_to(Lt[c + 1], self.shape)[lo], 0.0)
                    dLM = np.where(up, 0.0, np.broadcast_to(Lt[c + 1], self.shape)[hi])
                    dFP = TK*(L*dPhiP[c] + dLP*Phi)
                    dFM = TK*(L*dPhiM[c] + dLM*Phi)
                    dP[0, c] += w[0]*c0*dFP
                    dM[0, c] += w[0]*c0*dFM
                    dP[1, c] += ce*Tu*dFP
                    dM[1, c] += ce*Tu*dFM
                    if to2:
                        dP[2, c] += w[2]*dFP
                        dM[2, c] += w[2]*dFM
                dP[1, 1] += np.where(up, ce*F, 0.0)
                dM[1, 1] += np.where(up, 0.0, ce*F)
                if want_schur:
                    sP += np.where(up, ce*F, 0.0)
                    sM += np.where(up, 0.0, ce*F)
            kT, kT_S = pr["kT"]
            kP, kM = kT[lo], kT[hi]
            H, D = self._conduction(a, kT)
            dP[1, 1] += H
            dM[1, 1] -= H
            if want_schur:
                sP += H
                sM -= H
            if self.nph == 2:
                cP, cM = self.ca[a][lo], self.ca[a][hi]
                with np.errstate(divide="ignore", invalid="ignore"):
                    D2 = np.where(D == 0, 1.0, D)**2
                    dHP = np.where(D > 0, cP*kM**2/D2, 0.0)
                    dHM = np.where(D > 0, cM*kP**2/D2, 0.0)
                dT = T[lo] - T[hi]
                dP[1, 2] += dT*dHP*np.broadcast_to(kT_S, self.shape)[lo]
                dM[1, 2] += dT*dHM*np.broadcast_to(kT_S, self.shape)[hi]
            for r in range(b):
                for c in range(b):
                    J[0, r, c][lo] += dP[r, c]
                    J[2 + 2*a, r, c][lo] += dM[r, c]
                    J[0, r, c][hi] -= dM[r, c]
                    J[1 + 2*a, r, c][hi] -= dP[r, c]
            if want_schur:
                Sm[0][lo] += sP
                Sm[2 + 2*a][lo] += sM
                Sm[0][hi] -= sM
                Sm[1 + 2*a][hi] -= sP
        if self.src is not None:
            cidx = self.src["cell"]
            pc, Tc = p.reshape(-1)[cidx], T.reshape(-1)[cidx]
            Sc = S.reshape(-1)[cidx] if S is not None else None
            dS = self.source_jac(pc, Tc, Sc)
            Jd = J[0].reshape(b, b, -1)
            for r in range(b):
                for c in range(b):
                    np.subtract.at(Jd[r, c], cidx, dS[r, c])
            if want_schur:
                np.subtract.at(Sm[0].reshape(-1), cidx, self.schur_source_diag(pc, Tc, Sc))
        return (J, Sm) if want_schur else J


class GradedBcProblem(BcProblem, GradedProblem):
    """GradedProblem with BcProblem's sides: only the geometry of a boundary face differs (per-face arrays over the side)."""

    def __init__(self, spec, boundary=None, hs=None):
        GradedProblem.__init__(self, spec, hs)
        self.boundary = dict(spec.get("boundary") or {}) if boundary is None else dict(boundary)
        self.last_flux = np.zeros((6, self.b))
        self.last_phi = {}

    def _side(self, side, u):
        a, d = divmod(int(side), 2)
        B = self.boundary[side]
        sl = side_slice(side)
        p, T, S = self.split(u)
        pc, Tc = p[sl], T[sl]
        Sc = S[sl] if S is not None else None
        sub = copy.copy(self)                                   # props() on the side's cells: their own phi and static kT
        sub.phi, sub.shape = self.phi[sl], pc.shape
        sub.kT_static = self.kT_static[sl] if self.kT_static is not None else None
        shp = pc.shape
        z = 0*pc                                                # (carries a complex dtype through)
        pb = np.asarray(B["p"], dtype=float).reshape(shp) + z
        Tb = np.asarray(B["T"], dtype=float).reshape(shp) + z
        Sb = (np.asarray(B["S"], dtype=float).reshape(shp) + z) if S is not None else None
        cell = (pc, Tc, sub.props(pc, Tc, Sc))
        ghost = (pb, Tb, sub.props(pb, Tb, Sb))
        h, A = self.ha[a][sl], self.Aa[a][sl]                   # the boundary cell's own width and face area
        TK = 2.0*self.K[a][sl]*A/h if B["kind"] == "open" else np.zeros(shp)
        gam = self.prm["g"]*h*0.25 if a == self.gaxis else np.zeros(shp)
        P, M = (cell, ghost) if d else (ghost, cell)
        return a, d, sl, sub, P, M, TK, gam, 2.0*A/h


def graded_oracle(spec, opts, hs=None, boundary=None):
    """An OracleEngine whose problem is graded (with the Dirichlet sides of spec["boundary"], if any), its preconditioner rebuilt on
    the new problem: the scalar hierarchies coarsen by the problem's TK and G."""
    from oracle.engine import OracleEngine
    o = OracleEngine(spec, opts)
    bnd = spec.get("boundary") if boundary is None else boundary
    o.prob = GradedBcProblem(spec, bnd, hs) if bnd else GradedProblem(spec, hs)
    o.pc = la.TwoStagePC(o.prob, o.opts)
    return o


def cell_centres_internal(hs):
    """Centre coordinates along each internal axis from the cumulative widths."""
    return tuple(np.cumsum(w) - 0.5*w for w in hs)


def hydrostatic_graded_column(props=(1.0, 4.0, 2.0, 8.0, 1.0, 4.0)):
    """A single-phase z column 1x1xN (internal axis 0 = z, gravity on it) with widths proportional to `props`, uniform T, and at
    the cell centres the pressure of the hydrostat dp/dz = -rho(p, T) g, integrated from the bottom centre upwards with 4000
    midpoint steps per interval between two centres by the oracle's closures: no use of the face formula or of its distance.
    Returns spec (with "hs", no sources), u, and per interior face the scale T^K L rho g d of the flux the gravity head alone
    would drive (d the distance between the two centres, the properties those of the lower cell)."""
    import cases
    from oracle import closures as cl
    nz = len(props)
    spec, u0, prm, *_ = cases.c4_spe10_3d(Nx=1, Ny=1, Nz=nz, nphase=1)
    spec = dict(spec)
    spec["sources"] = None
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (nz, 1, 1)
    w = np.asarray(props, dtype=float)
    eq = equal_widths(spec)
    spec["hs"] = (w*(spec_lengths(spec)[0]/w.sum()), eq[1], eq[2])
    z = cell_centres_internal(spec["hs"])[0]
    u = np.array(u0, dtype=float)
    g, API = spec["prm"]["g"], spec["prm"]["API"]
    T = float(u[1, 0, 0, 0])
    p = float(u[0, 0, 0, 0])
    for i in range(1, nz):
        dz = (z[i] - z[i - 1])/4000
        for _ in range(4000):
            pm = p - 0.5*dz*g*cl.oil_rho(p, T, API)[0]
            p = p - dz*g*cl.oil_rho(pm, T, API)[0]
        u[0, 0, 0, i] = p
    u[1] = T
    P = GradedProblem(spec)
    pr = P.props(u[0], u[1], None)
    lo = (0, 0, slice(None, -1))
    scale = P.TK[0][lo]*pr["Lo"][0][lo]*pr["ro"][0][lo]*g*np.diff(z)
    return spec, u, np.asarray(scale, dtype=float).reshape(-1)


def field_change(Ra, Rb, spec):
    """Per field ||Ra - Rb|| / ||Rb|| over the cells that carry no well or heater entry: a source term is orders of magnitude
    above the face fluxes and does not depend on the spacing, so with those cells in, no norm would show the faces."""
    mask = np.ones(int(np.prod(Rb.shape[1:])), dtype=bool)
    src = spec.get("sources")
    if src is not None and len(src["cell"]):
        mask[np.asarray(src["cell"], dtype=np.int64)] = False
    assert mask.sum() >= 2
    out = []
    for f in range(Rb.shape[0]):
        a, b = Ra[f].reshape(-1)[mask], Rb[f].reshape(-1)[mask]
        out.append(float(np.linalg.norm(a - b)/np.linalg.norm(b)))
    return out
