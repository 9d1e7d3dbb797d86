"""CPU reference of the Dirichlet sides: ``BcProblem`` adds the boundary faces to the oracle's residual, Jacobian
and S~, written in numpy from the definition and not through the library.

A boundary face of side ``2*a + d`` is an interior face between the cell and a ghost state (p_b, T_b[, S_b]) half a cell away,
the ghost's properties evaluated with the cell's own phi and static kT.  The lower index is '+': on a high side (d = 1) the cell
is P, the ghost M and R += f, Jdiag += dP, S~diag += sP; on a low side the ghost is P, the cell M and R -= f, Jdiag -= dM,
S~diag -= sM.  T^K = 2 K_a(c)|E|/h_a^2 (open) or 0 (thermal), Ga = 2|e_a|/h_a, gam = g h_a/4 on the gravity axis.

``spec["boundary"]`` (or the ``boundary`` argument): {side: {"kind": "open" | "thermal", "p", "T", "S"}}, arrays shaped like the
side: (n_hi, n_lo) over the other two internal axes.  ``last_flux`` (6, b) and ``last_phi`` hold the per-side sums and the
driving forces of the last residual() call."""
import copy

import numpy as np

from oracle import linalg as la
from oracle.tpfa import Problem, harmonic


def side_slice(side):
    """Index of the side's cells in an (n2, n1, n0) array."""
    a, d = divmod(int(side), 2)
    sl = [slice(None)]*3
    sl[2 - a] = -1 if d else 0
    return tuple(sl)


def side_shape(n, side):
    a = int(side)//2
    lo, hi = [k for k in range(3) if k != a]
    return (n[hi], n[lo])


class BcProblem(Problem):
    def __init__(self, spec, boundary=None):
        super().__init__(spec)
        self.boundary = dict(spec.get("boundary") or {}) if boundary is None else dict(boundary)
        self.last_flux = np.zeros((6, self.b))
        self.last_phi = {}

    # one side: everything face_flux needs, as arrays over the side's faces
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
        geom = self.V/self.h[a]**2
        TK = 2.0*self.K[a][sl]*geom if B["kind"] == "open" else np.zeros(shp)
        gam = self.prm["g"]*self.h[a]*0.25 if a == self.gaxis else 0.0
        P, M = (cell, ghost) if d else (ghost, cell)
        return a, d, sl, sub, P, M, TK, gam, 2.0*geom

    def _bc_flux(self, side, u):
        a, d, sl, sub, (pP, TP, prP), (pM, TM, prM), TK, gam, Ga = self._side(side, u)
        f = [0.0]*self.b
        phis = []
        for (Lk, rk, ce, c0, to2) in self.phases():
            Phi = pP - pM - gam*(prP[rk][0] + prM[rk][0])
            phis.append(np.array(Phi.real))
            up = Phi.real > 0.0                                 # strict: ties -> '-' side
            L = np.where(up, prP[Lk][0], prM[Lk][0])
            Tu = np.where(up, TP, TM)
            F = TK*L*Phi
            f[0] = f[0] + self.w0*c0*F
            f[1] = f[1] + ce*Tu*F
            if to2:
                f[2] = f[2] + self.w2*F
        f[1] = f[1] + harmonic(prP["kT"][0], prM["kT"][0])*Ga*(TP - TM)
        return d, sl, f, phis

    def residual(self, u):
        u = self.as_fields(u)
        R = super().residual(u)
        flux = np.zeros((6, self.b))
        self.last_phi = {}
        for side in sorted(self.boundary):
            d, sl, f, phis = self._bc_flux(side, u)
            sg = 1.0 if d else -1.0
            for q in range(self.b):
                R[q][sl] += sg*f[q]
                flux[side, q] = float(np.sum((sg*f[q]).real))
            self.last_phi[side] = phis
        self.last_flux = flux
        return R

    def jacobian(self, u, want_schur=False):
        u = self.as_fields(u)
        out = super().jacobian(u, want_schur=want_schur)
        J, Sm = out if want_schur else (out, None)
        b = self.b
        for side in sorted(self.boundary):
            a, d, sl, sub, (pP, TP, prP), (pM, TM, prM), TK, gam, Ga = self._side(side, u)
            shp = TK.shape
            dP, dM = np.zeros((b, b) + shp), np.zeros((b, b) + shp)
            sP, sM = np.zeros(shp), np.zeros(shp)
            bc = lambda x: np.broadcast_to(x, shp)
            for (Lk, rk, ce, c0, to2) in self.phases():
                rP, rM, LP, LM = prP[rk], prM[rk], prP[Lk], prM[Lk]
                Phi = pP - pM - gam*(rP[0] + rM[0])
                up = Phi > 0.0
                L = np.where(up, LP[0], LM[0])
                Tu = np.where(up, TP, TM)
                F = TK*L*Phi
                dPhiP = [1.0 - gam*rP[1], -gam*rP[2], 0.0]
                dPhiM = [-1.0 - gam*rM[1], -gam*rM[2], 0.0]
                for c in range(b):
                    dFP = TK*(L*dPhiP[c] + np.where(up, bc(LP[c + 1]), 0.0)*Phi)
                    dFM = TK*(L*dPhiM[c] + np.where(up, 0.0, bc(LM[c + 1]))*Phi)
                    dP[0, c] += self.w0*c0*dFP
                    dM[0, c] += self.w0*c0*dFM
                    dP[1, c] += ce*Tu*dFP
                    dM[1, c] += ce*Tu*dFM
                    if to2:
                        dP[2, c] += self.w2*dFP
                        dM[2, c] += self.w2*dFM
                dP[1, 1] += np.where(up, ce*F, 0.0)
                dM[1, 1] += np.where(up, 0.0, ce*F)
                sP += np.where(up, ce*F, 0.0)
                sM += np.where(up, 0.0, ce*F)
            kP, kM = prP["kT"][0], prM["kT"][0]
            Hk = harmonic(kP, kM)
            dP[1, 1] += Hk*Ga
            dM[1, 1] -= Hk*Ga
            sP += Hk*Ga
            sM -= Hk*Ga
            if self.nph == 2:
                s2 = kP + kM
                with np.errstate(divide="ignore", invalid="ignore"):
                    dHP = np.where(s2 > 0, 2*kM**2/np.where(s2 == 0, 1, s2)**2, 0.0)
                    dHM = np.where(s2 > 0, 2*kP**2/np.where(s2 == 0, 1, s2)**2, 0.0)
                dT = TP - TM
                dP[1, 2] += Ga*dT*dHP*bc(prP["kT"][1])
                dM[1, 2] += Ga*dT*dHM*bc(prM["kT"][1])
            for r in range(b):
                for c in range(b):
                    J[0, r, c][sl] += dP[r, c] if d else -dM[r, c]
            if want_schur:
                Sm[0][sl] += sP if d else -sM
        return (J, Sm) if want_schur else J


def make_boundary(spec, u, kinds, seed=0):
    """Per-face ghost arrays for the sides in `kinds` ({side: "open" | "thermal"}) around the state `u`: p_b = the adjacent
    cell's p plus noise whose sign alternates from face to face (so a side of two or more faces has flow in both directions),
    T_b in 290..360, S_b in 0.05..0.95."""
    rng = np.random.default_rng(seed)
    u = np.asarray(u, dtype=float)
    n = tuple(int(v) for v in spec["n"])
    out = {}
    for side, kind in sorted(kinds.items()):
        shp = side_shape(n, side)
        nf = shp[0]*shp[1]
        sign = np.where((np.arange(nf) + side) % 2 == 0, 1.0, -1.0).reshape(shp)
        pc = u[0][side_slice(side)].reshape(shp)
        out[side] = {"kind": kind, "p": pc + sign*rng.uniform(0.3, 1.5, shp), "T": 290.0 + 70.0*rng.random(shp),
                     "S": 0.05 + 0.9*rng.random(shp) if spec["nphase"] == 2 else None}
    return out


def assert_both_directions(prob):
    """Every open side of `prob` (after a residual() call) has faces with Phi > 0 and faces with Phi <= 0 for each phase: a side
    that shows one direction only is an error of the test's inputs."""
    for side, B in prob.boundary.items():
        if B["kind"] != "open":
            continue
        for k, Phi in enumerate(prob.last_phi[side]):
            assert (Phi > 0.0).any() and (Phi <= 0.0).any(), ("one flow direction only", side, k)


def bc_oracle(spec, opts, boundary=None):
    """An OracleEngine whose problem carries the Dirichlet sides (its preconditioner rebuilt on the new problem)."""
    from oracle.engine import OracleEngine
    o = OracleEngine(spec, opts)
    o.prob = BcProblem(spec, boundary)
    o.pc = la.TwoStagePC(o.prob, o.opts)
    return o


def hydrostatic_column(nz=5):
    """A single-phase z column (internal axis 0 = z, gravity on it) at uniform p and T, and for its bottom (side 0) and top (side 1)
    the ghost pressure half a cell away on the hydrostat THROUGH the end cell's centre: dp/dz = -rho(p, T) g integrated with 2000
    midpoint steps by the oracle's closures -- no use of the face formula or of its factor g h/4.  Returns spec, u, {side: p_b}."""
    import cases
    from oracle import closures as cl
    spec, u0, prm, *_ = cases.c4_spe10_3d(Nx=1, Ny=1, Nz=nz, nphase=1)
    spec = dict(spec)
    spec["sources"] = None
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (nz, 1, 1)
    u = np.array(u0, dtype=float)
    g, h, API = spec["prm"]["g"], spec["h"][0], spec["prm"]["API"]
    pb = {}
    for side, cell, sgn in ((0, 0, -1.0), (1, nz - 1, 1.0)):      # z up: the bottom ghost lies h/2 below, the top one h/2 above
        p, T = float(u[0, 0, 0, cell]), float(u[1, 0, 0, cell])
        dz = sgn*0.5*h/2000
        for _ in range(2000):
            pm = p - 0.5*dz*g*cl.oil_rho(p, T, API)[0]
            p = p - dz*g*cl.oil_rho(pm, T, API)[0]
        pb[side] = p
    return spec, u, pb


def hydrostatic_boundary(spec, u, pb, shift=0.0):
    """Open bottom and top of hydrostatic_column at the hydrostatic ghost pressures (+ shift), ghost T = the cell's."""
    one = np.ones((1, 1))
    nz = spec["n"][0]
    return {side: {"kind": "open", "p": (pb[side] + shift)*one, "T": u[1, 0, 0, cell]*one, "S": None}
            for side, cell in ((0, 0), (1, nz - 1))}
