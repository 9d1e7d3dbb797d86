"""Inputs and independent checks for the saturation functions.  The reference itself is ``oracle.tpfa.Problem``
with ``spec["satfn"]`` (or its ``satfn`` argument); ``curves`` is the oracle's, written from the definitions and not through the
library or through thermalporous_amd.physicalparameters."""
import numpy as np

from oracle import closures as cl
from oracle.tpfa import SATFN_DEFAULT as DEFAULT
from oracle.tpfa import Problem, curves

M1 = dict(relperm="corey", Sr_o=0.2, Sr_w=0.15, n_o=2.0, n_w=3.0, kro_max=0.9, krw_max=0.4)
M2 = dict(relperm="brooks_corey", lmbda=2.0, Sr_o=0.2, Sr_w=0.15, capillary="linear", p_ct=0.05)
M3 = dict(M1, capillary="brooks_corey", p_ct=0.01, lmbda=2.0, pc_se_min=0.05)
DEGENERATE = dict(relperm="corey", Sr_o=0.0, Sr_w=0.0, n_o=1.0, n_w=1.0, kro_max=1.0, krw_max=1.0)
MODELS = {"M1": M1, "M2": M2, "M3": M3}


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
    P = Problem(spec)
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
