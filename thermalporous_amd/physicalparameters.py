"""Physical constants and closure laws (host-side mirror of the reference class).

Mirrors /root/reference/thermalporous/physicalparameters.py:3-98 attribute for attribute
(same names, same SI/MPa/mm^2 scaling), so driver scripts that mutate ``params.rate`` etc.
keep working.  The closure methods here are numpy restatements used on the host only for
diagnostics (oil in place, well rates); the device evaluates its own copy inside the HIP
assembly kernels (csrc/tp_closures.hpp).

Saturation functions.  The reference's Brooks-Corey / capillary-pressure members
(:100-152: ``Sr_o``, ``Sr_w``, ``lmbda``, ``p_ct``, ``rel_perm_*_B_C``, ``capillary_pressure_*``) sit
behind ``if False:`` (twophase.py:103,277) and never run there; here they are a model option, off by
default: ``relperm`` = "linear" (``kr_o = S_o``, ``kr_w = 1 - S_o``: the reference's executed curves) |
"corey" | "brooks_corey", ``capillary`` = None | "linear" | "brooks_corey", with the attributes below.
With D = 1 - Sr_o - Sr_w, Se_o = (S_o - Sr_o)/D, Se_w = (1 - S_o - Sr_w)/D (formed as ((1 - Sr_w) - S_o)/D, so that the
state S_o = 1 - Sr_w is the end of the curve exactly, as S_o = Sr_o is) and c(x) = min(max(x, 0), 1):

    corey          kr_o = kro_max c(Se_o)^n_o,  kr_w = krw_max c(Se_w)^n_w
    brooks_corey   corey with n_o = n_w = (2 + 3 lmbda)/lmbda (the reference's rel_perm_*_B_C, which however
                   has no clamp at Se > 1: there it grows past the end point, here it stays at it)
    p_c linear        p_ct (1 - c(Se_w))
    p_c brooks_corey  p_ct s^(-1/lmbda),  s = min(max(Se_w, pc_se_min), 1)

p_c = p_o - p_w >= 0 with p_o = p the unknown (twophase.py:104-106).  ``rel_perm_o`` / ``rel_perm_w`` follow
``relperm``; ``satfn_dict()`` is what ``build_spec`` passes on as ``spec["satfn"]`` when the setting is not the default.
"""
import numpy as np


class PhysicalParameters():
    ko = 0.15              # conductivity of oil in W/m*K            (:9)
    kw = 0.6005638         # conductivity of water                   (:10)
    kr = 1.7295772056      # conductivity of rock (SPE4)             (:12)
    c_v_w = 4181.3         # specific heat of water J/(K*kg)         (:13)
    c_v_o = 2093.4         # specific heat of oil                    (:14)
    c_r = 920.0            # specific heat of sandstone              (:15)
    rho_r = 2650.0         # density of sandstone                    (:16)
    p_inj = 6.895e7*1e-6   # injection bhp, MPa                      (:17)
    p_prod = 2.7579e7*1e-6  # production bhp, MPa                    (:18)
    T_inj = 422.039        # 300F                                    (:20)
    T_prod = 288.706       # 60F                                     (:23)
    API = 10.0             #                                         (:24)
    p_ref = 4.1369e7*1e-6  # SPE10 reference pressure, MPa           (:25)
    T_ref = (T_inj+T_prod)/2.0
    g = 9.80665*1e-6       # gravity in MPa-consistent units         (:27)
    S_o = 1.0              # default initial oil saturation          (:28)
    U = 5.44409e6          # heater coefficient J/(s*K)              (:29)
    rate = 1.8e-3          # max inj/prod rate m^3/s                 (:30)
    well_radius = 0.1      #                                         (:35)

    def oil_rho(self, p, T):                                   # (:37-46)
        SG = 141.5/(self.API + 131.5)
        rho_ref = SG*999.0
        c = 5.5e-5
        p0 = 1.01325
        e1 = 2.5e-4
        T0 = 15.5556 + 273.15
        pbar = p*1e1
        return rho_ref*np.exp(c*(pbar-p0))*np.exp(-e1*(T-T0))

    def oil_mu(self, T):                                       # (:48-57)
        A1, A2, A3, A4 = -0.8021, 23.8765, 0.31458, -9.21592
        Tf = 1.8*(T - 273.15) + 32.0
        return 1E-3*(10.0**(A1*self.API + A2) * Tf**(A3*self.API + A4))

    def water_rho(self, p, T):                                 # (:69-82)
        E_0, E_1, E_2, E_3 = 999.83952, 16.955176, -7.987E-3, -46.170461E-6
        E_4, E_5, E_6, E_7 = 105.56302E-9, -280.54353E-12, 16.87985E-3, 10.2
        Cw = 3.98854E-4
        Tc = T - 272.15
        return (E_0 + E_1*Tc + E_2*Tc**2 + E_3*Tc**3 + E_4*Tc**4 + E_5*Tc**5)*np.exp(Cw*(p-E_7))/(1 + E_6*Tc)

    def water_mu(self, T):                                     # (:84-90)
        Aw, Bw, Cw = 2.1850, 0.04012, 5.1547E-6
        Tf = 1.8*(T - 272.15) + 32
        return 1E-3*Aw/(-1 + Bw*Tf + Cw*Tf**2)

    # saturation functions (module docstring): the defaults are the reference's executed model
    relperm = "linear"     # "linear" | "corey" | "brooks_corey"
    Sr_o = 0.0             # residual oil saturation                 (:100-103)
    Sr_w = 0.0             # connate water saturation
    n_o = 2.0              # Corey exponents, >= 1
    n_w = 2.0
    kro_max = 1.0          # end-point relative permeabilities, > 0
    krw_max = 1.0
    lmbda = 2.0            # Brooks-Corey pore-size index, > 0
    capillary = None       # None | "linear" | "brooks_corey"
    p_ct = 0.0             # capillary entry pressure, MPa, >= 0
    pc_se_min = 0.05       # floor of Se_w in the Brooks-Corey p_c, in (0, 1]: a model parameter

    def effective_saturation_o(self, S_o):                     # (:100-103)
        return (S_o - self.Sr_o)/(1.0 - self.Sr_o - self.Sr_w)

    def effective_saturation_w(self, S_o):                     # (:105-109)
        return ((1.0 - self.Sr_w) - S_o)/(1.0 - self.Sr_o - self.Sr_w)     # (this order: S_o = 1 - Sr_w gives exactly 0)

    def _corey_exponents(self):
        if self.relperm == "brooks_corey":
            n = (2.0 + 3.0*self.lmbda)/self.lmbda              # (:129,137)
            return n, n
        return float(self.n_o), float(self.n_w)

    def rel_perm_o(self, S_o):                                 # (:92-94, :124-129)
        check_satfn(self.satfn_dict())
        if self.relperm == "linear":
            return S_o
        return self.kro_max*np.clip(self.effective_saturation_o(S_o), 0.0, 1.0)**self._corey_exponents()[0]

    def rel_perm_w(self, S_o):                                 # (:96-98, :131-138)
        check_satfn(self.satfn_dict())
        if self.relperm == "linear":
            return 1.0 - S_o
        return self.krw_max*np.clip(self.effective_saturation_w(S_o), 0.0, 1.0)**self._corey_exponents()[1]

    def capillary_pressure(self, S_o):                         # (:140-152)
        """p_c(S_o) = p_o - p_w in MPa; zero without ``capillary``."""
        check_satfn(self.satfn_dict())
        Se_w = self.effective_saturation_w(S_o)
        if self.capillary is None:
            return 0.0*Se_w
        if self.capillary == "linear":
            return self.p_ct*(1.0 - np.clip(Se_w, 0.0, 1.0))
        return self.p_ct*np.clip(Se_w, self.pc_se_min, 1.0)**(-1.0/self.lmbda)

    def satfn_dict(self):
        """The saturation-function setting as plain data (spec["satfn"], HipEngine.set_saturation_functions)."""
        d = {"relperm": self.relperm, "capillary": self.capillary}
        d.update({k: getattr(self, k) for k in SATFN_NUMBERS})          # (as set: check_satfn names what is no number)
        return d

    def as_dict(self):
        """Scalar parameters handed to the compute engine (tp_set_params)."""
        keys = ("ko", "kw", "kr", "c_v_w", "c_v_o", "c_r", "rho_r", "p_inj", "p_prod", "T_inj",
                "T_prod", "API", "p_ref", "g", "S_o", "U", "rate")
        return {k: float(getattr(self, k)) for k in keys}


SATFN_NUMBERS = ("Sr_o", "Sr_w", "n_o", "n_w", "kro_max", "krw_max", "lmbda", "p_ct", "pc_se_min")
SATFN_DEFAULT = {"relperm": "linear", "capillary": None, "Sr_o": 0.0, "Sr_w": 0.0, "n_o": 2.0, "n_w": 2.0, "kro_max": 1.0,
                 "krw_max": 1.0, "lmbda": 2.0, "p_ct": 0.0, "pc_se_min": 0.05}
RELPERMS = ("linear", "corey", "brooks_corey")
CAPILLARIES = (None, "linear", "brooks_corey")


def check_satfn(d):
    """A saturation-function setting against its ranges; every refusal names the key.  Returns the dict completed with the
    defaults."""
    unknown = sorted(set(d) - set(SATFN_DEFAULT))
    if unknown:
        raise ValueError("saturation functions: unknown key(s) %s: the keys are %s" % (unknown, sorted(SATFN_DEFAULT)))
    d = {**SATFN_DEFAULT, **d}
    if d["relperm"] not in RELPERMS:
        raise ValueError("relperm = %r: 'linear', 'corey' or 'brooks_corey'" % (d["relperm"],))
    if d["capillary"] not in CAPILLARIES:
        raise ValueError("capillary = %r: None, 'linear' or 'brooks_corey'" % (d["capillary"],))
    for k in SATFN_NUMBERS:
        v = d[k]
        if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isfinite(v):
            raise ValueError("%s = %r: a finite number" % (k, v))
        d[k] = float(v)
    if d["Sr_o"] < 0.0:
        raise ValueError("Sr_o = %r: the residual oil saturation, >= 0" % d["Sr_o"])
    if d["Sr_w"] < 0.0:
        raise ValueError("Sr_w = %r: the connate water saturation, >= 0" % d["Sr_w"])
    if not d["Sr_o"] + d["Sr_w"] < 1.0:
        raise ValueError("Sr_o + Sr_w = %r: the residual saturations must leave a mobile range, Sr_o + Sr_w < 1"
                         % (d["Sr_o"] + d["Sr_w"],))
    for k in ("n_o", "n_w"):
        if d[k] < 1.0:
            raise ValueError("%s = %r: a Corey exponent, >= 1" % (k, d[k]))
    for k in ("kro_max", "krw_max"):
        if not d[k] > 0.0:
            raise ValueError("%s = %r: an end-point relative permeability, > 0" % (k, d[k]))
    if not d["lmbda"] > 0.0:
        raise ValueError("lmbda = %r: the Brooks-Corey pore-size index, > 0" % d["lmbda"])
    if d["p_ct"] < 0.0:
        raise ValueError("p_ct = %r: the capillary entry pressure in MPa, >= 0" % d["p_ct"])
    if not 0.0 < d["pc_se_min"] <= 1.0:
        raise ValueError("pc_se_min = %r: the floor of Se_w in the Brooks-Corey p_c, in (0, 1]" % d["pc_se_min"])
    return d


def satfn_is_default(d):
    """True for the linear / no-p_c setting, whatever the other numbers hold: nothing reads them then."""
    return d is None or (d.get("relperm", "linear") == "linear" and d.get("capillary") is None)
