"""Water flood of an oil-saturated box, once with the straight-line relative permeabilities (``relperm = "linear"``) and once
with Corey curves (``relperm = "corey"``: residual oil, connate water, a saturation shock): homogeneous, two-phase, a water
injector in one corner column and a producer in the opposite one, nothing else.  Prints the water front of both runs: the mean
oil saturation of every x slice.  Under the linear curves the front smears and oil keeps flowing down to S_o = 0; under Corey's
it steepens and stops at Sr_o.  Usage:
    python test3D_waterflood_corey.py cptr 1.0 100.0 [Nx Ny Nz]      # pcname maxdt[days] end[days]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from thermalporous_amd.physicalparameters import PhysicalParameters as Params
from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo as GeoModel
from thermalporous_amd.wellcase import WellCase as TestCase
from thermalporous_amd.twophase import TwoPhase as ThermalModel

COREY = dict(relperm="corey", Sr_o=0.2, Sr_w=0.15, n_o=2.0, n_w=3.0, kro_max=0.9, krw_max=0.4)


def build(Nx=20, Ny=10, Nz=4, satfn=None, pcname="cptr", maxdt=1.0, end=100.0, filename=None, verbosity=False, **kw):
    """The flood's model: `satfn` are PhysicalParameters attributes (relperm, Sr_o, ..., capillary, p_ct) or None for the
    linear curves."""
    params = Params()
    params.S_o = 0.85                  # oil-saturated down to the connate water of COREY
    params.API = 30.0
    params.T_inj = params.T_prod       # an isothermal flood: the fronts are the saturation's alone
    params.rate = 2e-4
    for k, v in (satfn or {}).items():
        setattr(params, k, v)
    geo = GeoModel(Nx, Ny, Nz, params, Length=Nx*6.096, Length_y=Ny*6.096, Length_z=Nz*0.6096)
    L, Ly, Lz = geo.Length, geo.Length_y, geo.Length_z
    case = TestCase(params, geo, prod_points=[[L - 3.0, Ly - 3.0, 0.5*Lz]], inj_points=[[3.0, 3.0, 0.5*Lz]])
    return ThermalModel(geo, case, params, end=end, maxdt=maxdt, save=False, small_dt_start=False,
                        solver_parameters="pc_" + pcname, filename=filename, verbosity=verbosity, **kw)


def front(model):
    """Mean S_o of every x slice."""
    geo = model.geo
    S = np.asarray(model.u._read()[2]).reshape(geo.Nz, geo.Ny, geo.Nx)
    return S.mean(axis=(0, 1))


if __name__ == "__main__":
    pcname = sys.argv[1] if len(sys.argv) > 1 else "cptr"
    maxdt = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    end = float(sys.argv[3]) if len(sys.argv) > 3 else 100.0
    N = tuple(int(v) for v in sys.argv[4:7]) if len(sys.argv) > 6 else (20, 10, 4)
    suffix = os.path.splitext(__file__)[0]
    np.set_printoptions(precision=3, linewidth=200)
    for name, satfn in (("linear", None), ("corey", COREY)):
        model = build(*N, satfn=satfn, pcname=pcname, maxdt=maxdt, end=end,
                      filename=suffix + "_" + name + "_" + pcname + "_results.txt", verbosity=True)
        model.solve()
        print("%s: total Newton its %d, total Krylov its %d, failed solves %d, oil in place %.6g kg"
              % (name, model.total_nits, model.total_lits, model.failed_solves, model.oil_mass()))
        print("%s: mean S_o per x slice: %s" % (name, front(model)))
