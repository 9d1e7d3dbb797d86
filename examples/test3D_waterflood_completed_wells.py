"""Water flood of an oil-saturated layered box through COMPLETED wells: an injector and a producer in opposite corners, each open
over the whole column of layers, sharing one bottom-hole pressure along the bore, seeing the hydrostatic head between their
perforations, operated at a total rate until the BHP limit binds (``CompletedWellCase``).  Half-way through the
run the producer's rate target is doubled with ``model.set_well_control``.  Prints per well the BHP, the mode and the rates of
every time step, and at the end the rate of every perforation: the layers do not take equal shares.  Usage:
    python test3D_waterflood_completed_wells.py cptr 1.0 100.0 [Nx Ny Nz]      # pcname maxdt[days] end[days]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from thermalporous_amd.physicalparameters import PhysicalParameters as Params
from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo as GeoModel
from thermalporous_amd.completedwells import CompletedWellCase as TestCase
from thermalporous_amd.twophase import TwoPhase as ThermalModel


def build(Nx=20, Ny=10, Nz=8, pcname="cptr", maxdt=1.0, end=100.0, filename=None, verbosity=False, **kw):
    params = Params()
    params.S_o = 0.85
    params.API = 30.0
    params.T_inj = params.T_prod       # an isothermal flood
    geo = GeoModel(Nx, Ny, Nz, params, Length=Nx*6.096, Length_y=Ny*6.096, Length_z=Nz*0.6096)
    # layers: the permeability falls by a factor 30 from the top layer to the bottom one
    layer = np.logspace(0.0, -1.5, Nz)[::-1]
    for name in ("K_x", "K_y", "K_z"):
        setattr(geo, name, np.asarray(getattr(geo, name), dtype=float)*np.ones((Nx, Ny, Nz))*layer[None, None, :])
    L, Ly, Lz = geo.Length, geo.Length_y, geo.Length_z
    case = TestCase(params, geo)
    case.add_injector("I", xy=(3.0, 3.0), z=(0.0, Lz), rate=2e-4, bhp=params.p_inj)
    case.add_producer("P", xy=(L - 3.0, Ly - 3.0), z=(0.0, Lz), rate=1e-4, bhp=params.p_prod)
    return ThermalModel(geo, case, params, end=end, maxdt=maxdt, save=False, small_dt_start=False,
                        solver_parameters="pc_" + pcname, filename=filename, verbosity=verbosity, **kw)


if __name__ == "__main__":
    pcname = sys.argv[1] if len(sys.argv) > 1 else "cptr"
    maxdt = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    end = float(sys.argv[3]) if len(sys.argv) > 3 else 100.0
    N = tuple(int(v) for v in sys.argv[4:7]) if len(sys.argv) > 6 else (20, 10, 8)
    np.set_printoptions(precision=3, linewidth=200)
    model = build(*N, pcname=pcname, maxdt=maxdt, end=end,
                  filename=os.path.splitext(__file__)[0] + "_" + pcname + "_results.txt", verbosity=True)
    model.start()
    doubled = False
    while model.t < model.end*86400.0:
        model.step()
        if not doubled and model.t >= 0.5*model.end*86400.0:
            model.set_well_control("P", rate=2e-4)
            doubled = True
    model.finish()
    for w, q in zip(model.engine.well_info(), model.engine.well_perf_rates()):
        print("%s: bhp %.4f, mode %s, rate %.4e (water %.4e, oil %.4e), head density %.2f" %
              (w["name"], w["bhp"], w["mode"], w["rate"], w["water_rate"], w["oil_rate"], w["rho"]))
        print("%s: rate per perforation, bottom layer first: %s" % (w["name"], q["rate"]))
    print("total Newton its %d, total Krylov its %d, failed solves %d, oil in place %.6g kg"
          % (model.total_nits, model.total_lits, model.failed_solves, model.oil_mass()))
