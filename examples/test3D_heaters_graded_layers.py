"""Heat loss into cap and base rock on a graded grid: the box of test3D_heaters_thermal_walls.py -- homogeneous, two-phase,
two heaters, thermal top and bottom held at the initial temperature -- with its z layers thinned geometrically towards the cap
and the base (``geo.set_spacing``), so that the conduction fronts that leave the two walls are resolved without refining
every cell of the box.  The spacing is set before the case is built: the heaters pick their cells on the graded grid.  Usage:
    python test3D_heaters_graded_layers.py cptr 0.1 1.0 [Nx Ny Nz [ratio]]      # pcname maxdt[days] end[days]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from thermalporous_amd.physicalparameters import PhysicalParameters as Params
from thermalporous_amd.homogeneousboxgeo import HomogeneousBoxGeo as GeoModel
from thermalporous_amd.heatercase import HeaterCase as TestCase
from thermalporous_amd.spacing import geometric_widths
from thermalporous_amd.twophase import TwoPhase as ThermalModel

params = Params()
params.S_o = 0.9
params.T_inj = 373.15

pcname = sys.argv[1] if len(sys.argv) > 1 else "cptr"
maxdt = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
end = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
Nx, Ny, Nz = (int(v) for v in sys.argv[4:7]) if len(sys.argv) > 6 else (20, 20, 10)
ratio = float(sys.argv[7]) if len(sys.argv) > 7 else 1.6

geo = GeoModel(Nx, Ny, Nz, params, Length=Nx*6.096, Length_y=Ny*6.096, Length_z=Nz*0.6096)
geo.set_spacing(z=geometric_widths(Nz, geo.Length_z, ratio, refine="both"))      # thin layers at the base and at the cap
geo.set_boundary("z-", "thermal", T=params.T_prod)      # base rock
geo.set_boundary("z+", "thermal", T=params.T_prod)      # cap rock
case = TestCase(params, geo, well_case="default")

suffix = os.path.splitext(__file__)[0]
model = ThermalModel(geo, case, params, end=end, maxdt=maxdt, save=False, small_dt_start=False,
                     solver_parameters="pc_" + pcname, filename=suffix + "_" + pcname + "_results.txt")
model.solve()
hz = geo.cell_widths()[2]
loss = model.rates().get("boundary_energy", {})
print("z layers from %.4g to %.4g m (mean %.4g)" % (hz.min(), hz.max(), geo.Dz))
print("total Newton its %d, total Krylov its %d, last dt %.4g days, failed solves %d"
      % (model.total_nits, model.total_lits, model.last_dt/86400.0, model.failed_solves))
print("energy leaving through the walls at the last assembly:", loss)
