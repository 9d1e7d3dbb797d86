"""Graded grids in the time loop: ``geo.set_spacing`` -> case (wells and a heater picked by coordinate on the graded grid) -> model ->
engine, two time steps against the oracle engine stepping the same spec, oil in place with the cells' own volumes, and the
RectilinearGrid field output."""
import glob
import os

import numpy as np
import pytest

from oracle.engine import OracleEngine
from test_gpu_parity import rel2

pytestmark = pytest.mark.gpu


def _geo_case(nphase):
    """A 6x5x6 SPE10-like box whose z layers thin out towards the top and the base and whose x columns are refined towards the
    producer's end; the wells and the heater sit in thin cells that floor(w/D) with mean widths would miss."""
    from thermalporous_amd.physicalparameters import PhysicalParameters
    from thermalporous_amd.SPE10model3D import SPE10Model3D
    from thermalporous_amd.sourceterms import SourceTerms
    from thermalporous_amd.spacing import geometric_widths
    p = PhysicalParameters()
    p.rate = 2e-5          # (a producer in a cell a ninth of the mean volume: at config 4's 2e-4 the step of 0.002 d drains it and is halved)
    p.S_o = 0.9
    p.T_inj = 373.15
    g = SPE10Model3D(6, 5, 6, p)
    g.set_spacing(x=geometric_widths(6, g.Length, 1.5, "low"), z=geometric_widths(6, g.Length_z, 2.0, "both"))
    L, Ly, Lz = g.Length, g.Length_y, g.Length_z
    c = SourceTerms(p, g, prod_points=[[0.03*L, 0.5*Ly, 0.02*Lz]], inj_points=[[0.9*L, 0.5*Ly, 0.5*Lz]],
                    heater_points=[[0.5*L, 0.3*Ly, 0.98*Lz]])
    return g, c, p


def _model(tmp, nphase, save=False):
    from thermalporous_amd.singlephase import SinglePhase
    from thermalporous_amd.twophase import TwoPhase
    g, c, p = _geo_case(nphase)
    kw = dict(end=0.004, maxdt=0.002, small_dt_start=False, filename=os.path.join(tmp, "run%d.txt" % nphase), verbosity=False,
              save=save, n_save=1)
    if nphase == 2:
        return TwoPhase(g, c, p, solver_parameters="pc_cptr", **kw), p
    return SinglePhase(g, c, p, solver_parameters="pc_fieldsplit_cd", **kw), p


@pytest.mark.parametrize("nphase", [2, 1], ids=["TwoPhase", "SinglePhase"])
def test_two_time_steps_against_the_graded_oracle(tmp_path, nphase):
    from thermalporous_amd import utils
    from thermalporous_amd.problem import _flat
    m, p = _model(str(tmp_path), nphase)
    g = m.geo
    assert "hs" in m.spec and m.engine.spacing is not None and m.engine.spacing_info()["graded"]
    assert m.spec["axes"] == (2, 1, 0) and np.array_equal(m.spec["hs"][0], g.cell_widths()[2])
    # the sources sit where the coordinates say on the graded grid
    edges = g.cell_edges()
    prod = np.asarray(m.case.deltas_prod.cells)
    assert np.all(prod % 6 == 0) and np.all(prod // 30 == 0) and abs(m.case.deltas_prod.weights.sum() - 1.0) < 1e-14
    assert edges[0][1] < g.Dx/2 and edges[2][1] < g.Dz/2                  # (thin cells: mean widths would name others)
    m.start()
    o = OracleEngine(m.spec, m.engine_opts)
    o.set_state(m._to_internal(m.u._read()))
    for step in range(2):
        dt = float(m.dt.values()[0])
        o.set_old(o.get_state())
        o.set_dt(dt)
        ro = o.newton_solve()
        if nphase == 2:
            o.clamp_saturation()
        nits, lits = m.step()
        assert m.failed_solves == 0 and m.dt_vec[-1] == dt            # the model solved the step the oracle solved
        print("step %d: oracle nits %d lits %d, model nits %d lits %d" % (step, ro["nits"], ro["lits"], nits, lits))
        assert ro["reason"] > 0 and nits == ro["nits"] and abs(lits - ro["lits"]) <= max(2, 0.1*ro["lits"])
        uo = o.get_state()
        uh = m._to_internal(m.u._read())
        assert rel2(uh[0], uo[0]) < 1e-8 and rel2(uh[1], uo[1]) < 1e-8
        if nphase == 2:
            assert np.abs(uh[2] - uo[2]).max() < 1e-8
    assert m.failed_solves == 0 and len(m.dt_vec) == 2
    if nphase == 2:
        # oil in place, summed with the cells' own volumes, against the reference's state
        uo = m._from_internal(o.get_state())
        vol = utils.cell_volume(g)
        want = float(np.sum(_flat(g.phi, g)*uo[2]*p.oil_rho(uo[0], uo[1])*vol))
        mean = float(np.sum(_flat(g.phi, g)*uo[2]*p.oil_rho(uo[0], uo[1]))*g.Dx*g.Dy*g.Dz)
        print("oil in place %.9g, reference %.9g, with mean volumes %.9g" % (m.oil_mass(), want, mean))
        assert abs(m.oil_mass() - want) < 1e-8*want and abs(mean - want) > 1e-3*want
    m.finish()


def test_field_output_is_a_rectilinear_grid(tmp_path):
    from thermalporous_amd.output import read_vtr
    m, p = _model(str(tmp_path), 2, save=True)
    m.solve()
    files = sorted(glob.glob(os.path.join(str(tmp_path), "temperature_*.vtr")))
    assert len(files) == 3 and not glob.glob(os.path.join(str(tmp_path), "*.vti"))        # t = 0 and both steps
    name, vals, (x, y, z) = read_vtr(files[-1])
    ex, ey, ez = m.geo.cell_edges()
    assert name == "temperature" and np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(z, ez)
    assert np.array_equal(vals, m.u._read()[1])
    pvd = open(os.path.join(str(tmp_path), "saturation_o.pvd")).read()
    assert pvd.count(".vtr") == 3 and ".vti" not in pvd
