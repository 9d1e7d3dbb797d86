"""Dirichlet sides in the time loop: ``geo.set_boundary`` -> model -> engine, the ``boundary_energy`` entry of ``rates()`` under
the physical side names, the log line, ``model.set_boundary`` between two steps, the example script, and a results file that does
not change when no boundary is set."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(tmp, name, boundary, Nx=7, Ny=5, Nz=4, verbosity=True):
    """c4 at test size (Ny < Nx: internal axes (z, y, x), so 'x+' is internal side 5 and 'z-' side 0), two steps of 0.002 d."""
    from thermalporous_amd.twophase import TwoPhase
    spec, u0, p, g, c = cases.c4_spe10_3d(Nx=Nx, Ny=Ny, Nz=Nz, nphase=2)
    boundary(g, p)
    return TwoPhase(g, c, p, end=0.004, maxdt=0.002, small_dt_start=False, solver_parameters="pc_cptr",
                    filename=os.path.join(tmp, name + ".txt"), verbosity=verbosity), p


def _hot_floor(g, p):
    g.set_boundary("z-", "thermal", T=p.T_prod + 60.0)
    g.set_boundary("x+", "open", p=p.p_ref, T=p.T_prod, S=p.S_o)


def _layers(m, N):
    """Mean temperature of the physical bottom and top layers of cells."""
    T = np.asarray(m.u.dat.data_ro[1]).reshape(N[2], N[1], N[0])          # x fastest
    return T[0].mean(), T[-1].mean()


def _stable(text):
    """A log or results file without the lines that carry wall-clock figures."""
    skip = ("timings", "Total CPU time", "per second")
    return [ln for ln in text.splitlines() if not any(k in ln for k in skip)]


def test_rates_report_the_energy_flux_under_physical_side_names(tmp_path, capsys):
    N = (7, 5, 4)
    m, p = _model(str(tmp_path), "hot", _hot_floor)
    assert m.spec["axes"] == (2, 1, 0) and sorted(m.spec["boundary"]) == [0, 5]
    assert m.spec["boundary"][0]["kind"] == "thermal" and m.spec["boundary"][5]["kind"] == "open"
    m.solve()
    r = m.rates()
    flux = m.engine.boundary_flux()
    assert set(r) == {"inj", "prod", "water", "oil", "boundary_energy"}
    assert r["boundary_energy"] == {"z-": flux[0, 1], "x+": flux[5, 1]}
    assert np.all(flux[1:5] == 0.0)
    assert r["boundary_energy"]["z-"] < 0.0                         # a floor 60 K hotter than the rock: heat enters
    out = capsys.readouterr().out
    nz = out.count("Energy flux through side  z-  is ")          # one line per side and time step
    assert nz == len(m.dt_vec) >= 2 and out.count("Energy flux through side  x+  is ") == nz
    # the physical side: against the closed box the bottom layer of cells has warmed, the top layer has not
    m0, _ = _model(str(tmp_path), "closed", lambda g, p: None, verbosity=False)
    m0.solve()
    (b1, t1), (b0, t0) = _layers(m, N), _layers(m0, N)
    print("bottom layer %.6f against %.6f closed, top layer %.6f against %.6f" % (b1, b0, t1, t0))
    assert b1 - b0 > 1e-3 and abs(t1 - t0) < 0.05*(b1 - b0)
    assert m0.rates().keys() == {"inj", "prod", "water", "oil"}


def test_model_set_boundary_between_two_steps(tmp_path):
    m, p = _model(str(tmp_path), "switch", _hot_floor, verbosity=False)
    m.start()
    m.step()
    assert m.rates()["boundary_energy"]["z-"] < 0.0
    m.set_boundary("z-", "thermal", T=p.T_prod - 60.0)               # now a cold floor: heat leaves
    assert np.all(m.spec["boundary"][0]["T"] == p.T_prod - 60.0) and np.all(m.engine.boundary[0]["T"] == p.T_prod - 60.0)
    m.step()
    r = m.rates()["boundary_energy"]
    assert set(r) == {"z-", "x+"} and r["z-"] > 0.0
    m.set_boundary("x+", "none")
    assert sorted(m.engine.boundary) == [0] and sorted(m.spec["boundary"]) == [0]
    m.step()
    assert set(m.rates()["boundary_energy"]) == {"z-"}
    with pytest.raises(ValueError, match="unknown side"):
        m.set_boundary("w+", "thermal", T=300.0)
    m.finish()


def test_log_and_results_file_do_not_change_without_a_boundary(tmp_path, capsys):
    """A geo on which a side was set and removed again, and one that never heard of boundaries: the same log and the same results
    file, but for the lines that carry wall-clock figures; and no word of a boundary in either."""
    def set_and_remove(g, p):
        g.set_boundary("z-", "thermal", T=p.T_prod + 60.0)
        g.set_boundary("z-", "none")
    texts = []
    for name, b in (("plain", lambda g, p: None), ("removed", set_and_remove)):
        m, _ = _model(str(tmp_path), name, b)
        assert "boundary" not in m.spec
        m.solve()
        texts.append((capsys.readouterr().out, open(os.path.join(str(tmp_path), name + ".txt")).read()))
    for k in range(2):
        assert _stable(texts[0][k]) == _stable(texts[1][k]) and len(_stable(texts[0][k])) > 10
        assert "Energy flux" not in texts[0][k] and "boundary" not in texts[0][k]


def test_the_example_runs():
    script = os.path.join(ROOT, "examples", "test3D_heaters_thermal_walls.py")
    res = os.path.splitext(script)[0] + "_cptr_results.txt"
    r = subprocess.run([sys.executable, script, "cptr", "0.1", "0.2", "6", "6", "4"], capture_output=True, text=True, timeout=120)
    try:
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Energy flux through side  z-  is " in r.stdout and "Energy flux through side  z+  is " in r.stdout
        assert "failed solves 0" in r.stdout and "energy leaving through the walls at the last assembly: {'z-': " in r.stdout
    finally:
        if os.path.exists(res):
            os.remove(res)
