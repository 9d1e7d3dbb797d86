"""Regenerates problem_vectors.npz: what the CPU oracle's TPFA problem (oracle/tpfa.py) computes for every combination of graded
widths ("hs"), Dirichlet sides ("boundary"), saturation functions ("satfn") and completed wells ("wells") on small seeded boxes.

What the fixture is for: the committed file was written from the separate reference classes that tests/ held per feature and per
pair of features, before they became the one ``oracle.tpfa.Problem``; tests/test_problem_vectors.py holds the one class to it.
The problems are built through ``edge_cases.combo_problem`` and ``wells_ref.wells_problem`` only, so that this script runs
unchanged on either side of that change.

Per case: state u = perturbed_state(seed 3), old state = perturbed_state(seed 5), dt = 8640 -> R, J (7, b, b, ...), S~, last_flux
(6, b; zeros without sides) and, with wells, per well its bhp, its perforation rates q and the rank-1 factors c, b.
usage: python tests/golden/make_problem_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

import cases                                                        # noqa: E402
from bc_ref import assert_both_directions, make_boundary            # noqa: E402
from edge_cases import combo_problem                                # noqa: E402
from graded_ref import random_widths, spec_lengths                  # noqa: E402
from satfn_ref import M3                                            # noqa: E402
from wells_ref import line_cells, make_well, tune_wells, wells_problem   # noqa: E402

DT = 8640.0
BOX3 = (cases.c4_spe10_3d, dict(Nx=3, Ny=4, Nz=5))
BOX2 = (cases.c3_spe10_2d, dict(Nx=5, Ny=4))
SIDES3 = {0: "open", 1: "thermal", 2: "open", 3: "open", 4: "thermal", 5: "open"}
SIDES2 = {0: "open", 1: "open", 2: "thermal", 3: "open"}


def _cases():
    out = {}
    for nphase, keysets in ((1, [(h, b, False) for h in (False, True) for b in (False, True)]),
                            (2, [(h, b, s) for h in (False, True) for b in (False, True) for s in (False, True)])):
        for hs, bnd, sat in keysets:
            tag = "".join(t for t, on in (("_hs", hs), ("_bc", bnd), ("_sat", sat)) if on) or "_plain"
            out["c4_%dph%s" % (nphase, tag)] = (BOX3, nphase, hs, bnd, sat, False)
    out["c3_2ph_hs_bc"] = (BOX2, 2, True, True, False, False)
    out["wells_1ph_plain"] = (BOX3, 1, False, False, False, True)
    out["wells_2ph_hs_bc"] = (BOX3, 2, True, True, False, True)
    out["wells_2ph_sat"] = (BOX3, 2, False, False, True, True)
    out["wells_2ph_hs_bc_sat"] = (BOX3, 2, True, True, True, True)
    return out


ALL_CASES = _cases()


def build(name):
    """(problem with old state and dt set, state u) of one case."""
    (builder, kw), nphase, hs, bnd, sat, wells = ALL_CASES[name]
    spec, *_ = builder(nphase=nphase, **kw)
    spec = dict(spec)
    u, u_old = cases.perturbed_state(spec, seed=3), cases.perturbed_state(spec, seed=5)
    if hs:
        spec["hs"] = random_widths(spec["n"], spec_lengths(spec), seed=4)
    if bnd:
        spec["boundary"] = make_boundary(spec, u, SIDES3 if spec["n"][2] > 1 else SIDES2, seed=6)
    if sat:
        spec["satfn"] = dict(M3)
    if not wells:
        P = combo_problem(spec)
    else:
        if sat:                                                     # inside the mobile range of M3
            u[2], u_old[2] = np.clip(u[2], 0.25, 0.8), np.clip(u_old[2], 0.25, 0.8)
        n = spec["n"]
        ws = [make_well(spec, "P", "prod", line_cells(spec, 0, (2, 3)), 0, 1.0, 1.0, spec.get("hs")),
              make_well(spec, "I", "inj", line_cells(spec, 0, (0, 2), n[0] - 2, n[0] - 1), 0, 1.0, 1.0, spec.get("hs"))]
        P = wells_problem(spec, wells=ws)
        P.set_dt(DT)
        spec["wells"] = tune_wells(P, u, ws, {"P": ("rate", 0.3), "I": ("rate", 0.3)})
    P.set_old(u_old)
    P.set_dt(DT)
    return P, u


def compute(name):
    P, u = build(name)
    wells = ALL_CASES[name][-1]
    out = {"R": P.residual(u)}
    if P.spec.get("boundary"):
        assert_both_directions(P)
    out["J"], out["Sm"] = P.jacobian(u, want_schur=True)
    P.residual(u)
    out["last_flux"] = np.array(getattr(P, "last_flux", np.zeros((6, P.b))))      # (the classes without sides had none)
    if wells:
        st = P.well_state(u)
        assert [s["mode"] for s in st] == ["rate", "rate"] and not st[0]["open"].all() and st[0]["open"].sum() >= 2
        assert len(P.wells[0]["cells"]) > 1 and len(P.wells[1]["cells"]) == 1
        for i, (s, (cf, bf)) in enumerate(zip(st, P.last_factors)):
            out["well%d_bhp" % i] = np.float64(np.real(s["bhp"]))
            out["well%d_q" % i] = np.array(np.real(s["q"]))
            out["well%d_c" % i], out["well%d_b" % i] = np.array(cf), np.array(bf)
    return out


if __name__ == "__main__":
    blob = {}
    for name in ALL_CASES:
        for k, v in compute(name).items():
            blob[name + "/" + k] = v
    path = os.path.join(HERE, "problem_vectors.npz")
    np.savez_compressed(path, **blob)
    print("wrote problem_vectors.npz", len(blob), "arrays,", os.path.getsize(path), "bytes")
