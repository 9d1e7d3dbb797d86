"""Krylov counts of the numpy reference with line relaxation (amg_line_levels = 0..3): one right-preconditioned FGMRES solve of
the Jacobian system at a perturbed state, pc_cptr, on a C5-shaped box (the x4-refined SPE10-like field, 120x56x84) and on a
C4-shaped reduced box.  No GPU: tests/amg_line_ref.LineSemiAMG inside the oracle's TwoStagePC.

    python scripts/amg_line_study.py [--case c5|c4|both] [--levels 0,1,2,3] [--dt 8640]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                  # noqa: E402
from amg_line_ref import oracle_engine        # noqa: E402
import oracle.linalg as la                    # noqa: E402

SIZES = {"c5": ("c5slab", (120, 56, 84)), "c4": ("c4", (30, 55, 43))}


def spec_of(case):
    from bench import build_case
    from thermalporous_amd.problem import build_spec
    name, n = SIZES[case]
    params, geo, wells, _, _ = build_case(name, n)
    spec = build_spec(geo, wells, params, 2)
    return spec, cases.uniform_state(spec, params.p_ref, params.T_prod, params.S_o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both")
    ap.add_argument("--levels", default="0,1,2,3")
    ap.add_argument("--dt", type=float, default=8640.0)
    a = ap.parse_args()
    for case in (("c5", "c4") if a.case == "both" else (a.case,)):
        spec, u0 = spec_of(case)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        for L in (int(v) for v in a.levels.split(",")):
            o = oracle_engine(spec, dict(pc="cptr", amg_line_levels=L))
            o.set_old(u0)
            o.set_dt(a.dt)
            o.set_state(u)
            F = o.residual()
            J, Sm = o.jacobian(want_schur=True)
            t0 = time.time()
            x, its, reason, hist = o.linear_solve(J, Sm, F)
            print("%s n=%r dt=%g amg_line_levels=%d: line levels p/T %d/%d, FGMRES its %d, reason %d, %.0f s"
                  % (case, tuple(spec["n"]), a.dt, L, o.pc.amg_p.n_line_levels(), o.pc.amg_T.n_line_levels(), its, reason,
                     time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
