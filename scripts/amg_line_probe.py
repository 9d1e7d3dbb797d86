"""Timings of the line relaxation on one GPU (amg_line_levels off and on): pressure V-cycle and pc_apply through the
tp_time_kernel hooks, set-up time, and the factor-stream bytes, on C4 (60x220x85) or the config-5 slab.

    python scripts/amg_line_probe.py [--config c4|c5slab] [--levels 0,1,2] [--reps 50]

The level-0 sweep alone is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats): k_amg_line_sweep beside
k_amg_jacobi of the same level."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--levels", default="0,1,2")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from bench import build_case
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.problem import build_spec
    params, geo, wells, _, _ = build_case(a.config)
    spec = build_spec(geo, wells, params, 2)
    u0 = cases.uniform_state(spec, params.p_ref, params.T_prod, params.S_o)
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    for L in (int(v) for v in a.levels.split(",")):
        h = HipEngine(spec, dict(pc="cptr", amg_line_levels=L))
        h.set_old(u0)
        h.set_dt(8640.0)
        h.set_state(u)
        h.jacobian()
        h.pc_setup()
        out = dict(config=a.config, n=list(spec["n"]), amg_line_levels=L, line_info=h.amg_line_info(0),
                   vcycle_ms=h.time_kernel(2, a.reps), pc_apply_ms=h.time_kernel(4, a.reps), pc_setup_ms=h.time_kernel(5, 10))
        print(json.dumps(out), flush=True)
        h.close()


if __name__ == "__main__":
    main()
