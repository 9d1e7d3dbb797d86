"""Probe of the composite preconditioner's stage orders (engine key pc_order): for one configuration and each preset, runs
bench.py's time loop (dt ramp, warm-up, the measured window) under each order of --orders, alternating, `--repeats` times each,
every run from a fresh model, and prints one JSON line per run -- Newton steps/s, Krylov iterations per Newton step, ms per
Krylov iteration, failed solves, and the device time of one preconditioner application under the order in force
(tp_time_kernel 4, three times `--reps` replays of the recorded program, after the window).  --kernels also times the one-launch
stage-1 right-hand side of a later S stage (tp_time_kernel 9) against the pair of launches it replaces (10: block residual over
all fields + the decoupled right-hand side per primary field) and that block residual alone (11), interleaved, on the run's own
Jacobian.  Kernel names and per-kernel times come from a profiler run of its own, never together with the timings above:

    rocprofv3 --kernel-trace --stats -d OUTDIR -- python scripts/pc_order_probe.py --config c4 --presets pc_cptr \
        --orders SIS --repeats 1 --steps 5 --warmup 1

    python scripts/pc_order_probe.py [--config c4] [--presets pc_cptr,pc_cpr] [--orders SI,IS,ISI,SIS] [--repeats 2] [--kernels]
                                     [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def time_loop(args, preset, order):
    import torch
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=preset)
    eng = model.engine
    eng.set_options(pc_order=order)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    for _ in range(args.warmup):
        model.step()
    n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    nits, lits = model.total_nits - n0, model.total_lits - l0
    row = {"config": args.config, "preset": preset, "pc_order": order, "steps": args.steps,
           "newton_its": nits, "linear_its": lits, "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el,
           "linear_its_per_newton": lits/max(nits, 1), "ms_per_linear_it": 1e3*el/max(lits, 1), "seconds": el,
           "pc_apply_ms": [eng.time_kernel(4, args.reps) for _ in range(3)],
           "whole_run": {"newton_its": model.total_nits, "linear_its": model.total_lits, "failed_solves": model.failed_solves},
           "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
    if args.kernels:
        row["stage_rhs_ms"] = {"one_launch": [], "pair": [], "block_residual_alone": []}
        for _ in range(5):                                   # interleaved: the three see the same clocks
            for key, which in (("one_launch", 9), ("pair", 10), ("block_residual_alone", 11)):
                row["stage_rhs_ms"][key].append(eng.time_kernel(which, args.reps))
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--presets", default="pc_cptr,pc_cpr")
    ap.add_argument("--orders", default="SI,IS,ISI,SIS")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for preset in args.presets.split(","):
        for rep in range(args.repeats):
            for order in args.orders.split(","):
                row = time_loop(args, preset, order)
                row["repeat"] = rep
                print(json.dumps(row), flush=True)
                rows.append(row)
                if args.out:
                    with open(args.out, "w") as f:
                        for r in rows:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
