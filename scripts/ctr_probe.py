"""Probe of the composite's temperature stage (engine key pc_ctr): for one configuration and preset, runs bench.py's time loop (dt
ramp, warm-up, the measured window) with the stage off and on, alternating, `--repeats` times each, every run from a fresh
model, and prints one JSON line per run -- Newton steps/s, Krylov iterations per Newton iteration, V-cycles, failed solves, and
the device time of one preconditioner application (tp_time_kernel 4, three times `--reps` replays of the recorded program, after
the window).  --kernels also times, on the run's own Jacobian and interleaved, the T stage's row right-hand side (tp_time_kernel
12, k_row_rhs) against the one-launch stage-1 right-hand side of a later S stage (9, k_stage_rhs: with pc_cpr and decoupling No
the same number of Jacobian planes).

    python scripts/ctr_probe.py [--config c4] [--preset pc_cpr] [--order SI] [--repeats 2] [--kernels] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def time_loop(args, ctr):
    import torch
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=args.preset)
    eng = model.engine
    eng.set_options(pc_order=args.order, pc_ctr=ctr)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    for _ in range(args.warmup):
        model.step()
    n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
    v0 = eng.last.get("vcycles", 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    nits, lits = model.total_nits - n0, model.total_lits - l0
    row = {"config": args.config, "preset": args.preset, "pc_order": args.order, "pc_ctr": ctr, "steps": args.steps,
           "newton_its": nits, "linear_its": lits, "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el,
           "linear_its_per_newton": lits/max(nits, 1), "ms_per_linear_it": 1e3*el/max(lits, 1), "seconds": el,
           "vcycles": eng.last.get("vcycles", 0) - v0,
           "pc_apply_ms": [eng.time_kernel(4, args.reps) for _ in range(3)],
           "whole_run": {"newton_its": model.total_nits, "linear_its": model.total_lits, "failed_solves": model.failed_solves},
           "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
    if ctr:
        row["ctr_info"] = eng.ctr_info()
    if args.kernels and ctr:
        row["rhs_ms"] = {"row_rhs": [], "stage_rhs": []}
        for _ in range(5):                                   # interleaved: the two see the same clocks
            for key, which in (("row_rhs", 12), ("stage_rhs", 9)):
                row["rhs_ms"][key].append(eng.time_kernel(which, args.reps))
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--preset", default="pc_cpr")
    ap.add_argument("--order", default="SI")
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
    for rep in range(args.repeats):
        for ctr in (False, True):
            row = time_loop(args, ctr)
            row["repeat"] = rep
            print(json.dumps(row), flush=True)
            rows.append(row)
            if args.out:
                with open(args.out, "w") as f:
                    for r in rows:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
