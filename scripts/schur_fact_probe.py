"""Probe of the factorisation types of the Schur split on (p,T) (engine keys schur_fact / schur_scale): for one
configuration and each preset, runs bench.py's time loop (dt ramp, warm-up, the measured window) under each factorisation of
--facts, alternating, `--repeats` times each, every run from a fresh model in this one process, and prints one JSON line per run
-- Newton steps/s, Krylov iterations per Newton step, ms per Krylov iteration, failed solves, the K(A00) / K(S) applications the
library counted for the last set-up (tp_schur_info), and the device time of one preconditioner application under the
factorisation in force (tp_time_kernel 4, three times `--reps` replays of the recorded program, after the window).  --opt passes
further engine options to every run (an inner pressure solve: --opt s1_ksp=fgmres --opt s1_max_it=4).

    python scripts/schur_fact_probe.py [--config c4] [--presets pc_cptr] [--facts full,lower,upper,diag] [--repeats 2]
                                       [--opt KEY=VALUE ...] [--out FILE]
"""
import argparse
import ast
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def parse_opts(pairs):
    out = {}
    for kv in pairs:
        k, v = kv.split("=", 1)
        try:
            out[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            out[k] = v
    return out


def time_loop(args, preset, fact, extra):
    import torch
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=preset)
    eng = model.engine
    eng.set_options(schur_fact=fact, **extra)
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
    info = eng.schur_info()
    row = {"config": args.config, "preset": preset, "schur_fact": fact, "options": extra, "steps": args.steps,
           "newton_its": nits, "linear_its": lits, "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el,
           "linear_its_per_newton": lits/max(nits, 1), "ms_per_linear_it": 1e3*el/max(lits, 1), "seconds": el,
           "schur_info_last_setup": info,
           "pc_apply_ms": [eng.time_kernel(4, args.reps) for _ in range(3)],
           "whole_run": {"newton_its": model.total_nits, "linear_its": model.total_lits, "failed_solves": model.failed_solves},
           "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
    if extra.get("s1_ksp", "preonly") != "preonly":
        applies, its, unconv = eng.inner_stats()
        row["inner_last_setup"] = {"solves": applies, "its": its, "above_tolerance": unconv}
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--presets", default="pc_cptr")
    ap.add_argument("--facts", default="full,lower,upper,diag")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    extra = parse_opts(args.opt)
    rows = []
    for preset in args.presets.split(","):
        for rep in range(args.repeats):
            for fact in args.facts.split(","):
                row = time_loop(args, preset, fact, extra)
                row["repeat"] = rep
                print(json.dumps(row), flush=True)
                rows.append(row)
                if args.out:
                    with open(args.out, "w") as f:
                        for r in rows:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
