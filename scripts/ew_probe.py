"""Probe of the Eisenstat-Walker inexact Newton (engine key ksp_ew: off | 1 | 2).  The time loop of one configuration from its cold
start -- the reference's dt ramp included, which is where extra Newton iterations slow the growth of dt -- once per setting: off,
and versions 1 and 2 at ew_rtol0 0.3, 0.1 and 0.01.  Every setting is a child process of its own under its own `timeout`, one
after the other, and the script ends at the first one that fails.

Per time step a child prints dt (days), Newton iterations, Krylov iterations per linear solve, eta per linear solve (under the
option), wall ms and failed solves so far; at the end one JSON line with the totals and the simulated days per wall second.

    python scripts/ew_probe.py [--config c4] [--steps 40] [--out profiles/ew_probe_c4.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SETTINGS = [(0, 0.3)] + [(v, r0) for v in (1, 2) for r0 in (0.3, 0.1, 0.01)]


def child(args):
    import torch
    import bench
    grid = tuple(args.grid) if args.grid else None
    model = bench.make_model(args.config, Nxyz=grid)
    eng = model.engine
    if args.version:
        eng.set_options(ksp_ew=args.version, ew_rtol0=args.rtol0)
    solves = []                        # (eta per linear solve, Krylov iterations per linear solve, reason) of every Newton solve
    inner = eng.newton_solve

    def newton_solve():
        r = inner()
        h = eng.ew_history()
        solves.append(([float(v) for v in h["rtol"]], h["kits"] if h["n"] else [r["lits"]], r["reason"]))
        return r
    eng.newton_solve = newton_solve
    tag = "off" if not args.version else "v%d rtol0 %g" % (args.version, args.rtol0)
    model.start()
    for i in range(args.steps):
        if model.t >= model.end*86400.0:
            break
        del solves[:]
        torch.cuda.synchronize()
        model.step()
        torch.cuda.synchronize()
        eta, kits, _ = solves[-1]
        print("%s step %3d dt %.5g d  Newton %2d  Krylov %s%s  %.1f ms  failed solves %d" %
              (tag, i + 1, model.dt_vec[-1]/86400.0, model.nits_vec[-1], kits if args.version else "%d in all" % model.lits_vec[-1],
               "  eta " + " ".join("%.2g" % v for v in eta) if eta else "", 1e3*model.timings[-1], model.failed_solves), flush=True)
    wall = float(sum(model.timings))
    row = {"config": args.config, "ksp_ew": args.version, "ew_rtol0": args.rtol0 if args.version else None, "steps": len(model.dt_vec),
           "newton_its": model.total_nits, "krylov_its": model.total_lits, "failed_solves": model.failed_solves,
           "dt_last_days": model.dt_vec[-1]/86400.0, "simulated_days": model.t/86400.0, "solve_seconds": wall,
           "ms_per_step": 1e3*wall/max(len(model.dt_vec), 1), "simulated_days_per_wall_second": model.t/86400.0/wall, "ew_info": eng.ew_info()}
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--limit", type=int, default=240, help="time limit (s) of every child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--version", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rtol0", type=float, default=0.3, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.version is not None:
        child(args)
        return
    text, done = [], 0
    for version, rtol0 in SETTINGS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--version", str(version), "--rtol0", str(rtol0),
               "--config", args.config, "--steps", str(args.steps)]
        if args.grid:
            cmd += ["--grid"] + [str(v) for v in args.grid]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        text.append(r.stdout)
        if r.returncode != 0:
            print("ew_probe: version %d rtol0 %g ended with status %d: stopping" % (version, rtol0, r.returncode), file=sys.stderr)
            break
        done += 1
    if args.out and text:
        with open(args.out, "w") as f:
            f.write("".join(text))
    sys.exit(0 if done == len(SETTINGS) else 1)


if __name__ == "__main__":
    main()
