"""Probe of the red-black Gauss-Seidel smoother (engine keys amg_gs_levels = L, amg_gs_sweeps = g) on one GPU.  Every variant --
option off, then L in --levels x g in --sweeps -- is a child process of its own under its own `timeout`, one after the other, and
the script ends at the first one that fails.  Per variant, bench.py's time loop on one configuration (dt ramp, warm-up, a K-step
window) from a fresh model:

  vcycle_ms / pc_apply_ms   pressure V-cycle and pc_apply through the tp_time_kernel hooks, on the Jacobian the window left
  its_per_newton            Krylov iterations per Newton step of the window
  newton_per_s              Newton steps/s of the window (wall time, failed solves' time included)
  failed_solves             of the window (and of the ramp)

    python scripts/amg_gs_probe.py [--config c4|c5slab] [--levels 1,2,3] [--sweeps 1,2] [--steps 20] [--out profiles/amg_gs_probe_c4.txt]

The level-0 half-sweep alone is read from a kernel trace of one child (rocprofv3 --kernel-trace --stats -- python
scripts/amg_gs_probe.py --child --gs-levels 3 ...): k_amg_gs_half beside k_amg_jacobi, which levels >= L of the same cycle still run,
and beside the option-off child's k_amg_jacobi of level 0."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def child(args):
    import torch
    import bench
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None)
    eng = model.engine
    if args.gs_levels:
        eng.set_options(amg_gs_levels=args.gs_levels, amg_gs_sweeps=args.gs_sweeps)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    ramp = {"steps": len(model.dt_vec), "failed_solves": model.failed_solves, "newton_its": model.total_nits, "linear_its": model.total_lits}
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
    row = {"config": args.config, "n": [int(v) for v in eng.spec["n"]], "amg_gs_levels": args.gs_levels, "amg_gs_sweeps": args.gs_sweeps,
           "gs_info": eng.amg_gs_info(0), "steps": args.steps, "newton_its": nits, "linear_its": lits,
           "its_per_newton": lits/max(nits, 1), "newton_per_s": nits/el, "failed_solves": model.failed_solves - f0, "seconds": el,
           "vcycle_ms": eng.time_kernel(2, args.reps), "pc_apply_ms": eng.time_kernel(4, args.reps), "ramp": ramp}
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--levels", default="1,2,3")
    ap.add_argument("--sweeps", default="1,2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--limit", type=int, default=240, help="time limit (s) of every child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gs-levels", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--gs-sweeps", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    jobs = [(0, 1)] + [(int(L), int(g)) for L in args.levels.split(",") if L for g in args.sweeps.split(",")]
    lines = []
    for L, g in jobs:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--gs-levels", str(L),
               "--gs-sweeps", str(g), "--config", args.config, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--reps", str(args.reps), "--spinup-cap", str(args.spinup_cap)]
        if args.grid:
            cmd += ["--grid"] + [str(v) for v in args.grid]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0:
            print("amg_gs_probe: L=%d g=%d ended with status %d: stopping" % (L, g, r.returncode), file=sys.stderr)
            break
        if args.out:                               # (rewritten after every variant: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    sys.exit(0 if len(lines) >= len(jobs) else 1)


if __name__ == "__main__":
    main()
