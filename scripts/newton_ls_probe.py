"""Probe of the Newton line search (engine key linesearch: basic | bt).  Every measurement is a child process of its own under its
own `timeout`, one after the other, and the script ends at the first one that fails:

  window   bench.py's time loop on one configuration (dt ramp, warm-up, a K-step window) once per line search from a fresh
           model: Newton steps/s, failed solves, residual evaluations (= trials) per Newton step, and how many Newton
           iterations accepted their first trial
  cold     the cold first time step at maxdt without the dt ramp (small_dt_start False): dt halvings and wall time
  trial    wall time of one trial as a sequence -- update, (exchange,) residual-only assembly, norm and its host wait --
           through tp_ls_trial + tp_residual on the state the window left (host time, not event time)

    python scripts/newton_ls_probe.py [--config c4] [--what window,cold,trial] [--steps 60] [--out profiles/newton_ls_probe_c4.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def counting(eng):
    """Accumulate the search's counters over every Newton solve of the engine."""
    tot = dict(trials=0, nonfinite=0, first_accepted=0, searches=0, failed_searches=0)
    inner = eng.newton_solve

    def newton_solve():
        r = inner()
        if eng.opts.get("linesearch") == "bt":
            h, li = eng.ls_history(), eng.ls_info()
            tot["trials"] += li["evaluations"]
            tot["nonfinite"] += li["nonfinite"]
            tot["searches"] += h["n"] + (1 if r["reason"] == -6 else 0)
            tot["first_accepted"] += sum(1 for t in h["trials"] if t == 1)
            tot["failed_searches"] += 1 if r["reason"] == -6 else 0
        return r
    eng.newton_solve = newton_solve
    return tot


def child(args):
    import torch
    import bench
    grid = tuple(args.grid) if args.grid else None
    if args.child == "cold":
        model = bench.make_model(args.config, Nxyz=grid, small_dt_start=False)
        eng = model.engine
        eng.set_options(linesearch=args.linesearch)
        tot = counting(eng)
        model.start()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        row = {"what": "cold", "config": args.config, "linesearch": args.linesearch, "maxdt_days": model.maxdt, "dt_halvings": model.failed_solves,
               "dt_days": model.dt_vec[0]/86400.0, "newton_its": model.total_nits, "linear_its": model.total_lits, "seconds": el, "search": tot}
        print(json.dumps(row), flush=True)
        eng.close()
        return
    model = bench.make_model(args.config, Nxyz=grid)
    eng = model.engine
    eng.set_options(linesearch=args.linesearch)
    tot = counting(eng)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    ramp = {"steps": len(model.dt_vec), "failed_solves": model.failed_solves, "solve_seconds": float(sum(model.timings)), "newton_its": model.total_nits}
    for _ in range(args.warmup):
        model.step()
    n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
    s0 = dict(tot)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    nits, lits = model.total_nits - n0, model.total_lits - l0
    w = {k: tot[k] - s0[k] for k in tot}
    row = {"what": "window", "config": args.config, "linesearch": args.linesearch, "steps": args.steps, "newton_its": nits, "linear_its": lits,
           "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el, "linear_its_per_s": lits/el, "seconds": el,
           "residual_evaluations_per_search": w["trials"]/max(w["searches"], 1), "search": w, "ramp": ramp, "ls_info": eng.ls_info()}
    print(json.dumps(row), flush=True)
    if args.child == "window+trial":
        import ctypes as C
        reps = 50
        u, d = eng.vec("ls_probe_u"), eng.vec("ls_probe_d")
        eng.vec_set("ls_probe_u", eng.get_state())
        nrm = C.c_double()
        eng._ck(eng.lib.tp_ls_trial(eng.ctx, u, d, C.c_double(0.5), u))          # (d = 0: the state does not move)
        eng._ck(eng.lib.tp_residual(eng.ctx, C.byref(nrm)))
        t0 = time.perf_counter()
        for _ in range(reps):
            eng._ck(eng.lib.tp_ls_trial(eng.ctx, u, d, C.c_double(0.5), u))
            eng._ck(eng.lib.tp_residual(eng.ctx, C.byref(nrm)))
        ms = 1e3*(time.perf_counter() - t0)/reps
        print(json.dumps({"what": "trial", "config": args.config, "reps": reps, "host_ms_per_trial": ms,
                          "assembly_fused_ms": eng.time_kernel(3, 20)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--what", default="window,cold,trial")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--limit", type=int, default=420, help="time limit (s) of every child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--linesearch", default="basic", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    what = args.what.split(",")
    jobs = []
    if "window" in what:
        jobs += [("window", "basic"), ("window+trial" if "trial" in what else "window", "bt")]
    if "cold" in what:
        jobs += [("cold", "basic"), ("cold", "bt")]
    lines = []
    for kind, ls in jobs:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", kind, "--linesearch", ls,
               "--config", args.config, "--steps", str(args.steps), "--warmup", str(args.warmup), "--spinup-cap", str(args.spinup_cap)]
        if args.grid:
            cmd += ["--grid"] + [str(v) for v in args.grid]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0:
            print("newton_ls_probe: %s/%s ended with status %d: stopping" % (kind, ls, r.returncode), file=sys.stderr)
            break
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if len(lines) >= len(jobs) else 1)


if __name__ == "__main__":
    main()
