"""Probe of the Gram-Schmidt refinement of the outer FGMRES (engine key ksp_reorth): for one configuration and each preset, runs
bench.py's time loop (dt ramp, warm-up, the measured window) under each mode of --modes, alternating, `--repeats` times each,
every run from a fresh model, and prints one JSON line per run -- Newton steps/s, ms per linear iteration, linear iterations per
Newton step, failed solves and what tp_ksp_reorth_info counted over the measured window: orthogonalisation steps, second passes
executed and skipped, and the fraction of steps on which the criterion fired.  --kernels also times one Gram-Schmidt step
against 16 basis vectors under each mode on the run's own basis (tp_time_kernel 7, which goes through the solver's
orthogonalisation and therefore through the second pass the mode asks for; the steps it adds are not in the counts above).
Kernel names and per-kernel times come from a profiler run of its own, never together with the timings above:

    rocprofv3 --kernel-trace --stats -d OUTDIR -- python scripts/reorth_probe.py --config c4 --presets pc_cptr \
        --modes always --repeats 1 --steps 5 --warmup 1

    python scripts/reorth_probe.py [--config c4] [--presets pc_cptr] [--modes never,ifneeded,always] [--eta 0.7071] [--repeats 2]
                                   [--kernels] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def time_loop(args, preset, mode):
    import torch
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=preset)
    eng = model.engine
    eng.set_options(ksp_reorth=mode, ksp_reorth_eta=args.eta)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    for _ in range(args.warmup):
        model.step()
    n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
    i0 = eng.ksp_reorth_info()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    i1 = eng.ksp_reorth_info()
    nits, lits = model.total_nits - n0, model.total_lits - l0
    steps, refined, skipped = (i1[k] - i0[k] for k in ("steps", "refined", "skipped"))
    row = {"config": args.config, "preset": preset, "ksp_reorth": mode, "ksp_reorth_eta": args.eta, "steps": args.steps,
           "newton_its": nits, "linear_its": lits, "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el,
           "linear_its_per_newton": lits/max(nits, 1), "ms_per_linear_it": 1e3*el/max(lits, 1), "seconds": el,
           "orth_steps": steps, "second_passes": refined, "second_passes_skipped": skipped,
           "fraction_refined": refined/max(steps, 1), "whole_run": {"newton_its": model.total_nits, "linear_its": model.total_lits,
                                                                    "failed_solves": model.failed_solves, "reorth": i1},
           "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
    if args.kernels:
        row["gs16_ms"] = {}
        for m in ("never", "ifneeded", "always"):
            eng.set_options(ksp_reorth=m)
            row["gs16_ms"][m] = [eng.time_kernel(7, 200) for _ in range(3)]
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--presets", default="pc_cptr")
    ap.add_argument("--modes", default="never,ifneeded,always")
    ap.add_argument("--eta", type=float, default=2.0**-0.5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for preset in args.presets.split(","):
        for rep in range(args.repeats):
            for mode in args.modes.split(","):
                row = time_loop(args, preset, mode)
                row["repeat"] = rep
                print(json.dumps(row), flush=True)
                rows.append(row)
                if args.out:
                    with open(args.out, "w") as f:
                        for r in rows:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
