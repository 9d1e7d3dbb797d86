"""Probe of the outer Krylov method (engine key ksp: fgmres | bcgs): for C4 and the presets pc_cptr and pc_cpr, runs bench.py's
time loop (dt ramp, warm-up, the 20-step window) once per method from a fresh model and prints one JSON line per row -- Newton
steps/s, linear iterations and preconditioner applications per Newton step, failed solves and the Krylov workspace tp_ksp_info
reports.  Preconditioner applications are derived from the linear iterations: an FGMRES iteration applies the preconditioner
once, a BiCGStab iteration twice (both applications of an iteration are enqueued before its one host wait, so a half-step exit
applies twice as well).  This holds for every preset and every s1_* / fs_* option; V-cycles per application do not enter.

    python scripts/bcgs_probe.py [--out profiles/bcgs_probe_c4.txt] [--presets pc_cptr,pc_cpr] [--methods fgmres,bcgs]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--presets", default="pc_cptr,pc_cpr")
    ap.add_argument("--methods", default="fgmres,bcgs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rows = []
    for preset in args.presets.split(","):
        for ksp in args.methods.split(","):
            model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=preset)
            eng = model.engine
            eng.set_options(ksp=ksp)
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
            applies = lits*(2 if ksp == "bcgs" else 1)
            info = eng.ksp_info()
            row = {"config": args.config, "preset": preset, "ksp": ksp, "steps": args.steps, "newton_its": nits, "linear_its": lits,
                   "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el, "linear_its_per_newton": lits/max(nits, 1),
                   "pc_applies_per_newton": applies/max(nits, 1), "ms_per_linear_it": 1e3*el/max(lits, 1),
                   "seconds": el, "ksp_info": info, "vector_bytes": eng.b*eng.ntot*8,
                   "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
            print(json.dumps(row), flush=True)
            rows.append(row)
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
