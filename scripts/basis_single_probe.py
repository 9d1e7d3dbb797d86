"""Probe of the fp32 FGMRES bases (engine key ksp_basis_single): for one configuration and each preset, runs bench.py's time loop
(dt ramp, warm-up, the measured window) with the option off and on, alternating, `--repeats` times each, every run from a
fresh model, and prints one JSON line per run -- Newton steps/s, linear iterations and restart cycles per Newton step, failed
solves and the Krylov workspace tp_ksp_info reports.  Cycles: tp_ksp_basis_info holds the cycle count of the LAST linear
solve, so the probe reads it after every Newton solve (it wraps the engine's newton_solve) and reports the mean over Newton
solves of that last linear solve's cycles -- one linear solve per Newton solve is sampled, the final and tightest one -- next to
linear iterations per Newton step, which are exact.  --kernels also times one Gram-Schmidt step against 16 basis vectors in
both representations in one process (tp_time_kernel 7 against 8).  Kernel names and per-kernel times come from a profiler run
of its own, never together with the timings above:

    rocprofv3 --kernel-trace --stats -d OUTDIR -- python scripts/basis_single_probe.py --config c4 --presets pc_cptr \
        --repeats 1 --steps 5 --warmup 1

    python scripts/basis_single_probe.py [--config c4] [--presets pc_cptr,pc_cpr] [--repeats 2] [--kernels] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def time_loop(args, preset, single):
    import torch
    model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, solver_parameters=preset)
    eng = model.engine
    eng.set_options(ksp_basis_single=single)
    model.start()
    bench.spin_up(model, args.spinup_cap)
    for _ in range(args.warmup):
        model.step()
    n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
    cycles = []
    solve = eng.newton_solve

    def counted():
        r = solve()
        cycles.append(eng.ksp_basis_info()["cycles"])
        return r
    eng.newton_solve = counted
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    nits, lits = model.total_nits - n0, model.total_lits - l0
    row = {"config": args.config, "preset": preset, "ksp_basis_single": bool(single), "steps": args.steps, "newton_its": nits,
           "linear_its": lits, "failed_solves": model.failed_solves - f0, "newton_per_s": nits/el,
           "linear_its_per_newton": lits/max(nits, 1), "cycles_of_last_linear_solve_per_newton_solve": sum(cycles)/max(len(cycles), 1),
           "ms_per_linear_it": 1e3*el/max(lits, 1), "seconds": el, "ksp_info": eng.ksp_info(), "basis_info": eng.ksp_basis_info(),
           "vector_bytes": eng.b*eng.ntot*8, "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}
    if args.kernels:
        # one Gram-Schmidt step against 16 vectors, the representation this run has a basis of, then the other one in the same
        # process (a few forced iterations give it 17 vectors)
        row["gs16_ms"] = {}
        for rep in (single, not single):
            if rep != single:
                eng.set_options(ksp_basis_single=rep, ksp_rtol=1e-30, ksp_atol=1e-300, ksp_max_it=20)
                eng.jacobian()
                eng.residual()
                eng.pc_setup()
                eng.copy_residual_to("probe_b")
                eng.fgmres("probe_b", "probe_x")
            which = 8 if rep else 7
            row["gs16_ms"]["fp32" if rep else "fp64"] = [eng.time_kernel(which, 200) for _ in range(3)]
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--presets", default="pc_cptr,pc_cpr")
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
            for single in (False, True):
                row = time_loop(args, preset, single)
                row["repeat"] = rep
                print(json.dumps(row), flush=True)
                rows.append(row)
                if args.out:
                    with open(args.out, "w") as f:
                        for r in rows:
                            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
