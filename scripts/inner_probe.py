"""Probe of the inner stage-1 solve (tp_options.s1_ksp): for ONE configuration and preset, runs bench.py's time loop (dt ramp,
warm-up, timed steps) once per setting and prints one JSON line per setting -- outer FGMRES iterations per Newton step, inner
iterations per outer iteration, failed solves, ms per outer iteration and Newton steps/s.

    python scripts/inner_probe.py --config c4 --preset pc_cptr --settings "preonly;richardson:2;fgmres:4:1e-2;fgmres:32:1e-8"

A setting is  preonly | richardson:K | fgmres:K[:RTOL].  Every setting starts from a fresh model, so the rows are independent.
--shared-ramp (for configurations whose dt ramp takes minutes, c5slab): ONE model, the ramp once with preonly, then the
settings one after the other on consecutive windows of the same trajectory (warm-up + timed steps each): the rows then
see different time steps of the same regime.
Inner counts come from tp_inner_stats, which counts since the last PC set-up: they are sampled after every time step (the
last linear solve of the step), and they count every application that was launched, the one speculative application per
linear solve that the pipelined outer loop discards included: "inner per outer" is inner iterations per inner solve times
the inner solves per application (2 for pc_cptr / pc_fieldsplit_cd), which that extra application does not distort."""
import argparse
import ast
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench          # noqa: E402


def parse(s):
    p = s.split(":")
    if p[0] == "preonly":
        return dict(s1_ksp="preonly", s1_max_it=1, s1_rtol=0.0)
    if p[0] == "richardson":
        return dict(s1_ksp="richardson", s1_max_it=int(p[1]), s1_rtol=0.0)
    if p[0] == "fgmres":
        return dict(s1_ksp="fgmres", s1_max_it=int(p[1]), s1_rtol=float(p[2]) if len(p) > 2 else 0.0)
    raise SystemExit("setting %r: preonly | richardson:K | fgmres:K[:RTOL]" % s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--preset", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spinup-cap", type=int, default=80)
    ap.add_argument("--grid", type=int, nargs=3, default=None)
    ap.add_argument("--settings", default="preonly;richardson:2;fgmres:4:1e-2;fgmres:32:1e-8")
    ap.add_argument("--shared-ramp", action="store_true", help="one model and one preonly dt ramp for all settings")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="further engine options (e.g. amg_gather_cells=-1)")
    args = ap.parse_args()
    import torch
    extra = {}
    for kv in args.opt:
        k, v = kv.split("=", 1)
        extra[k] = ast.literal_eval(v)
    model = None
    for setting in args.settings.split(";"):
        s1 = parse(setting)
        if model is None or not args.shared_ramp:
            over = {"solver_parameters": args.preset} if args.preset else {}
            model = bench.make_model(args.config, Nxyz=tuple(args.grid) if args.grid else None, **over)
            eng = model.engine
            eng.set_options(**(parse("preonly") if args.shared_ramp else s1), **extra)
            model.start()
            bench.spin_up(model, args.spinup_cap)
        if args.shared_ramp:
            eng.set_options(**s1)
        for _ in range(args.warmup):
            model.step()
        n0, l0, f0 = model.total_nits, model.total_lits, model.failed_solves
        applies = its = unconv = 0
        per_outer = 2 if (eng.opts["pc"] in ("cptr", "fieldsplit_cd") and not eng.opts.get("fs_additive")) else 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.step()
            if s1["s1_ksp"] != "preonly":
                a, i, u = eng.inner_stats()
                applies, its, unconv = applies + a, its + i, unconv + u
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        nits, lits = model.total_nits - n0, model.total_lits - l0
        print(json.dumps({"config": args.config, "preset": args.preset or "default", "setting": setting, **s1,
                          "steps": args.steps, "newton_its": nits, "outer_its": lits, "failed_solves": model.failed_solves - f0,
                          "outer_per_newton": lits/max(nits, 1),
                          "inner_per_outer": (per_outer*its/applies) if applies else (0.0 if s1["s1_ksp"] == "preonly" else None),
                          "inner_above_tolerance": unconv, "inner_solves_sampled": applies,
                          "ms_per_outer": 1e3*el/max(lits, 1), "newton_per_s": nits/el, "seconds": el,
                          "shared_ramp": bool(args.shared_ramp), "dt_days": [float(model.dt_vec[-args.steps])/86400.0, float(model.dt_vec[-1])/86400.0]}),
              flush=True)
        if not args.shared_ramp:
            eng.close()


if __name__ == "__main__":
    main()
