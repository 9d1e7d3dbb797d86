"""What a graded grid costs on one GPU, on config 4's size (60x220x85, two-phase, pc_cptr):

  assembly_ms   residual + Jacobian + S~ through tp_time_kernel 3 on a uniform context, on one given equal widths (the graded
                kernel on the uniform geometry) and on one whose z widths span a ratio of 8 (geometric, thin at top and base)
  newton        Krylov iterations per Newton step over --steps time steps of --dt seconds from the uniform initial state: the uniform
                box as a control, then the ratio-8 box with amg_line_levels off and on

    python scripts/graded_probe.py [--reps 200] [--steps 10] [--dt 86.4] [--line-levels 2] [--skip-newton] [--skip-assembly]

One JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                   # noqa: E402


def widths(spec, ratio):
    """Equal widths on every internal axis but the gravity axis (z), graded geometrically towards both ends at max/min = ratio."""
    from thermalporous_amd.spacing import geometric_widths
    hs = [np.full(int(spec["n"][a]), float(spec["h"][a])) for a in range(3)]
    if ratio > 1.0:
        a = int(spec["gaxis"])
        n = int(spec["n"][a])
        hs[a] = geometric_widths(n, n*float(spec["h"][a]), ratio**(1.0/((n - 1)//2)), refine="both")
    return tuple(hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--line-levels", type=int, default=2)
    ap.add_argument("--dt", type=float, default=86.4, help="time step of the Newton window in seconds, from the uniform initial state")
    ap.add_argument("--skip-newton", action="store_true")
    ap.add_argument("--skip-assembly", action="store_true")
    a = ap.parse_args()
    from bench import build_case
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.problem import build_spec
    params, geo, wells, _, _ = build_case("c4")
    spec = build_spec(geo, wells, params, 2)
    u0 = cases.uniform_state(spec, params.p_ref, params.T_prod, params.S_o)
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    settings = (("uniform", None), ("graded_equal", widths(spec, 1.0)), ("graded_z_ratio8", widths(spec, 8.0)))
    for rnd in range(0 if a.skip_assembly else 3):      # interleaved: every setting sees the same clocks
        for name, hs in settings:
            h = HipEngine(spec if hs is None else dict(spec, hs=hs), dict(pc="cptr"))
            h.set_old(u0)
            h.set_dt(8640.0)
            h.set_state(u)
            h.jacobian(want_schur=False)
            info = h.spacing_info()
            print(json.dumps(dict(what="assembly", setting=name, round=rnd, n=list(spec["n"]), assembly_ms=h.time_kernel(3, a.reps),
                                  hmin=info["hmin"], hmax=info["hmax"])), flush=True)
            h.close()
    if a.skip_newton:
        return
    g8 = dict(spec, hs=widths(spec, 8.0))
    for name, sp, L in (("uniform", spec, 0), ("graded_z_ratio8", g8, 0), ("graded_z_ratio8", g8, a.line_levels)):
        h = HipEngine(sp, dict(pc="cptr", amg_line_levels=L))
        h.set_state(u0)
        nits, lits = [], []
        for step in range(a.steps):
            h.set_old(None)
            h.set_dt(a.dt)
            r = h.newton_solve()
            nits.append(r["nits"])
            lits.append(r["lits"])
            if r["reason"] <= 0:
                break
        print(json.dumps(dict(what="newton", setting=name, amg_line_levels=L, dt=a.dt, steps=len(nits), nits=nits, lits=lits,
                              lits_per_nit=sum(lits)/max(sum(nits), 1), reason=r["reason"])), flush=True)
        h.close()


if __name__ == "__main__":
    main()
