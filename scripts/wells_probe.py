"""What the completed wells cost on one GPU, on config 4's box (60x220x85, two-phase, pc_cptr), with wells that
are open over all 85 layers beside the configuration's own single-cell wells and heaters:

  kernels    average device time of k_well_apply (tp_time_kernel 14) and k_wells (15) beside k_spmv_block (0), k_sources (16) and
             the whole assembly (3), with 2 wells and with 42 wells of 85 perforations, all in rate mode; three rounds each
  newton     --steps time steps of the time loop from the end of bench.py's dt ramp with one producer and one injector in rate
             mode, then the same steps from the same start with the same wells forced into BHP mode at the bottom-hole pressures
             the rate run ended with (there the rank-1 term is zero and the preconditioner sees the whole operator): Newton
             iterations per step and Krylov iterations per Newton step.  The difference is the price of keeping c b^T out of
             the preconditioner.

    python scripts/wells_probe.py [--reps 200] [--steps 10] [--skip-newton] [--skip-kernels] > profiles/wells_probe_c4.txt

One JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                   # noqa: E402


def add_wells(case, geo, params, nwells, rate, far=True, limits=None):
    """nwells wells over the whole thickness on a lattice of columns, producers and injectors alternating."""
    nx = max(1, int(round((nwells*geo.Length/geo.Length_y)**0.5)))
    ny = -(-nwells//nx)
    k = 0
    for j in range(ny):
        for i in range(nx):
            if k == nwells:
                return
            xy = ((i + 0.5)*geo.Length/nx, (j + 0.5)*geo.Length_y/ny)
            prod = k % 2 == 0
            name = ("P%d" if prod else "I%d") % (k//2)
            lim = limits[name] if limits else ((1.0 if prod else 200.0) if far else (params.p_prod if prod else params.p_inj))
            (case.add_producer if prod else case.add_injector)(name, xy=xy, z=(0.0, geo.Length_z), rate=rate, bhp=lim)
            k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-newton", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    from bench import build_case, spin_up
    from thermalporous_amd.completedwells import CompletedWellCase
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.problem import build_spec
    for nwells in (() if a.skip_kernels else (2, 42)):
        params, geo, base, _, _ = build_case("c4")
        case = CompletedWellCase(params, geo, base=base)
        add_wells(case, geo, params, nwells, params.rate)
        spec = build_spec(geo, case, params, 2)
        u0 = cases.uniform_state(spec, params.p_ref, params.T_prod, params.S_o)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        h = HipEngine(spec, dict(pc="cptr"))
        h.set_old(u0)
        h.set_dt(8640.0)
        h.set_state(u)
        h.jacobian(want_schur=False)
        info = h.well_info()
        for rnd in range(3):
            ms = {name: h.time_kernel(which, a.reps) for name, which in (("k_spmv_block", 0), ("k_well_apply", 14), ("k_wells", 15),
                                                                         ("k_sources", 16), ("assembly", 3))}
            h.jacobian(want_schur=False)            # (15 added to R, J: a fresh assembly for the next round)
            print(json.dumps(dict(what="kernels", wells=nwells, perforations=sum(w["cells"].size for w in h.wells), round=rnd,
                                  n=list(spec["n"]), ms_avg=ms, modes=sorted({i["mode"] for i in info}),
                                  rounds_max=max(i["rounds"] for i in info), open_min=min(i["nopen"] for i in info))), flush=True)
        h.close()
    if a.skip_newton:
        return
    limits = None
    for setting in ("rate", "bhp"):
        params, geo, base, cls, kw = build_case("c4")
        case = CompletedWellCase(params, geo, base=base)
        if limits is None:
            add_wells(case, geo, params, 2, params.rate)
        else:                                       # the same wells at the limits the rate run ended with, and a rate they cannot reach
            add_wells(case, geo, params, 2, 1e3*params.rate, limits=limits)
        model = cls(geo, case, params, end=1e9, filename=None, verbosity=False, **kw)
        model.start()
        n_spin, _ = spin_up(model, 80)
        ramp = dict(steps=n_spin, newton_its=model.total_nits, fgmres_its=model.total_lits, failed_solves=model.failed_solves)
        failed0 = model.failed_solves
        nits, lits, modes = [], [], []
        for _ in range(a.steps):
            n, l = model.step()
            nits.append(n)
            lits.append(l)
            modes.append([w["mode"] for w in model.engine.well_info()])
        info = model.engine.well_info()
        print(json.dumps(dict(what="newton", setting=setting, steps=len(nits), nits=nits, lits=lits, nits_per_step=sum(nits)/len(nits),
                              lits_per_nit=sum(lits)/max(sum(nits), 1), failed_solves=model.failed_solves - failed0, ramp=ramp,
                              dt_days=float(model.dt)/86400.0, modes=modes[-1], modes_all_same=all(m == modes[0] for m in modes),
                              wells=[dict(name=w["name"], bhp=w["bhp"], rate=w["rate"], nopen=w["nopen"]) for w in info])), flush=True)
        if limits is None:
            limits = {w["name"]: w["bhp"] for w in info}
        model.finish()
        model.engine.close()


if __name__ == "__main__":
    main()
