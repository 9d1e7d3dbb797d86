"""What the saturation functions cost on one GPU, on config 4's box (60x220x85, two-phase, pc_cptr):

  assembly   residual + Jacobian + S~ through tp_time_kernel 3 under the linear curves and under the models M1 (Corey, n 2 and 3),
             M2 (Brooks-Corey kr with exponent 4, linear p_c) and M3 (M1 with the Brooks-Corey p_c): ms_avg and the algorithmic
             bytes per ms from the 616 B per cell of csrc/tp_assembly.hip's header; three interleaved rounds, so that every
             setting sees the same clocks and the spread between rounds is on the page
  newton     --steps time steps of the time loop from the end of bench.py's dt ramp, under the linear curves and under M1: Newton
             iterations per step, Krylov iterations per Newton step, failed solves

    python scripts/satfn_probe.py [--reps 200] [--steps 20] [--skip-newton] [--skip-assembly] > profiles/satfn_probe_c4.txt

One JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases                                   # noqa: E402

M1 = dict(relperm="corey", Sr_o=0.2, Sr_w=0.15, n_o=2.0, n_w=3.0, kro_max=0.9, krw_max=0.4)
M2 = dict(relperm="brooks_corey", lmbda=2.0, Sr_o=0.2, Sr_w=0.15, capillary="linear", p_ct=0.05)
M3 = dict(M1, capillary="brooks_corey", p_ct=0.01, lmbda=2.0, pc_se_min=0.05)
BYTES_PER_CELL = 616.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-newton", action="store_true")
    ap.add_argument("--skip-assembly", action="store_true")
    a = ap.parse_args()
    from bench import build_case, spin_up
    from thermalporous_amd.engine import HipEngine
    from thermalporous_amd.problem import build_spec
    params, geo, wells, _, _ = build_case("c4")
    spec = build_spec(geo, wells, params, 2)
    ncell = int(spec["n"][0])*int(spec["n"][1])*int(spec["n"][2])
    u0 = cases.uniform_state(spec, params.p_ref, params.T_prod, params.S_o)
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    settings = (("linear", None), ("M1", M1), ("M2", M2), ("M3", M3))
    for rnd in range(0 if a.skip_assembly else 3):
        for name, sat in settings:
            h = HipEngine(spec if sat is None else dict(spec, satfn=sat), dict(pc="cptr"))
            h.set_old(u0)
            h.set_dt(8640.0)
            h.set_state(u)
            h.jacobian(want_schur=False)
            ms = h.time_kernel(3, a.reps)
            print(json.dumps(dict(what="assembly", setting=name, round=rnd, n=list(spec["n"]), ms_avg=ms,
                                  algorithmic_GB_per_s=BYTES_PER_CELL*ncell/ms*1e-6, active=h.saturation_info()["active"])), flush=True)
            h.close()
    if a.skip_newton:
        return
    for name, sat in (("linear", None), ("M1", M1)):
        params, geo, case, cls, kw = build_case("c4")
        for k, v in (sat or {}).items():
            setattr(params, k, v)
        model = cls(geo, case, params, end=1e9, filename=None, verbosity=False, **kw)
        model.start()
        n_spin, _ = spin_up(model, 80)
        ramp = dict(steps=n_spin, newton_its=model.total_nits, fgmres_its=model.total_lits, failed_solves=model.failed_solves)
        failed0 = model.failed_solves
        nits, lits = [], []
        for _ in range(a.steps):
            n, l = model.step()
            nits.append(n)
            lits.append(l)
        S = model.u._read()[2]
        print(json.dumps(dict(what="newton", setting=name, steps=len(nits), nits=nits, lits=lits, nits_per_step=sum(nits)/len(nits),
                              lits_per_nit=sum(lits)/max(sum(nits), 1), failed_solves=model.failed_solves - failed0, ramp=ramp,
                              dt_days=float(model.dt)/86400.0, S_o_min=float(S.min()), S_o_max=float(S.max()))), flush=True)
        model.finish()
        model.engine.close()


if __name__ == "__main__":
    main()
