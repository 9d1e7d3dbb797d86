"""Child process of tests/test_gpu_ew.py::test_env_paths: the switches the Krylov loops read once per process (TP_PIN: the pinned
hand-over of the sums and latches, or a copy; TP_FGMRES_PIPE: the pipelined FGMRES loop with its speculative preconditioner
application, or a host wait per iteration) cannot be changed inside one process, so the parent starts this script once per
setting, each time as a fresh process.  It runs the ramp of tests/ew_ref.py under Eisenstat-Walker version 2 with FGMRES and with
BiCGStab and writes to the .npz path given as argv[1], per method: <ksp>.counts = per step (nits, lits, reason), <ksp>.rtol /
.fnorm / .lresid / .kits = the histories of all steps one after the other, and the final state <ksp>.x."""

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import ew_ref as R
from thermalporous_amd.engine import HipEngine


def main():
    out = {}
    spec, u0, *_ = R.ramp_case()
    for ksp in ("fgmres", "bcgs"):
        h = HipEngine(spec, dict(R.RAMP_OPTS, ksp=ksp, ksp_ew=2))
        hist = {k: [] for k in ("rtol", "fnorm", "lresid", "kits")}

        def solve(e):
            r = e.newton_solve()
            eh = e.ew_history()
            for k in hist:
                hist[k].extend(eh[k])
            return r
        steps = R.run_ramp(h, u0, R.RAMP_DT, solve)
        out[ksp + ".counts"] = np.array([(s["nits"], s["lits"], s["reason"]) for s in steps])
        for k in hist:
            out[ksp + "." + k] = np.array(hist[k])
        out[ksp + ".x"] = h.get_state()
        h.close()
    return out


if __name__ == "__main__":
    child_main(main)
