"""Child process of tests/test_gpu_reorth.py::test_env_switches: the switches the orthogonalisation reads once per process
(TP_PIN: the pinned hand-over of the sums, or a copy; TP_FGMRES_PIPE: the pipelined loop, or a host wait per iteration;
TP_REORTH_DOT_REVERSE: the direction of the second dot pass) cannot be changed inside one process, so the parent runs this
script once per setting.  It runs a Newton solve of the 7 x 13 x 9 two-phase case with ksp_reorth "always" and "ifneeded" and
writes to the .npz path given as argv[1], per mode: <mode>.counts = (nits, lits, reason, second passes executed), <mode>.fnorm and
the final state <mode>.x."""

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import bcgs_ref as R
from thermalporous_amd.engine import HipEngine


def main():
    out = {}
    builder, kw = R._shapes()["c4"]
    spec, u0, *_ = builder(**kw)
    for mode in ("always", "ifneeded"):
        h = HipEngine(spec, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, ksp_reorth=mode))
        h.set_state(u0)
        h.set_old(u0)
        h.set_dt(86.4)
        r = h.newton_solve()
        out[mode + ".counts"] = np.array([r["nits"], r["lits"], r["reason"], h.ksp_reorth_info()["refined"]])
        out[mode + ".fnorm"] = r["fnorm"]
        out[mode + ".x"] = h.get_state()
        h.close()
    return out


if __name__ == "__main__":
    child_main(main)
