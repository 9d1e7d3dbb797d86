"""Child process of tests/test_gpu_bcgs.py::test_env_switches: the switches tp_bcgs reads once per process (TP_PIN: the pinned
hand-over of ||r||^2 and the latches, or a copy of the state block; TP_BCGS_WIDE: 16-byte or 8-byte items; TP_GRAPH: recorded or
eager pc_apply) cannot be changed inside one process, so the parent runs this script once per setting.  It runs tp_bcgs on two
inputs of bcgs_ref.PARITY -- c3_cptr (even plane size: 16-byte items by default) and c4_cptr (7 x 13 planes: 8-byte items
always) -- with the right-hand side the GPU assembles, and writes to the .npz path given as argv[1], per input <name>:
<name>.its, .reason, .rnorm, .programs (tp_ksp_info's pc_apply programs) and <name>.x."""

from switches import child_main     # first: it puts the repository root on the path
import bcgs_ref as R
import cases
from thermalporous_amd.engine import HipEngine

NAMES = ("c3_cptr", "c4_cptr")


def main():
    out = {}
    for name, shape, opts, dt, seed in R.PARITY:
        if name not in NAMES:
            continue
        builder, kw = R._shapes()[shape]
        spec, u0, *_ = builder(**kw)
        h = HipEngine(spec, opts)
        h.set_old(u0)
        h.set_dt(dt)
        h.set_state(cases.perturbed_state(spec, seed=seed, amp=0.3))
        h.jacobian()
        h.residual()
        h.pc_setup()
        h.copy_residual_to("b")
        its, reason, rn = h.bcgs("b", "x")
        out[name + ".its"], out[name + ".reason"], out[name + ".rnorm"] = its, reason, rn
        out[name + ".programs"] = h.ksp_info()["pc_programs"]
        out[name + ".x"] = h.vec_get("x")
        h.close()
    return out


if __name__ == "__main__":
    child_main(main)
