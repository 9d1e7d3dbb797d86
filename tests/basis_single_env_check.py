"""Child process of tests/test_gpu_basis_single.py::test_env_switches: the switches the fp32-basis FGMRES reads once per process
(TP_FGMRES_PIPE: the pipelined or the plain loop; TP_PIN: the pinned hand-over of the Gram-Schmidt sums, without which the loop
cannot pipeline either; TP_GRAPH: recorded or eager pc_apply; TP_MD_CHUNK: 8 or 4 entries per lane in the Gram-Schmidt kernels)
cannot be changed inside one process, so the parent runs this script once per setting.  It runs tp_fgmres with ksp_basis_single
on two inputs of basis_single_ref.PARITY -- c3_cptr and c4_cptr -- with the right-hand side the GPU assembles, and writes to
the .npz path given as argv[1], per input <name>: <name>.its, .reason, .rnorm, .cycles, .programs and <name>.x."""

from switches import child_main     # first: it puts the repository root on the path
import basis_single_ref as R
import cases
from thermalporous_amd.engine import HipEngine

NAMES = ("c3_cptr", "c4_cptr")


def main():
    out = {}
    for name, shape, opts, dt, seed, kw in R.PARITY:
        if name not in NAMES:
            continue
        builder, bkw = R._shapes()[shape]
        spec, u0, *_ = builder(**bkw)
        h = HipEngine(spec, dict(opts, ksp_basis_single=True, **R.solver_kw(kw)[1]))
        h.set_old(u0)
        h.set_dt(dt)
        h.set_state(cases.perturbed_state(spec, seed=seed, amp=0.3))
        h.jacobian()
        h.residual()
        h.pc_setup()
        h.copy_residual_to("b")
        its, reason, rn = h.fgmres("b", "x")
        out[name + ".its"], out[name + ".reason"], out[name + ".rnorm"] = its, reason, rn
        out[name + ".cycles"] = h.ksp_basis_info()["cycles"]
        out[name + ".programs"] = h.ksp_info()["pc_programs"]
        out[name + ".x"] = h.vec_get("x")
        h.close()
    return out


if __name__ == "__main__":
    child_main(main)
