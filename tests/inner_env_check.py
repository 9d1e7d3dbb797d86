"""Child process of tests/test_gpu_inner.py::test_graph_and_eager_agree: TP_GRAPH (captured hipGraph or eager launches of
pc_apply) is read once per process.  Prints a digest of the pc_apply outputs with the inner solve named on the command line;
the parent compares the digests of the two modes bit for bit."""
import hashlib
import sys

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import cases
from thermalporous_amd.engine import HipEngine


def main():
    s1 = dict(s1_ksp="fgmres", s1_max_it=6, s1_rtol=1e-3) if sys.argv[1] == "fgmres" else dict(s1_ksp="richardson", s1_max_it=3)
    for opts in (dict(pc="cpr", decoup="QI"), dict(pc="cptr"), dict(pc="cptramg", decoup="QI")):
        spec, u0, *_ = cases.c4_spe10_3d(Nx=7, Ny=13, Nz=9, nphase=2)
        h = HipEngine(spec, dict(opts, **s1))
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        h.set_old(u0)
        h.set_dt(8640.0)
        h.set_state(u)
        h.jacobian()
        h.pc_setup()
        for seed in (11, 12):
            h.vec_set("x", np.random.default_rng(seed).standard_normal(u.shape))
            for rep in range(2):                            # second call: the replay of the captured graph
                h.pc_apply("x", "y")
                y = h.vec_get("y")
                assert np.isfinite(y).all() and y.any()
                print("digest", opts["pc"], seed, rep, hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest())
        print("stats", h.inner_stats())
        h.close()


if __name__ == "__main__":
    child_main(main)
