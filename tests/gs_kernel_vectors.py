"""Inputs and GPU results of the Gram-Schmidt kernels (k_multi_dot, k_multi_axpy_norm, their predicated and fp32-basis
siblings) at nf = 2 and nf = 3 fields, for tests/test_gpu_gs_field_index.py.

compute() runs tp_vec_dot_batch, tp_vec_norm2, tp_vec_orth_step ("never": one pass, "always": the predicated second pass) and
tp_fvec_dot_batch on seeded vectors over a 7 x 13 x 9 box: 819 owned cells, so the 512-entry chunk of a wave straddles the
boundary between two fields (entries 819 and 1638) and the last chunk is partial.  Every kernel sums in a fixed order, so the
results are reproducible bit for bit.

    python tests/gs_kernel_vectors.py tests/golden/gs_kernel_vectors.npz

writes them as data; the committed file was written by the commit before the field index lost its 64-bit division."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GRID = dict(Nx=7, Ny=13, Nz=9)
K = 6                        # one batch of MD_U = 4 vectors and a remainder of two
CASES = [(2, dict(nphase=1), dict(pc="cpr", decoup="TI")), (3, dict(nphase=2), dict(pc="cptr"))]


def compute():
    import cases
    from thermalporous_amd.engine import HipEngine
    out = {}
    for nf, kw, opts in CASES:
        spec, u0, *_ = cases.c4_spe10_3d(**GRID, **kw)
        h = HipEngine(spec, opts)
        assert h.b == nf and np.shape(u0)[0] == nf and spec["phi"].size % 512 != 0
        rng = np.random.default_rng(100 + nf)
        V = rng.standard_normal((K,) + np.shape(u0))
        w = rng.standard_normal(np.shape(u0))
        h.vec_batch("v", K)
        for i in range(K):
            h.vec_set("v%d" % i, V[i])
        key = "nf%d_" % nf
        h.vec_set("w", w)
        out[key + "dot"] = h.dot_batch("v", K, "w")
        out[key + "norm"] = np.array([h.norm2("w")])
        for mode in ("never", "always"):
            h.vec_set("w", w)
            hc, n2, ran = h.orth_step("v", K, "w", mode)
            assert ran == (mode == "always")
            out[key + mode + "_h"] = hc
            out[key + mode + "_n2"] = np.array([n2])
            out[key + mode + "_w"] = h.vec_get("w")
        h.fvec_batch("f", K)
        for i in range(K):
            h.vec_set("t", V[i])
            h.fvec_store("f", i, "t")
        h.vec_set("w", w)
        out[key + "fdot"] = h.fdot_batch("f", K, "w")
        h.close()
    return out


if __name__ == "__main__":
    res = compute()
    np.savez(sys.argv[1], **res)
    print("wrote %s: %s" % (sys.argv[1], ", ".join(sorted(res))))
