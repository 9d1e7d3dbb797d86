"""The Gram-Schmidt kernels' field index from two comparisons instead of a 64-bit division (k_multi_dot, k_multi_axpy_norm, their
predicated and fp32-basis siblings): tp_vec_dot_batch, tp_vec_norm2, tp_vec_orth_step (one and two passes) and tp_fvec_dot_batch at
nf = 2 and nf = 3 on 819 owned cells -- no multiple of the 512-entry chunk, so chunks straddle the field boundaries -- bitwise
against tests/golden/gs_kernel_vectors.npz, which the commit before this change wrote on the GPU (tests/gs_kernel_vectors.py)."""
import os

import numpy as np
import pytest

import gs_kernel_vectors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_kernel_vectors.npz")


@pytest.fixture(scope="module")
def results():
    return gs_kernel_vectors.compute(), dict(np.load(GOLDEN))


@pytest.mark.parametrize("nf", [2, 3])
def test_gram_schmidt_kernels_bitwise(results, nf):
    got, want = results
    keys = sorted(k for k in want if k.startswith("nf%d_" % nf))
    assert len(keys) == 9 and set(keys) == {k for k in got if k.startswith("nf%d_" % nf)}
    for k in keys:
        a, b = np.asarray(got[k], dtype=np.float64), want[k]
        assert a.shape == b.shape and np.isfinite(b).all() and np.abs(b).max() > 0, k
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (k, float(np.abs(a - b).max()))
