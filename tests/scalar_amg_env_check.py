"""Child process of tests/test_gpu_scalar_amg.py::test_pair_switch_child: the pairing of a smoothed V(0,post) level with the
pure-transfer level below it (k_amg_restrict2 / k_amg_prolong2_jacobi) is selected by TP_AMG_PAIR, read once per process.  With
the variable at 0 and nothing else set, every level runs its own transfer kernels: the paired case and the default shape against
the oracle, the vectors written to the .npz named on the command line for the parent's comparison with the paired kernels."""
import os

from switches import child_main     # first: it puts the repository root on the path
import test_gpu_scalar_amg as G


def main():
    assert os.environ.get("TP_AMG_PAIR") == "0"
    for k in ("TP_AMG_TAIL_CELLS", "TP_AMG_FUSE_BELOW", "TP_AMG_TAIL_LDS", "TP_AMG_TAIL_DENSE"):
        assert k not in os.environ, k
    out = {}
    for cid in G.PAIR_CHILD_CASES:
        ref = G.reference(cid)
        got = G.run_variant(cid, "default", {})
        G.check_against_oracle("TP_AMG_PAIR=0, %s" % cid, ref, got)
        for k in G.KEYS:
            out["%s/%s" % (cid, k)] = got[k]
    return out


if __name__ == "__main__":
    child_main(main)
