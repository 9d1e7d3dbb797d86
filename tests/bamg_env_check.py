"""Child process of tests/test_gpu_system_amg.py::test_global_memory_dense_inverse_child: the system AMG's dense inverse is
selected by TP_BAMG_DENSE_LDS, read once per process.  With the variable at 0 and nothing else set, the global-memory
Gauss-Jordan kernel inverts the coarsest 54-cell (108-unknown) system that the LDS kernel handles by default; the default
cycle and the V(3,3) cycle on 12 x 20 x 10 against the oracle."""
import os

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import cases
from oracle.engine import OracleEngine
from thermalporous_amd.engine import HipEngine


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def main():
    assert os.environ.get("TP_BAMG_DENSE_LDS") == "0"
    assert "TP_BAMG_TAIL_CELLS" not in os.environ and "TP_BAMG_FUSE_BELOW" not in os.environ
    spec, u0, *_ = cases.c4_spe10_3d(Nx=12, Ny=20, Nz=10, nphase=2)
    u = cases.perturbed_state(spec, seed=5, amp=0.3)
    x = np.random.default_rng(11).standard_normal(u.shape)
    for amg_opts in (dict(), dict(amg_nu=3)):
        opts = dict(pc="cptramg", decoup="QI", **amg_opts)
        o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
        for e in (o, h):
            e.set_old(u0)
            e.set_dt(8640.0)
            e.set_state(u)
        o.pc.setup(o.jacobian())
        h.jacobian()
        h.pc_setup()
        assert h.amg_info(2)[0] == len(o.pc.amg_pT.levels) == 7
        h.vec_set("x", x)
        h.amg_vcycle(2, "x", 0, "y", 0)
        dv = rel2(h.vec_get("y")[:2], o.pc.amg_pT.vcycle(x[:2]))
        h.stage1_apply("x", "y")
        ds = rel2(h.vec_get("y"), o.pc.stage1(x))
        h.pc_apply("x", "y")
        dp = rel2(h.vec_get("y"), o.pc.apply(x))
        print("global-memory dense inverse, %s: V-cycle %.3e, stage 1 %.3e, pc_apply %.3e" % (amg_opts, dv, ds, dp))
        assert dv < 1e-10, (amg_opts, dv)
        assert ds < 1e-9 and dp < 1e-9, (amg_opts, ds, dp)
        h.close()


if __name__ == "__main__":
    child_main(main)
