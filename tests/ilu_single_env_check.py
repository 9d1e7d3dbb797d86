"""Child process of tests/test_gpu_ilu_single.py::test_one_wave_kernel: the fp32 factor stream (ilu_single) through the sweep
kernel the environment selects (TP_ILU_MW is read once per process; TP_ILU_MW=0 is the one-wave kernel k_ilu_solve) against
ilu_single_ref.SingleILU0 -- compact rows (9x14x8, both block sizes) and 64-lane rows (a tile of 8 x 8 columns)."""
import os

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import cases
from ilu_single_ref import swap_into
from oracle.engine import OracleEngine
from thermalporous_amd.engine import HipEngine


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


CASES = [(dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr")),
         (dict(Nx=9, Ny=14, Nz=8, nphase=1), dict(pc="cpr")),
         (dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr", ilu_tile=(1 << 30, 8, 8)))]


def main():
    for kw, opts in CASES:
        spec, u0, *_ = cases.c4_spe10_3d(**kw)
        o, h = OracleEngine(spec, opts), HipEngine(spec, dict(opts, ilu_single=True))
        swap_into(o)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        for e in (o, h):
            e.set_old(u0)
            e.set_dt(8640.0)
            e.set_state(u)
        schur = opts["pc"] == "cptr"
        out = o.jacobian(want_schur=schur)
        J, Sm = out if schur else (out, None)
        h.jacobian()
        o.pc.setup(J, Sm)
        h.pc_setup()
        x = np.random.default_rng(11).standard_normal(u.shape)
        h.vec_set("x", x)
        h.ilu_solve("x", "y")
        y32 = h.vec_get("y").copy()
        d = rel2(y32, o.pc.ilu.solve(x))
        print("TP_ILU_MW=%s %r %r: sweep vs SingleILU0 %.3e" % (os.environ.get("TP_ILU_MW"), kw, opts, d), flush=True)
        assert d <= 1e-6, (kw, opts, d)
        h.pc_apply("x", "y")
        d = rel2(h.vec_get("y"), o.pc.apply(x))
        print("    pc_apply %.3e" % d, flush=True)
        assert d <= 1e-6, (kw, opts, d)
        h.set_options(ilu_single=False)
        h.pc_setup()
        h.ilu_solve("x", "y")
        assert not np.array_equal(h.vec_get("y"), y32), (kw, opts)
        h.close()


if __name__ == "__main__":
    child_main(main)
