"""Child process of tests/test_gpu_assembly_edges.py: the assembly kernel this process selects (TP_ASM_LDS, read once per
process: the LDS-tiled k_assemble_lds or the default k_assemble) at every (box, edge state) pair of edge_cases.edge_pairs()
on one slab, against the oracle; R, J and S~ of every pair are written to the .npz given as argument, so that the parent can
hold the two kernels to bitwise equality."""
import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import edge_cases as ec
from oracle.engine import OracleEngine
from thermalporous_amd.engine import HipEngine


def main():
    out = {}
    for pid, name, builder, kw, kind in ec.edge_pairs():
        spec, u = ec.edge_input(builder, kw, kind)
        opts = dict(pc="cptr" if kw["nphase"] == 2 else "fieldsplit_cd")
        o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
        for e in (o, h):
            e.set_old(u)
            e.set_dt(8640.0)
            e.set_state(u)
        Ro, (Jo, So) = o.residual(), o.jacobian(want_schur=True)
        Rh, (Jh, Sh) = h.residual(), h.jacobian(want_schur=True)
        assert np.isfinite(Ro).all() and np.isfinite(Jo).all() and np.isfinite(So).all(), pid
        for f in range(o.b):
            assert np.abs(Rh[f] - Ro[f]).max() < 1e-11*np.abs(Ro[f]).max(), (pid, "residual field", f)
            for c in range(o.b):
                sc = np.abs(Jo[:, f, c]).max()
                assert np.abs(Jh[:, f, c] - Jo[:, f, c]).max() < 1e-11*sc or (sc == 0.0 and np.abs(Jh[:, f, c]).max() == 0.0), (pid, f, c)
        assert np.abs(Sh - So).max() < 1e-11*np.abs(So).max(), (pid, "S~")
        out[pid + "/R"], out[pid + "/J"], out[pid + "/S"] = Rh, Jh, Sh
        h.close()
    return out


if __name__ == "__main__":
    child_main(main)
