"""Child process of tests/test_gpu_pj_fuse.py: TP_AMG_PJ_FUSE and TP_AMG_INVD_LOAD are read once per process, so each setting runs this script in a process of its own and the parent compares what the processes wrote, bit for bit, and holds
the default form against the numpy oracle.

    python tests/pj_fuse_env_check.py OUT.npz

writes per case the pressure and S~ V-cycles of a seeded random vector (and one whole pc_apply), the truncation levels and the
hierarchies' layouts (tp_amg_layout).  The cases, inputs and the two-slab run of rr_fuse_env_check as they are, and more."""

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import rr_fuse_env_check as K
from thermalporous_amd import engine as E

TOP = K.TOP         # every level above an 8-cell tail is a "big" level, every V(nu,nu) level takes the top levels' up-leg path
SMALL = dict(pc="cptr", amg_min_cells=4)

# name -> (grid, options, environment of the hierarchy's build, also one pc_apply)
CASES = dict(K.CASES)
CASES.update({
    # one sweep each way: the fused launch is the level's only post-sweep and writes its output (level 0: the cycle's result)
    "nu1": (dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_nu=1), TOP, True),
    # lines of 130 cells: the halo of a run (2 x 130 cells) is more than one slot per thread; then 65 cells: the most one slot holds
    "wide_130": (dict(Nx=5, Ny=6, Nz=130, nphase=2), SMALL, TOP, False),
    # lines of 128 cells: the halo fills its 256 slots exactly
    "wide_128": (dict(Nx=5, Ny=6, Nz=128, nphase=2), SMALL, TOP, False),
    # the thinnest levels: one or two cells along the axes that are not coarsened -- lines of one cell, planes of one line,
    # levels of one plane
    "thin_2x37x2": (dict(Nx=2, Ny=37, Nz=2, nphase=2), SMALL, TOP, False),
    "thin_2x2x37": (dict(Nx=2, Ny=2, Nz=37, nphase=2), SMALL, TOP, False),
    "thin_37x2x2": (dict(Nx=37, Ny=2, Nz=2, nphase=2), SMALL, TOP, False),
})
SLABS, DT, AMP, inputs = K.SLABS, K.DT, K.AMP, K.inputs


def main():
    out = {}
    for name, (kw, opts, env, whole) in CASES.items():
        spec, u0, u, x = K.inputs(kw)
        with K.setup_env(**env):
            h = E.HipEngine(spec, opts)
            h.set_old(u0)
            h.set_dt(K.DT)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
        h.vec_set("x", x)
        for which in (0, 1):
            h.amg_vcycle(which, "x", which, "y", which)
            out["%s_v%d" % (name, which)] = h.vec_get("y")[which].copy()
            out["%s_layout%d" % (name, which)] = K.layout_row(h, which)
        out[name + "_trunc"] = np.array([h.amg_trunc(0)[0], h.amg_trunc(1)[0]])
        if whole:
            h.pc_apply("x", "z")
            out[name + "_pc"] = h.vec_get("z").copy()
        h.close()
    out.update(slabs_run())
    return out


def slabs_run():
    """rr_fuse_env_check's two slabs in one process: the pressure V-cycle of both ranks, joined, and rank 0's layout."""
    import ctypes as C
    import threading
    name, kw, opts, env, dt, amp = SLABS
    spec, u0, u, xs = K.inputs(kw, amp)
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(2, C.byref(group)) == 0
    res, err = [None, None], []

    def worker(rank):
        try:
            h = E.HipEngine(spec, opts, rank=rank, nranks=2, local_group=group)
            h.set_old(u0)
            h.set_dt(dt)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
            h.vec_set("x", xs)
            h.amg_vcycle(0, "x", 0, "v0", 0)
            res[rank] = (h.vec_get("v0")[0].copy(), K.layout_row(h, 0))
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    with K.setup_env(**env):
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    return {name + "_v0": np.concatenate([r[0] for r in res], axis=-3), name + "_layout0": res[0][1]}


if __name__ == "__main__":
    child_main(main)
