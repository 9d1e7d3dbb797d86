"""Child process of tests/test_gpu_rr_fuse.py: TP_AMG_RR_FUSE and TP_AMG_INVD_LOAD are read once per process, so each setting runs
this script in a process of its own and the parent compares what the processes wrote, bit for bit, and holds the default form
against the numpy oracle.

    python tests/rr_fuse_env_check.py OUT.npz

writes per case the pressure and S~ V-cycles of a seeded random vector (and one whole pc_apply), the truncation levels and the
hierarchies' layouts (tp_amg_layout)."""
import ctypes as C
import threading

import numpy as np

from switches import child_main, setup_env     # first: it puts the repository root on the path
import cases
from thermalporous_amd import engine as E

# Every level above an 8-cell tail runs as a "big" level and every V(2,2) level takes the top levels' residual -> restriction path
TOP = {"TP_AMG_TAIL_CELLS": "8", "TP_AMG_FUSE_BELOW": "1"}
SEED_STATE, SEED_X, AMP, DT = 5, 11, 0.3, 8640.0

# name -> (grid, options, environment of the hierarchy's build, also one pc_apply)
CASES = {
    # pressure: axis 1 with 27 cells (odd; two tiles along the axis) and rows of 37 cells in two tiles of 19, then axis 0 with lines of
    # 37 cells (46 620 cells = 184 runs of 254), then axis 1 with 14 cells (even); S~: axis 0 with lines of 37, 19 and 10 cells
    "ax1_90x27x37": (dict(Nx=90, Ny=27, Nz=37, nphase=2), dict(pc="cptr", amg_min_cells=4), TOP, True),
    # pressure: axis 2 with 37 and 19 planes of 30 cells (three and two tiles along the axis), then axis 1 with 6 cells (even);
    # S~: axis 0 with lines of 5, 3 and 2 cells
    "ax2_6x37x5": (dict(Nx=6, Ny=37, Nz=5, nphase=2), dict(pc="cptr", amg_min_cells=4), TOP, False),
    # pressure: axis 2 with 6 and 3 planes, then axis 1 with 5 cells and rows of 37; S~: axis 0, lines of 37, 19, 10
    "ax2_5x6x37": (dict(Nx=5, Ny=6, Nz=37, nphase=2), dict(pc="cptr", amg_min_cells=4), TOP, False),
    # pressure: axis 1 with 6 cells (even), axis 0 with lines of 5, axis 1 with 3 cells
    "ax1_37x6x5": (dict(Nx=37, Ny=6, Nz=5, nphase=2), dict(pc="cptr", amg_min_cells=4), TOP, False),
    # odd extents on every axis: pressure axis 1 (11), axis 0 (9), axis 1 (6)
    "odd_13x11x9": (dict(Nx=13, Ny=11, Nz=9, nphase=2), dict(pc="cptr", amg_min_cells=4), TOP, False),
    # 18 x 20 x 26: pressure axis 2 with 26 and 13 planes of 360 cells (twelve row tiles, the last of 8; two tiles along the axis on
    # level 0), then axis 1 with 20 cells; S~: axis 0 with lines of 18, 9 and 5 cells
    "fp32_operators": (dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_single=True), TOP, False),
    "gs_levels": (dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_gs_levels=2), TOP, False),
    "line_levels": (dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_line_levels=2), TOP, False),
    # both cycles end at level 0 with relaxation only: no residual, no restriction
    "truncated": (dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_dom_tau=1e6), TOP, False),
}
# two slabs in one process, every level with two planes per slab distributed: level 0 coarsens the slab axis, level 1 axis 0
SLABS = ("slabs2_8x21x7", dict(Nx=8, Ny=21, Nz=7, nphase=2), dict(pc="cptr", amg_gather_cells=0), TOP, 3000.0, 0.2)


def inputs(kw, amp=AMP):
    spec, u0, *_ = cases.c4_spe10_3d(**kw)
    u = cases.perturbed_state(spec, seed=SEED_STATE, amp=amp)
    return spec, u0, u, np.random.default_rng(SEED_X).standard_normal(u.shape)


def layout_row(h, which):
    nd, axes = h.amg_layout(which)
    return np.array([nd] + list(axes))


def main():
    out = {}
    for name, (kw, opts, env, whole) in CASES.items():
        spec, u0, u, x = inputs(kw)
        with setup_env(**env):
            h = E.HipEngine(spec, opts)
            h.set_old(u0)
            h.set_dt(DT)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
        h.vec_set("x", x)
        for which in (0, 1):
            h.amg_vcycle(which, "x", which, "y", which)
            out["%s_v%d" % (name, which)] = h.vec_get("y")[which].copy()
            out["%s_layout%d" % (name, which)] = layout_row(h, which)
        out[name + "_trunc"] = np.array([h.amg_trunc(0)[0], h.amg_trunc(1)[0]])
        if whole:
            h.pc_apply("x", "z")
            out[name + "_pc"] = h.vec_get("z").copy()
        h.close()
    name, kw, opts, env, dt, amp = SLABS
    spec, u0, u, xs = inputs(kw, amp)
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
            res[rank] = (h.vec_get("v0")[0].copy(), layout_row(h, 0))
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    with setup_env(**env):
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    out[name + "_v0"] = np.concatenate([r[0] for r in res], axis=-3)
    out[name + "_layout0"] = res[0][1]
    return out


if __name__ == "__main__":
    child_main(main)
