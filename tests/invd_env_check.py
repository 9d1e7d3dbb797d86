"""Child process of tests/test_gpu_invd_registers.py: TP_AMG_INVD_LOAD is read once per process, so each setting runs this script
in a process of its own and the parent compares what the two processes wrote, bit for bit.

    python tests/invd_env_check.py OUT.npz

writes one array per case: a whole pc_apply, or the pressure and S~ V-cycles."""
import ctypes as C
import threading

import numpy as np

from switches import child_main, setup_env     # first: it puts the repository root on the path
import cases
from thermalporous_amd import engine as E

# (name, grid, options, environment of the hierarchy's build, what to run)
CASES = [
    # 132 000 cells: three V(2,2) levels, two pairs of a smoothed and a pure transfer level, the tail: k_amg_jacobi,
    # k_amg_prolong_jacobi and k_amg_prolong2_jacobi all run
    ("pc_apply_30x110x40", dict(Nx=30, Ny=110, Nz=40, nphase=2), dict(pc="cptr"), {}, "pc_apply"),
    # the top levels on the unfused path (k_amg_prolong_add + k_amg_jacobi), odd extents on every axis, deep hierarchy
    ("unfused_13x11x9", dict(Nx=13, Ny=11, Nz=9, nphase=2), dict(pc="cptr", amg_full_levels=2, amg_min_cells=4),
     {"TP_AMG_TAIL_CELLS": "8", "TP_AMG_FUSE_BELOW": "500"}, "vcycle"),
    # operators, weights and inverse diagonals stored in fp32: the quotient is rounded to float as the set-up rounds it
    ("fp32_operators", dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_single=True), {}, "vcycle"),
    # kernels that keep the stored plane next to the ones that do not: Gauss-Seidel levels, line levels, a truncated cycle
    ("gs_levels", dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_gs_levels=2), {}, "vcycle"),
    ("line_levels", dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_line_levels=2), {}, "vcycle"),
    ("truncated", dict(Nx=20, Ny=26, Nz=18, nphase=2), dict(pc="cptr", amg_dom_tau=1e6), {}, "vcycle"),
]
SLABS = ("slabs2_8x21x7", dict(Nx=8, Ny=21, Nz=7, nphase=2), dict(pc="cptr", amg_gather_cells=0), 3000.0)


def main():
    out = {}
    for name, kw, opts, env, what in CASES:
        spec, u0, *_ = cases.c4_spe10_3d(**kw)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        x = np.random.default_rng(11).standard_normal(u.shape)
        with setup_env(**env):
            h = E.HipEngine(spec, opts)
            h.set_old(u0)
            h.set_dt(8640.0)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
        h.vec_set("x", x)
        if what == "vcycle":
            for which in (0, 1):
                h.amg_vcycle(which, "x", which, "y", which)
                out["%s_v%d" % (name, which)] = h.vec_get("y")[which].copy()
            out[name + "_trunc"] = np.array([h.amg_trunc(0)[0], h.amg_trunc(1)[0]])
        else:
            h.pc_apply("x", "y")
            out[name] = h.vec_get("y").copy()
        h.close()
    # two slabs in one process: the sweeps of the distributed levels run on each slab's owned cells
    name, kw, opts, dt = SLABS
    spec, u0, *_ = cases.c4_spe10_3d(**kw)
    u = cases.perturbed_state(spec, seed=5, amp=0.2)
    xs = np.random.default_rng(11).standard_normal(u.shape)
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
            res[rank] = (h.vec_get("v0")[0].copy(), h.amg_layout(0)[0])
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    out[name + "_v0"] = np.concatenate([r[0] for r in res], axis=-3)
    out[name + "_dist"] = np.array([res[0][1]])
    return out


if __name__ == "__main__":
    child_main(main)
