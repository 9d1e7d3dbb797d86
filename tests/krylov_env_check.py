"""Child process of tests/test_gpu_krylov.py::test_env_switches_keep_krylov_results: the FGMRES / reduction fall-back
switches that the library reads once per process (TP_FGMRES_PIPE, TP_PIN, TP_GRAPH, TP_SPEC_MARGIN, TP_GS_REVERSE,
TP_MD_CHUNK, TP_HALO_OVERLAP) cannot be changed inside one process, so the parent runs this script once per setting.
It runs a fixed list of linear and Newton solves and writes what they returned to the .npz path given as argv[1]:
  linear solve <name>: <name>.its, .reason, .rnorm and <name>.x (the raw float64 entries of the owned cells)
  Newton run <name>:   <name>.nits, .lits, .reason, .vcycles (one entry per time step) and <name>.u (final state);
                       1, 2 and 3 slabs, and one single-slab run with ksp_restart 5."""
import ctypes as C
import threading

import numpy as np

from switches import child_main     # first: it puts the repository root on the path
import cases
from thermalporous_amd import engine as E

LINEAR = [
    ("cptr3d", cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", ksp_rtol=1e-10)),
    ("cpr2d", cases.c3_spe10_2d, dict(Nx=14, Ny=19, nphase=1), dict(pc="cpr", decoup="QI", ksp_rtol=1e-10,
                                                                     ilu_tile=(1 << 30, 64, 1))),
    ("restart5", cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", ksp_rtol=1e-10, ksp_restart=5)),
    ("maxit7", cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", ksp_rtol=1e-10, ksp_max_it=7)),
]
NEWTON_SPEC = (cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2))
NEWTON_OPTS = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
NEWTON_DTS = (86.4, 864.0)


def linear(out, name, builder, kw, opts):
    spec, u0, *_ = builder(**kw)
    h = E.HipEngine(spec, opts)
    h.set_old(u0)
    h.set_dt(8640.0)
    h.set_state(cases.perturbed_state(spec, seed=5, amp=0.3))
    h.jacobian()
    h.residual()
    h.copy_residual_to("b")
    its, reason, rn = h.fgmres("b", "x")
    out[name + ".its"], out[name + ".reason"], out[name + ".rnorm"] = its, reason, rn
    out[name + ".x"] = h.vec_get("x")
    h.close()


def newton(out, name, nranks, **extra):
    builder, kw = NEWTON_SPEC
    spec, u0, *_ = builder(**kw)
    opts = dict(NEWTON_OPTS, **extra)
    lib = E.load_library()
    group = C.c_void_p()
    if nranks > 1:
        assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    res = [None]*nranks
    err = []

    def worker(rank):
        try:
            h = E.HipEngine(spec, opts, rank=rank, nranks=nranks, local_group=group if nranks > 1 else None)
            h.set_state(u0)
            infos = []
            for dt in NEWTON_DTS:
                h.set_old(None)
                h.set_dt(dt)
                infos.append(dict(h.newton_solve()))
            res[rank] = (infos, h.get_state())
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    if nranks > 1:
        lib.tp_local_group_destroy(group)
    assert not err, err
    infos = res[0][0]
    for k in ("nits", "lits", "reason", "vcycles"):
        out[name + "." + k] = np.array([i[k] for i in infos])
    out[name + ".u"] = np.concatenate([r[1] for r in res], axis=1)


def main():
    out = {}
    for name, builder, kw, opts in LINEAR:
        linear(out, name, builder, kw, opts)
    for nranks in (1, 2, 3):
        newton(out, "newton%d" % nranks, nranks)
    newton(out, "newton_restart5", 1, ksp_restart=5)     # a speculation may not be issued on a cycle's last iteration
    return out


if __name__ == "__main__":
    child_main(main)
