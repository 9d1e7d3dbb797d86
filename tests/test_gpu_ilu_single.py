"""ilu_single: the block-ILU(0) factor stream stored in fp32 (tp_options.ilu_single), everything else fp64.

Reference: ilu_single_ref.SingleILU0 -- the oracle's factorisation, the solve in the device's form on the three stored arrays
rounded to float32.  Both sides round fp64 products to fp32, and a product that differs in its last bit between the device
and numpy may round to the neighbouring float: the bound is the one the project uses wherever both sides round stored
operators to fp32, rel <= 1e-6 in the 2-norm (2e-6 on slabs), not the 1e-10 of the fp64 sweeps."""
import ctypes as C
import threading

import numpy as np
import pytest

import cases
from ilu_single_ref import swap_into
from switches import run_child

pytestmark = pytest.mark.gpu

TOL = 1e-6


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def engines(builder, kw, opts, hip_opts=None, dt=8640.0, seed=5, amp=0.3):
    """Oracle with SingleILU0 in place of its stage 2 (built WITHOUT the new key) and the GPU engine with ilu_single, both at
    the seeded perturbed state; Jacobian assembled on the GPU, assembled and set up in the oracle."""
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = builder(**kw)
    o = OracleEngine(spec, opts)
    swap_into(o)
    h = HipEngine(spec, {**opts, "ilu_single": True, **(hip_opts or {})})
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    for e in (o, h):
        e.set_old(u0)
        e.set_dt(dt)
        e.set_state(u)
    schur = opts["pc"] == "cptr"
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    h.jacobian()
    o.pc.setup(J, Sm)
    return spec, u0, o, h


SWEEPS = [
    # default tile (whole line x t1 x t2): ragged tiles along both tile axes, compact rows, 3x3 blocks
    ("box_2ph", cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr")),
    ("box_1ph", cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=1), dict(pc="cpr")),                 # 2x2 blocks
    ("layer2d", cases.c3_spe10_2d, dict(Nx=20, Ny=30, nphase=2), dict(pc="cptr")),                      # one plane, rows narrower than a wave
    # axis-0 extent 3: fewer steps (5 and 13) than either ring depth; planes of 6 and of 18 cells (the second is wide enough
    # for the sweeps' block transfers of the vectors: a plane must hold one block of the deepest ring)
    ("line3_tiny", cases.c4_spe10_3d, dict(Nx=2, Ny=2, Nz=3, nphase=2), dict(pc="cptr")),
    ("line3", cases.c4_spe10_3d, dict(Nx=6, Ny=6, Nz=3, nphase=2), dict(pc="cptr")),
    # axis-0 extent 1: planes of 9 cells (single transfers) and of 16 (block transfers)
    ("line1", cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=1, nphase=2), dict(pc="cptr")),
    ("line1_wide", cases.c4_spe10_3d, dict(Nx=16, Ny=20, Nz=1, nphase=2), dict(pc="cptr")),
    ("tile64", cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr", ilu_tile=(1 << 30, 8, 8))),   # t1*t2 = 64: wave-wide rows
]


@pytest.mark.parametrize("name,builder,kw,opts", SWEEPS, ids=[c[0] for c in SWEEPS])
def test_sweep_parity(name, builder, kw, opts):
    spec, u0, o, h = engines(builder, kw, opts)
    x = np.random.default_rng(11).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    h.ilu_factor()
    h.ilu_solve("x", "y")
    y32 = h.vec_get("y").copy()
    b32 = h.ilu_factor_bytes()
    d = rel2(y32, o.pc.ilu.solve(x))
    # the fp64 factor of the same context
    h.set_options(ilu_single=False)
    h.ilu_factor()
    h.ilu_solve("x", "y")
    y64 = h.vec_get("y").copy()
    b64 = h.ilu_factor_bytes()
    print("%s: tile %r, fp32 sweep vs SingleILU0 %.3e; fp32 vs fp64 sweep %.3e; factor bytes %d / %d = %.4f"
          % (name, h.ilu_layout()["block"], d, rel2(y32, y64), b32, b64, b32/b64))
    assert d <= TOL, (name, d)
    assert not np.array_equal(y32, y64), name
    assert b32 <= 0.55*b64, (name, b32, b64)
    h.close()


def test_one_wave_kernel():
    """TP_ILU_MW=0 (read once per process): k_ilu_solve's fp32 instantiation in ONE fresh child process."""
    run_child("ilu_single_env_check.py", {"TP_ILU_MW": "0"}, timeout=300)


PCS = [("cpr", dict(pc="cpr")), ("cptr", dict(pc="cptr")), ("cptr_amg_single", dict(pc="cptr", amg_single=True))]


@pytest.mark.parametrize("name,opts", PCS, ids=[c[0] for c in PCS])
def test_whole_preconditioner(name, opts):
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2), opts)
    h.pc_setup()
    x = np.random.default_rng(12).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    h.pc_apply("x", "y")
    d = rel2(h.vec_get("y"), o.pc.apply(x))
    print("%s: pc_apply with the fp32 factor vs TwoStagePC with SingleILU0 %.3e" % (name, d))
    assert d <= TOL, (name, d)
    h.close()


def test_two_slabs():
    """Two slab contexts in two threads (in-process slab group): each slab factors its own rows, the reference restarts its
    tiles at the slab boundary (SingleILU0 with the same slabs).  Bound: the slab tests' fp32 tolerance."""
    from oracle.engine import OracleEngine
    from thermalporous_amd import engine as E
    nranks = 2
    spec, u0, *_ = cases.c4_spe10_3d(Nx=8, Ny=21, Nz=7, nphase=2)
    opts = dict(pc="cptr")
    u = cases.perturbed_state(spec, seed=5, amp=0.2)
    xs = np.random.default_rng(11).standard_normal(u.shape)
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    out, err = [None]*nranks, []

    def worker(rank):
        try:
            h = E.HipEngine(spec, dict(opts, ilu_single=True), rank=rank, nranks=nranks, local_group=group)
            h.set_old(u0)
            h.set_dt(3000.0)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
            h.vec_set("x", xs)
            h.pc_apply("x", "pc")
            out[rank] = h.vec_get("pc")
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    o = OracleEngine(spec, dict(opts, nslabs=nranks))
    swap_into(o)
    assert o.pc.ilu.shape == o.prob.shape and len(o.pc.slabs) == nranks
    o.set_old(u0)
    o.set_dt(3000.0)
    o.set_state(u)
    J, Sm = o.jacobian(want_schur=True)
    o.pc.setup(J, Sm)
    d = rel2(np.concatenate(out, axis=-3), o.pc.apply(xs))
    print("two slabs: pc_apply with the fp32 factor vs the 2-slab oracle with SingleILU0 %.3e" % d)
    assert d <= 2e-6, d


def test_one_newton_solve():
    """tp_newton_solve with the fp32 factor against the oracle's Newton solve with SingleILU0: equal Newton counts, Krylov
    counts within +-1 per linear solve (both report the sum over the solves: |difference| <= number of solves), states
    rel <= 1e-8.  The fp64 factor's counts on the same case are printed beside them."""
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = cases.c4_spe10_3d(Nx=12, Ny=22, Nz=10, nphase=2)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25)
    o = OracleEngine(spec, opts)
    swap_into(o)
    h = HipEngine(spec, dict(opts, ilu_single=True))
    h64 = HipEngine(spec, opts)
    for e in (o, h, h64):
        e.set_state(u0)
        e.set_old(u0)
        e.set_dt(86.4)
    ro, rh, r64 = o.newton_solve(), h.newton_solve(), h64.newton_solve()
    uo, uh = o.get_state(), h.get_state()
    errs = [rel2(uh[f], uo[f]) for f in range(3)]
    print("Newton its: oracle+SingleILU0 %d, GPU fp32 factor %d, GPU fp64 factor %d; FGMRES its %d, %d, %d; state errors %r"
          % (ro["nits"], rh["nits"], r64["nits"], ro["lits"], rh["lits"], r64["lits"], errs))
    assert ro["reason"] > 0 and rh["reason"] == ro["reason"], (ro, rh)
    assert rh["nits"] == ro["nits"], (ro, rh)
    assert abs(rh["lits"] - ro["lits"]) <= ro["nits"], (ro, rh)
    assert max(errs) <= 1e-8, errs
    h.close()
    h64.close()


def test_live_toggle():
    """off -> on -> off on one context, a tp_pc_setup after each: the stage-2 data are re-allocated and re-factored."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr"), hip_opts=dict(ilu_single=False))
    x = np.random.default_rng(13).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    ys, nbytes = [], []
    for single in (False, True, False):
        h.set_options(ilu_single=single)
        h.pc_setup()
        h.pc_apply("x", "y")
        ys.append(h.vec_get("y").copy())
        nbytes.append(h.ilu_factor_bytes())
    fresh = HipEngine(spec, dict(pc="cptr", ilu_single=True))
    fresh.set_old(u0)
    fresh.set_dt(8640.0)
    fresh.set_state(cases.perturbed_state(spec, seed=5, amp=0.3))
    fresh.jacobian()
    fresh.pc_setup()
    fresh.vec_set("x", x)
    fresh.pc_apply("x", "y")
    assert np.array_equal(ys[0], ys[2])
    assert not np.array_equal(ys[0], ys[1])
    assert np.array_equal(ys[1], fresh.vec_get("y"))
    assert nbytes[0] == nbytes[2] and nbytes[1] == fresh.ilu_factor_bytes() and nbytes[1] <= 0.55*nbytes[0], nbytes
    assert rel2(ys[1], o.pc.apply(x)) <= TOL
    fresh.close()
    h.close()


def test_device_side_rejections():
    """The C ABI refuses ilu_single with ilu_whole, ilu_levels 1 (tp_set_options) and a multi-tile ilu_block (tp_pc_setup),
    naming both options; the context goes on working with the option off."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, o, h = engines(cases.c4_spe10_3d, dict(Nx=9, Ny=14, Nz=8, nphase=2), dict(pc="cptr"), hip_opts=dict(ilu_single=False))
    x = np.random.default_rng(14).standard_normal(np.shape(u0))
    h.vec_set("x", x)
    h.pc_setup()
    h.pc_apply("x", "y")
    y0 = h.vec_get("y").copy()

    def refused(other, **kw):
        """(return code of tp_set_options, of tp_pc_setup, last error) with the host-side checks bypassed"""
        opt = HipEngine._make_options(dict(h.opts, ilu_single=True, **kw))
        rc = h.lib.tp_set_options(h.ctx, C.byref(opt))
        rc2 = h.lib.tp_pc_setup(h.ctx) if rc == 0 else None
        msg = h.lib.tp_last_error().decode()
        assert (rc != 0 or rc2 != 0) and "ilu_single" in msg and other in msg, (other, rc, rc2, msg)
        h.set_options(ilu_single=False)          # h.opts never saw the refused combination
        h.pc_setup()
        h.pc_apply("x", "y")
        assert np.array_equal(h.vec_get("y"), y0), other

    refused("ilu_whole", ilu_whole=True)
    refused("ilu_levels", ilu_levels=1)
    refused("ilu_block", ilu_block=(1 << 30, 9, 7), ilu_tile=(4, 3, 7))
    h.set_options(ilu_single=True)
    h.pc_setup()
    h.pc_apply("x", "y")
    assert rel2(h.vec_get("y"), o.pc.apply(x)) <= TOL
    h.close()
