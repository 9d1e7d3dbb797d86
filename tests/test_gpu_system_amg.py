"""The system (2x2-block) AMG of pc_cptramg (csrc/tp_amg_block.hip) at the cycle shapes, level layouts and kernel variants that
the default-shape parity checks do not reach, against oracle/linalg.py:BlockSemiAMG (itself checked in
tests/test_oracle_block_amg.py).

Every case: two-phase, dt 8640, perturbed_state(seed=5, amp=0.3), x = default_rng(11); the system V-cycle alone
(tp_amg_vcycle(which=2)) rel 2-norm < 1e-10, stage 1 and the whole preconditioner < 1e-9 -- the bounds of test_gpu_parity.py and
ilu_env_check.py; a one-ulp perturbation of J and x moves the oracle itself by <= 2.9e-12 (V-cycle) and 1.1e-11 (stages) on
these cases (transfer_only_big_levels: 2.8e-12, 3.7e-13, 6.8e-14).  Each case also asserts, from the oracle's level shapes, that it
reaches the path it is named for.  Measured differences on an MI355X: <= 2.3e-12 (V-cycle), 4.6e-12 (stage 1), 4.3e-12
(pc_apply) over all cases; the per-level and unfused kernel variants equal the default kernels bit for bit."""
import threading

import numpy as np
import pytest

import cases
from switches import run_child, setup_env

pytestmark = pytest.mark.gpu

VTOL, STOL = 1e-10, 1e-9
DT, SEED, AMP = 8640.0, 5, 0.3


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def levels_of(amg):
    """(cells, coarsening axis, pre, post) of every level of the oracle's hierarchy (the rules of BlockSemiAMG.vcycle);
    the coarsest level is (cells, -1, 0, 0)."""
    out = []
    for l, A in enumerate(amg.levels):
        cells = int(np.prod(A.shape[3:]))
        if l == len(amg.levels) - 1:
            out.append((cells, -1, 0, 0))
            continue
        if l < amg.full_levels:
            pre, post = amg.nu, amg.nu
        else:
            pre, post = amg.coarse_pre, (amg.tail_post if cells <= 1024 else amg.coarse_post)
            if amg.mid_skip and cells > 1024 and (l - amg.full_levels) % 2 == 1:
                pre, post = 0, 0
        out.append((cells, amg.sched[l], pre, post))
    return out


def big(T):
    """The levels above the single-workgroup tail: more than 1024 cells."""
    return [lv for lv in T if lv[0] > 1024]


def shapes(T):
    """(pre, post) of every level but the coarsest."""
    return [lv[2:] for lv in T[:-1]]


def bshapes(T):
    return [lv[2:] for lv in big(T)]


BOX, LAYER = cases.c4_spe10_3d, cases.c3_spe10_2d
B12 = dict(Nx=12, Ny=20, Nz=10, nphase=2)         # 2400, 1200 | 600, 300, 150, 90, 54
B11 = dict(Nx=11, Ny=21, Nz=13, nphase=2)         # 3003, 1573 | 847, 462, 252, 144, 72, 36; internal extents 13 x 11 x 21
B16 = dict(Nx=16, Ny=18, Nz=16, nphase=2)         # 4608, 2304, 1152 | 640, ...
B15 = dict(Nx=15, Ny=25, Nz=21, nphase=2)         # 7875, 4095, 2205, 1155 | 616, ...
B9 = dict(Nx=9, Ny=14, Nz=8, nphase=2)            # 1008: the tail is level 0
L2D = dict(Nx=30, Ny=41, nphase=2)                # 1230 | 630, ...
TILE2D = (1 << 30, 64, 1)

# (id, builder, grid, decoupling, AMG options, path: level table -> bool)
CASES = [
    ("v11", BOX, B12, "QI", dict(amg_nu=1),
     # k_bamg_smooth<FIRST>, the fused correction writing the output directly (post == 1 on level 0), tail pre = 1
     lambda T: bshapes(T) == [(1, 1)]*2 and T[2][0] <= 1024 and T[2][2:] == (1, 1)),
    ("v33", BOX, B12, "QI", dict(amg_nu=3),
     # pre/post >= 3: the x/x2 ping-pong above the tail and inside it (one extra pre-sweep: odd)
     lambda T: bshapes(T) == [(3, 3)]*2 and T[2][0] <= 1024 and T[2][2:] == (3, 3) and T[3][2:] == (0, 2)),
    ("v44_odd_extents", BOX, B11, "QI", dict(amg_nu=4, amg_tail_post=3, amg_full_levels=99),
     # two extra pre-sweeps (even), a big level along axis 0, odd extents on level 0
     lambda T: [lv[1] for lv in big(T)] == [2, 0] and all(s == (4, 4) for s in shapes(T)) and len(T) == 8),
    ("v12_every_big_level", BOX, B12, "QI", dict(amg_full_levels=0, amg_coarse_pre=1, amg_coarse_post=2, amg_mid_skip=False),
     lambda T: bshapes(T) == [(1, 2)]*2 and T[2][2:] == (1, 2)),
    ("v31_beside_transfer_level", BOX, B16, "QI", dict(amg_full_levels=1, amg_coarse_pre=3, amg_coarse_post=1, amg_tail_post=1),
     lambda T: bshapes(T) == [(2, 2), (3, 1), (0, 0)] and T[3][0] <= 1024 and T[3][2:] == (3, 1)),
    ("pre0_on_level0", BOX, B16, "QI", dict(amg_full_levels=0, amg_coarse_pre=0, amg_coarse_post=2),
     # xs[0] null: residual = b, fused correction without x
     lambda T: bshapes(T) == [(0, 2), (0, 0), (0, 2)] and T[3][2:] == (0, 2)),
    ("four_big_levels_axis1", BOX, B15, "QI", dict(amg_full_levels=99),
     lambda T: [lv[1] for lv in big(T)] == [2, 2, 0, 1] and all(s == (2, 2) for s in shapes(T))),
    ("four_big_levels_axis1_v11", BOX, B15, "QI", dict(amg_full_levels=99, amg_nu=1),
     lambda T: [lv[1] for lv in big(T)] == [2, 2, 0, 1] and all(s == (1, 1) for s in shapes(T))),
    ("transfer_only_big_levels", BOX, B15, "QI", dict(amg_full_levels=0),
     # pure transfer levels above the tail, one along axis 1: k_bamg_prolong on its own, without the environment switch
     lambda T: [lv[1:] for lv in big(T)] == [(2, 0, 1), (2, 0, 0), (0, 0, 1), (1, 0, 0)] and T[4][2:] == (0, 2)),
    ("layer2d_big_level", LAYER, L2D, "QI", dict(ilu_tile=TILE2D),
     lambda T: [lv[:2] for lv in big(T)] == [(1230, 1)] and T[0][2:] == (2, 2)),
    ("layer2d_big_level_v33", LAYER, L2D, "QI", dict(amg_nu=3, ilu_tile=TILE2D),
     lambda T: [lv[:2] for lv in big(T)] == [(1230, 1)] and T[0][2:] == (3, 3) and T[1][2:] == (3, 3)),
    # 1008 cells: the tail kernel works on the caller's b and x at its first level
    ("tail_is_level0_v01", BOX, B9, "QI", dict(amg_full_levels=0, amg_coarse_pre=0, amg_tail_post=1),
     lambda T: not big(T) and T[0][0] == 1008 and all(s == (0, 1) for s in shapes(T))),
    ("tail_is_level0_v33", BOX, B9, "QI", dict(amg_nu=3, amg_tail_post=3),
     lambda T: not big(T) and shapes(T) == [(3, 3)]*3 + [(0, 3)]*2),
    ("tail_is_level0_v22_v21", BOX, B9, "QI", dict(amg_full_levels=1, amg_coarse_pre=2, amg_coarse_post=2, amg_tail_post=1),
     lambda T: not big(T) and shapes(T) == [(2, 2)] + [(2, 1)]*4),
    ("coarsest_180_unknowns", BOX, B12, "QI", dict(amg_min_cells=100),
     # above 128 unknowns: the global-memory dense inverse under the default environment
     lambda T: T[-1][0] == 90 and 2*T[-1][0] > 128),
    ("coarsest_one_cell", BOX, B11, "QI", dict(amg_min_cells=1),
     lambda T: len(T) == 14 and T[-1][0] == 1 and T[-2][0] == 2),
    ("default_shape_No", BOX, B12, "No", dict(),
     lambda T: shapes(T) == [(2, 2)]*3 + [(0, 2)]*3 and len(big(T)) == 2),
]
CASE = {c[0]: c for c in CASES}

_REF = {}


def reference(cid):
    """The oracle's side of a case, computed once: spec, states, x, level table, V-cycle / stage 1 / preconditioner of x."""
    if cid not in _REF:
        from oracle.engine import OracleEngine
        _, builder, kw, decoup, amg_opts, path = CASE[cid]
        spec, u0, *_ = builder(**kw)
        opts = dict(pc="cptramg", decoup=decoup, **amg_opts)
        o = OracleEngine(spec, opts)
        u = cases.perturbed_state(spec, seed=SEED, amp=AMP)
        o.set_old(u0)
        o.set_dt(DT)
        o.set_state(u)
        o.pc.setup(o.jacobian())
        x = np.random.default_rng(11).standard_normal(u.shape)
        amg = o.pc.amg_pT
        T = levels_of(amg)
        assert path(T), (cid, T)
        _REF[cid] = dict(spec=spec, u0=u0, u=u, x=x, opts=opts, T=T, sched=list(amg.sched), v=amg.vcycle(x[:2]), s1=o.pc.stage1(x),
                         pc=o.pc.apply(x))
    return _REF[cid]


def hip_engine(ref, env=None):
    """A fresh engine at the case's state with the Jacobian assembled and the preconditioner set up (under `env`)."""
    from thermalporous_amd.engine import HipEngine
    with setup_env(**(env or {})):
        h = HipEngine(ref["spec"], ref["opts"])
        h.set_old(ref["u0"])
        h.set_dt(DT)
        h.set_state(ref["u"])
        h.jacobian()
        h.pc_setup()
    return h


def run_three(h, x):
    """System V-cycle, stage 1 and whole preconditioner of x."""
    h.vec_set("x", x)
    h.amg_vcycle(2, "x", 0, "y", 0)
    v = h.vec_get("y")[:2].copy()
    h.stage1_apply("x", "y")
    s1 = h.vec_get("y").copy()
    h.pc_apply("x", "y")
    return v, s1, h.vec_get("y").copy()


def check_against_oracle(tag, ref, got):
    d = [rel2(got[0], ref["v"]), rel2(got[1], ref["s1"]), rel2(got[2], ref["pc"])]
    print("%s: GPU vs oracle: V-cycle %.3e, stage 1 %.3e, pc_apply %.3e" % (tag, d[0], d[1], d[2]))
    assert d[0] < VTOL, (tag, d)
    assert d[1] < STOL and d[2] < STOL, (tag, d)


def check_layout(h, ref):
    assert h.amg_info(2)[0] == len(ref["T"])
    assert h.amg_layout(2) == (0, ref["sched"])


_DEFAULT_VARIANT = {}


def default_variant(cid):
    """The three results of the default kernels on a case, computed once."""
    if cid not in _DEFAULT_VARIANT:
        ref = reference(cid)
        h = hip_engine(ref)
        check_layout(h, ref)
        _DEFAULT_VARIANT[cid] = run_three(h, ref["x"])
        h.close()
    return _DEFAULT_VARIANT[cid]


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_cycle_shapes_and_level_layouts(cid):
    check_against_oracle(cid, reference(cid), default_variant(cid))


@pytest.mark.parametrize("cid", ["v33", "pre0_on_level0"])
def test_vcycle_is_repeatable(cid):
    """The cycle keeps no state between applications: x, another vector, x again -- first and third bitwise equal."""
    ref = reference(cid)
    h = hip_engine(ref)
    h.vec_set("x", ref["x"])
    h.vec_set("z", np.random.default_rng(12).standard_normal(ref["x"].shape))
    out = []
    for src in ("x", "z", "x"):
        h.amg_vcycle(2, src, 0, "y", 0)
        out.append(h.vec_get("y")[:2].copy())
    h.close()
    assert np.array_equal(out[0], out[2])
    assert rel2(out[1], out[0]) > 1e-3
    assert rel2(out[0], ref["v"]) < VTOL


VARIANTS = [("per_level_tail", {"TP_BAMG_TAIL_CELLS": "0"}), ("unfused_correction", {"TP_BAMG_FUSE_BELOW": "0"}),
            ("per_level_unfused", {"TP_BAMG_TAIL_CELLS": "0", "TP_BAMG_FUSE_BELOW": "0"})]


@pytest.mark.parametrize("cid", ["v33", "pre0_on_level0", "v11", "four_big_levels_axis1"])
@pytest.mark.parametrize("vid,env", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_kernel_variants(vid, env, cid):
    """The per-level kernels in place of the single-workgroup tail, k_bamg_prolong + a plain sweep in place of the fused
    correction: the same cycle, against the oracle and against the default kernels."""
    ref = reference(cid)
    base = default_variant(cid)
    h = hip_engine(ref, env)
    check_layout(h, ref)
    got = run_three(h, ref["x"])
    h.close()
    check_against_oracle("%s/%s" % (cid, vid), ref, got)
    d = [rel2(a, b) for a, b in zip(got, base)]
    print("%s/%s: against the default kernels: V-cycle %.3e, stage 1 %.3e, pc_apply %.3e" % (cid, vid, d[0], d[1], d[2]))
    assert max(d) < 1e-10, (cid, vid, d)


def test_global_memory_dense_inverse_child():
    """TP_BAMG_DENSE_LDS is read once per process: tests/bamg_env_check.py runs the default and the V(3,3) case with only that
    variable set, in one child process."""
    run_child("bamg_env_check.py", {"TP_BAMG_DENSE_LDS": "0"}, timeout=300)


def test_live_option_changes_rebuild_the_hierarchy():
    """tp_set_options drops the hierarchy, the next set-up builds the new plan: each V-cycle is the oracle's with those options,
    and back at the defaults the first result returns bit for bit."""
    from oracle.engine import OracleEngine, DEFAULT_OPTS
    from thermalporous_amd.engine import HipEngine
    keys = ("amg_nu", "amg_full_levels", "amg_coarse_pre", "amg_coarse_post", "amg_min_cells")
    base = {k: DEFAULT_OPTS[k] for k in keys}
    steps = [dict(), dict(amg_nu=3), dict(amg_full_levels=0, amg_coarse_pre=0), dict(amg_min_cells=100), dict()]
    spec, u0, *_ = BOX(**B12)
    u = cases.perturbed_state(spec, seed=SEED, amp=AMP)
    x = np.random.default_rng(11).standard_normal(u.shape)
    h = HipEngine(spec, dict(pc="cptramg", decoup="QI"))
    h.set_old(u0)
    h.set_dt(DT)
    h.set_state(u)
    h.jacobian()
    h.vec_set("x", x)
    J, got, nlev = None, [], []
    for step in steps:
        opts = dict(base, **step)
        o = OracleEngine(spec, dict(pc="cptramg", decoup="QI", **opts))
        o.set_old(u0)
        o.set_dt(DT)
        o.set_state(u)
        J = o.jacobian() if J is None else J
        o.pc.setup(J)
        h.set_options(**opts)
        h.pc_setup()
        h.amg_vcycle(2, "x", 0, "y", 0)
        y = h.vec_get("y")[:2].copy()
        d = rel2(y, o.pc.amg_pT.vcycle(x[:2]))
        print("live options %s: V-cycle vs oracle %.3e" % (step, d))
        assert h.amg_info(2)[0] == len(o.pc.amg_pT.levels) and h.amg_layout(2)[1] == o.pc.amg_pT.sched
        assert d < VTOL, (step, d)
        got.append(y)
        nlev.append(h.amg_info(2)[0])
    h.close()
    assert nlev == [7, 7, 7, 6, 7]
    assert np.array_equal(got[0], got[-1])
    for k in (1, 2, 3):
        assert rel2(got[k], got[0]) > 1e-6, k


SLAB_SHAPES = [("v11", dict(amg_nu=1)), ("v33", dict(amg_nu=3)), ("v12_v10", dict(amg_full_levels=0, amg_coarse_pre=1))]


@pytest.mark.parametrize("sid,amg_opts", SLAB_SHAPES, ids=[s[0] for s in SLAB_SHAPES])
def test_cycle_shapes_on_slabs(sid, amg_opts):
    """The distributed hierarchy (as test_gpu_slabs.py::test_system_amg_on_slabs_equals_single_slab: 8 x 21 x 7, every level
    with two planes per slab kept on the slabs, 2 ranks as 2 host threads) at other cycle shapes: stage 1 equals the
    single-slab hierarchy to round-off, the whole preconditioner the 2-slab oracle's (ILU tiles restart per slab)."""
    import ctypes as C
    from oracle.engine import OracleEngine
    nranks = 2
    spec, u0, *_ = BOX(Nx=8, Ny=21, Nz=7, nphase=2)
    u = cases.perturbed_state(spec, seed=SEED, amp=AMP)
    xs = np.random.default_rng(11).standard_normal(u.shape)
    opts = dict(pc="cptramg", decoup="QI", amg_gather_cells=0, **amg_opts)

    def stage(n):
        from thermalporous_amd import engine as E
        lib = E.load_library()
        group = C.c_void_p()
        if n > 1:
            assert lib.tp_local_group_create(n, C.byref(group)) == 0
        out, err = [None]*n, []

        def worker(rank):
            try:
                h = E.HipEngine(spec, opts, rank=rank, nranks=n, local_group=group if n > 1 else None)
                h.set_old(u0)
                h.set_dt(DT)
                h.set_state(u)
                h.jacobian()
                h.pc_setup()
                h.vec_set("x", xs)
                h.stage1_apply("x", "s1")
                s1 = h.vec_get("s1")
                h.vec_set("x", xs)
                h.pc_apply("x", "pc")
                out[rank] = (s1, h.vec_get("pc"), h.amg_layout(2))
                h.close()
            except Exception as e:      # noqa: BLE001
                err.append((rank, repr(e)))
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in ts), "slab worker hung"
        if n > 1:
            lib.tp_local_group_destroy(group)
        assert not err, err
        return [np.concatenate([o[k] for o in out], axis=-3) for k in range(2)] + [out[0][2]]
    s1_one, _, lay1 = stage(1)
    s1_n, pc_n, layn = stage(nranks)
    assert lay1[0] == 0 and layn[0] >= 2 and 2 in layn[1][:layn[0]], (lay1, layn)     # distributed, incl. a slab-axis level
    o = OracleEngine(spec, dict(opts, nslabs=nranks))
    o.set_old(u0)
    o.set_dt(DT)
    o.set_state(u)
    o.pc.setup(o.jacobian())
    d1, d2, d3 = rel2(s1_n, s1_one), rel2(pc_n, o.pc.apply(xs)), rel2(s1_n, o.pc.stage1(xs))
    print("slabs %s: stage 1 on 2 slabs vs 1 slab %.3e, vs oracle %.3e; pc_apply vs 2-slab oracle %.3e" % (sid, d1, d3, d2))
    assert d1 < 1e-11, d1
    assert d2 < STOL, d2
