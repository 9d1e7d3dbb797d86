"""The scalar semicoarsening AMG of pc_cptr (csrc/tp_amg.hip: the pressure hierarchy, which=0, and the S~ hierarchy, which=1) at
the cycle shapes, coarse-solve sizes and truncation depths that the default-shape parity checks do not reach, against
oracle/linalg.py:SemiAMG (itself checked in tests/test_oracle_scalar_amg.py, which also re-asserts on the CPU every path
predicate, truncation margin, sensitivity and coarsest size of the table below).

Every case: two-phase pc="cptr", perturbed_state(seed=5, amp), x = default_rng(11); both V-cycles, stage 1 and the whole
preconditioner rel 2-norm < 1e-10 against the oracle (the bound of test_gpu_parity.py::test_linear_stages_parity; 1e-6 with
amg_single, as there); the truncation level, the level count and the tail facts (first tail level, dense operator or multilevel
kernel, applications issued) equal what the oracle's level table implies.  A one-ulp perturbation of J, S~ and x moves the oracle
itself by <= 6.2e-14 (V-cycles), 1.7e-12 (stage 1) and 1.9e-13 (apply) on these cases (asserted <= 1e-11 on the CPU; the
12 x 20 x 10 box, at 1.5e-10 in stage 1, serves only the amg_single case with its 1e-6 bound).

Measured on an MI355X over all cases and build-switch variants: V-cycles <= 7.7e-14, stage 1 <= 5.7e-13, pc_apply <= 1.6e-13
(amg_single: 6.7e-15).  Bitwise equal, and asserted so: TP_AMG_PAIR=0 (every level its own transfer kernels) to the paired kernels,
TP_AMG_TAIL_LDS=0 (the tail's vectors in global memory) to the LDS tail under the dense operator and under the multilevel kernel;
also TP_AMG_TAIL_CELLS=8 on the truncated 2-D layer.  Round-off only: the multilevel tail against the dense operator <= 2.5e-16
(V-cycles), 2.4e-14 (stage 1), the unfused kernels (TP_AMG_FUSE_BELOW=1, TP_AMG_TAIL_CELLS=8) against the fused ones <= 1.1e-16
(V-cycles), 5.7e-14 (stage 1), 2.2e-13 (pc_apply)."""
import collections

import numpy as np
import pytest

import cases
from switches import run_child, setup_env

pytestmark = pytest.mark.gpu

TOL, TOL_SINGLE = 1e-10, 1e-6
SEED = 5
KEYS = ("vp", "vS", "s1", "pc")


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def levels_of(amg):
    """(cells, coarsening axis, pre, post) of every level of the oracle's hierarchy (the rules of SemiAMG.vcycle); the coarsest
    level is (cells, -1, 0, 0).  The truncation level is not marked: it replaces the level's shape whatever that is."""
    out = []
    for l, A in enumerate(amg.levels):
        cells = int(np.prod(A.shape[1:]))
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


def layout(T):
    """(cells, axis) per level."""
    return [lv[:2] for lv in T]


def tail_facts(T, opts, env, trunc):
    """What tp_amg_tail_info must report for a hierarchy with level table T right after one V-cycle on a fresh engine:
    (tail_level, dense, dense_applies, tail_launches).  The rules of amg_plan / setup_impl / vcycle_impl: the tail starts at the
    first level of at most TP_AMG_TAIL_CELLS (1024) cells, else it is the coarsest level alone; it is applied as one dense operator
    when it spans at least two levels, none of them among the levels that truncation is decided on (tail_level >= nratio), unless
    TP_AMG_TAIL_DENSE=0; a cycle truncated above the tail applies neither form."""
    from oracle.engine import DEFAULT_OPTS
    o = dict(DEFAULT_OPTS, **opts)
    tail_cells = int(env.get("TP_AMG_TAIL_CELLS", 1024))
    lt = next((l for l, lv in enumerate(T) if lv[0] <= tail_cells), len(T) - 1)
    nratio = min(o["amg_full_levels"], len(T) - 1, 8) if o["amg_dom_tau"] > 0.0 else 0
    dense = env.get("TP_AMG_TAIL_DENSE", "1") != "0" and len(T) - lt >= 2 and T[lt][0] <= 1024 and lt >= nratio
    reached = trunc < 0 or trunc >= lt
    return lt, dense, int(reached and dense), int(reached and not dense)


BOX, LAYER = cases.c4_spe10_3d, cases.c3_spe10_2d
TILE2D = (1 << 30, 64, 1)
# grids, and their (cells, axis) per level of the pressure and the S~ hierarchy at dt = 8640, amp = 0.3, amg_min_cells = 64
# (B11: amg_min_cells = 1); tests/test_oracle_scalar_amg.py::test_level_tables_of_the_boxes re-asserts them
B12 = dict(Nx=12, Ny=20, Nz=10, nphase=2)
B11 = dict(Nx=11, Ny=21, Nz=13, nphase=2)
B16 = dict(Nx=16, Ny=18, Nz=16, nphase=2)
B15 = dict(Nx=15, Ny=25, Nz=21, nphase=2)
B9 = dict(Nx=9, Ny=14, Nz=8, nphase=2)
B20 = dict(Nx=20, Ny=26, Nz=18, nphase=2)
B7 = dict(Nx=7, Ny=13, Nz=9, nphase=2)
L2D = dict(Nx=30, Ny=41, nphase=2)
TABLES = {
    "B12": (BOX, B12, dict(),
            [(2400, 2), (1200, 2), (600, 0), (300, 1), (150, 2), (90, 0), (54, -1)],
            [(2400, 0), (1200, 0), (720, 0), (480, 2), (240, 0), (120, 1), (60, -1)]),
    "B11": (BOX, B11, dict(amg_min_cells=1),
            [(3003, 2), (1573, 0), (847, 2), (462, 1), (252, 0), (144, 2), (72, 1), (36, 0), (18, 2), (12, 1), (8, 0), (4, 2), (2, 1),
             (1, -1)],
            [(3003, 0), (1617, 0), (924, 0), (462, 2), (242, 0), (121, 2), (66, 1), (36, 2), (18, 1), (9, 2), (6, 1), (4, 2), (2, 1),
             (1, -1)]),
    "B16": (BOX, B16, dict(),
            [(4608, 2), (2304, 0), (1152, 2), (640, 1), (320, 0), (160, 2), (96, 1), (48, -1)],
            [(4608, 0), (2304, 0), (1152, 0), (576, 2), (288, 0), (144, 1), (72, 2), (40, -1)]),
    "B15": (BOX, B15, dict(),
            [(7875, 2), (4095, 2), (2205, 0), (1155, 1), (616, 2), (352, 0), (192, 1), (96, 2), (48, -1)],
            [(7875, 0), (4125, 0), (2250, 0), (1125, 2), (585, 0), (390, 1), (208, 2), (112, 0), (56, -1)]),
    "B9": (BOX, B9, dict(),
           [(1008, 2), (504, 2), (288, 0), (144, 1), (80, 2), (40, -1)],
           [(1008, 0), (504, 0), (252, 0), (126, 2), (63, -1)]),
    "L2D": (LAYER, L2D, dict(ilu_tile=TILE2D),
            [(1230, 1), (630, 1), (330, 0), (165, 1), (90, 0), (48, -1)],
            [(1230, 1), (630, 0), (315, 1), (165, 0), (88, 1), (48, -1)]),
}

DT, AMP = 8640.0, 0.3            # the state of the cycle-shape and coarse-solve cases
DT_DOM, AMP_DOM = 86.4, 0.05     # the truncation cases: S~ strongly diagonally dominant, the pressure operator (ratio 1) never

# id; builder, grid; dt, amp; AMG options (amg_dom_tau = 0 unless given); path(P, S): the level tables of the pressure and the S~
# hierarchy -> bool; the level at which each hierarchy is truncated (-1: not); the build-switch variants run besides the default
Case = collections.namedtuple("Case", "id builder kw dt amp opts path trunc variants")
DENSE_OFF = {"TP_AMG_TAIL_DENSE": "0"}
UNFUSED = {"TP_AMG_FUSE_BELOW": "1", "TP_AMG_TAIL_CELLS": "8"}
TAIL_VARIANTS = (("dense_off", DENSE_OFF), ("lds_off", {"TP_AMG_TAIL_LDS": "0"}),
                 ("lds_off_dense_off", {"TP_AMG_TAIL_LDS": "0", "TP_AMG_TAIL_DENSE": "0"}))
# variants measured bitwise equal to another run of their case on an MI355X: the tail's vectors in global memory instead of LDS
# (TP_AMG_TAIL_LDS=0), under the dense operator and under the multilevel kernel; the other variants differ from the default
# kernels by round-off (another evaluation order: T b, or x += P e and a sweep in place of the fused correction)
BITWISE = {"lds_off": "default", "lds_off_dense_off": "dense_off"}


def case(cid, builder, kw, opts, path, dt=DT, amp=AMP, trunc=(-1, -1), variants=()):
    return Case(cid, builder, kw, dt, amp, dict(dict(amg_dom_tau=0.0), **opts), path, trunc, tuple(variants))


def both(f):
    return lambda P, S: f(P) and f(S)


CASES = [
    # ---- cycle shapes above the tail and inside it
    case("default_shape", BOX, B16, dict(),
         # three V(2,2) levels above a tail of five; nothing to pair (the control of the TP_AMG_PAIR child)
         both(lambda T: bshapes(T) == [(2, 2)]*3 and len(T) == 8 and shapes(T)[3:] == [(0, 2)]*4)),
    case("v11", BOX, B11, dict(amg_nu=1),
         # k_amg_pre with two = 0, one post-sweep writing the output directly
         both(lambda T: bshapes(T) == [(1, 1)]*2 and T[2][0] <= 1024 and T[2][2:] == (1, 1)), variants=[("unfused", UNFUSED)]),
    case("v33", BOX, B11, dict(amg_nu=3),
         # one extra sweep of the x/x2 ping-pong (odd) above the tail and inside it
         # unfused: every level on its own, x += P e (k_amg_prolong_add) and three plain sweeps in place of the fused correction
         both(lambda T: bshapes(T) == [(3, 3)]*2 and T[2][0] <= 1024 and T[2][2:] == (3, 3) and T[3][2:] == (0, 2)),
         variants=[("unfused", UNFUSED)]),
    case("v44_odd_extents_to_one_cell", BOX, B11, dict(amg_nu=4, amg_full_levels=99, amg_tail_post=3, amg_min_cells=1),
         # two extra sweeps (even), odd extents, 14 levels, a coarsest grid of 2 cells and then 1; pressure: a big level along axis 0
         lambda P, S: all(len(T) == 14 and all(s == (4, 4) for s in shapes(T)) and [lv[0] for lv in T[-2:]] == [2, 1]
                          for T in (P, S)) and [lv[1] for lv in big(P)] == [2, 0] and len(big(S)) == 2),
    case("v12_every_big_level", BOX, B11, dict(amg_full_levels=0, amg_coarse_pre=1, amg_coarse_post=2, amg_mid_skip=False),
         both(lambda T: bshapes(T) == [(1, 2)]*2 and T[2][2:] == (1, 2))),
    case("v31_beside_transfer_level", BOX, B16, dict(amg_full_levels=1, amg_coarse_pre=3, amg_coarse_post=1, amg_tail_post=1),
         # a smoothed level WITH pre-sweeps next to a pure-transfer level: paired() must return false
         both(lambda T: bshapes(T) == [(2, 2), (3, 1), (0, 0)] and T[3][0] <= 1024 and T[3][2:] == (3, 1)),
         variants=[("unfused", UNFUSED)]),
    case("pre0_post2_paired", BOX, B15, dict(amg_full_levels=0, amg_coarse_pre=0, amg_coarse_post=2),
         # V(0,2) levels paired with transfer levels: k_amg_restrict2 / k_amg_prolong2_jacobi, then a second sweep;
         # unfused: the same shapes level by level, src == nullptr with post = 2
         both(lambda T: bshapes(T) == [(0, 2), (0, 0)]*2 and T[4][0] <= 1024 and T[4][2:] == (0, 2)),
         variants=[("unfused", UNFUSED)]),
    case("four_big_levels", BOX, B15, dict(amg_full_levels=99),
         lambda P, S: [lv[1] for lv in big(P)] == [2, 2, 0, 1] and [lv[1] for lv in big(S)] == [0, 0, 0, 2]
         and all(s == (2, 2) for s in shapes(P) + shapes(S))),
    case("four_big_levels_v11", BOX, B15, dict(amg_full_levels=99, amg_nu=1),
         lambda P, S: len(big(P)) == len(big(S)) == 4 and all(s == (1, 1) for s in shapes(P) + shapes(S))),
    case("layer2d_v33", LAYER, L2D, dict(amg_nu=3, ilu_tile=TILE2D),
         both(lambda T: [lv[:2] for lv in big(T)] == [(1230, 1)] and shapes(T)[:3] == [(3, 3)]*3 and shapes(T)[3:] == [(0, 2)]*2)),
    # 1008 cells: the tail kernel works on the caller's b and x at its first level
    case("tail_is_level0_v01", BOX, B9, dict(amg_full_levels=0, amg_coarse_pre=0, amg_tail_post=1),
         both(lambda T: not big(T) and T[0][0] == 1008 and all(s == (0, 1) for s in shapes(T))), variants=TAIL_VARIANTS),
    case("tail_is_level0_v33", BOX, B9, dict(amg_nu=3, amg_tail_post=3),
         lambda P, S: not big(P) and not big(S) and shapes(P) == [(3, 3)]*3 + [(0, 3)]*2 and shapes(S) == [(3, 3)]*3 + [(0, 3)],
         variants=TAIL_VARIANTS),
    case("tail_is_level0_v22_v21", BOX, B9, dict(amg_full_levels=1, amg_coarse_pre=2, amg_coarse_post=2, amg_tail_post=1),
         lambda P, S: not big(P) and not big(S) and shapes(P) == [(2, 2)] + [(2, 1)]*4 and shapes(S) == [(2, 2)] + [(2, 1)]*3,
         variants=TAIL_VARIANTS),
    case("v33_fp32_operators", BOX, B12, dict(amg_nu=3, amg_single=True),
         both(lambda T: bshapes(T) == [(3, 3)]*2 and T[2][2:] == (3, 3))),
    # ---- coarse solve
    case("coarsest_160_cells", BOX, B16, dict(amg_min_cells=200),
         # more than 64 cells: k_amg_dense_inverse (global memory), and a coarse mat-vec with n > 64 in the tail
         lambda P, S: P[-1][0] == 160 and S[-1][0] == 144 and len(P) == len(S) == 6, variants=[("dense_off", DENSE_OFF)]),
    case("coarsest_65_cells", BOX, B11, dict(amg_min_cells=72),
         # the first sizes past the LDS inverse kernels (n <= 64): pressure 72 cells, S~ 66
         lambda P, S: P[-1][0] == 72 and S[-1][0] == 66 and 64 < S[-1][0] < P[-1][0] <= 72, variants=[("dense_off", DENSE_OFF)]),
    # ---- truncation depth (S~ only; its dominance ratios per level in the comments)
    case("trunc2_big_level", BOX, B16, dict(amg_dom_tau=0.07),
         # 0.0873, 0.0870, 0.0508: level 2 (1152 cells) lies above the tail, whose dense operator is never applied
         lambda P, S: S[2][0] == 1152 and S[3][0] <= 1024 and bshapes(S)[:2] == [(2, 2)]*2,
         dt=DT_DOM, amp=AMP_DOM, trunc=(-1, 2)),
    case("trunc3_first_tail_level", BOX, B16, dict(amg_dom_tau=0.045, amg_full_levels=4),
         # ..., 0.0508, 0.0381: level 3 (576 cells) is the tail's first level, so the multilevel kernel ends where it starts;
         # tail_level 3 < nratio 4 switches the dense tail off in both hierarchies
         lambda P, S: S[3][0] == 576 and S[2][0] > 1024 and P[3][0] == 640 and P[2][0] > 1024,
         dt=DT_DOM, amp=AMP_DOM, trunc=(-1, 3)),
    case("trunc3_big_level", BOX, B20, dict(amg_dom_tau=0.12, amg_full_levels=4),
         # 0.166, 0.1564, 0.1564, 0.0873: three smoothed levels above a relaxation-only one of 1560 cells
         lambda P, S: S[3][0] == 1560 and bshapes(S)[:3] == [(2, 2)]*3,
         dt=DT_DOM, amp=AMP_DOM, trunc=(-1, 3)),
    case("trunc1_layer2d", LAYER, L2D, dict(amg_dom_tau=0.03, ilu_tile=TILE2D),
         # 0.087, 0.0119: level 1 (630 cells) is the tail's first level; TP_AMG_TAIL_CELLS=8: a relaxation-only level above the tail
         lambda P, S: S[0][0] == 1230 and S[1][0] == 630 and S[0][2:] == (2, 2),
         dt=DT_DOM, amp=AMP_DOM, trunc=(-1, 1), variants=[("tail_cells_8", {"TP_AMG_TAIL_CELLS": "8"})]),
    case("trunc4_inside_tail", BOX, B7, dict(amg_dom_tau=0.02, amg_full_levels=5),
         # 0.0462, 0.0461, 0.0461, 0.0461, 0.0081: the tail starts at level 0 and ends at level 4 of 6 (k_amg_tail with trunc > lt)
         lambda P, S: S[0][0] == 819 and len(S) == 6 and S[4][0] == 98 and shapes(S)[:4] == [(2, 2)]*4,
         dt=DT_DOM, amp=AMP_DOM, trunc=(-1, 4)),
]
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES)

# tail facts pinned by hand where the issue names them: (case, variant, hierarchy) -> (tail_level, dense)
PINNED = {
    ("default_shape", "default", 0): (3, True),
    ("pre0_post2_paired", "default", 0): (4, True), ("pre0_post2_paired", "unfused", 0): (8, False),
    ("tail_is_level0_v33", "default", 1): (0, True), ("tail_is_level0_v33", "dense_off", 1): (0, False),
    ("tail_is_level0_v33", "lds_off", 0): (0, True), ("tail_is_level0_v33", "lds_off_dense_off", 0): (0, False),
    ("coarsest_160_cells", "default", 0): (3, True), ("coarsest_160_cells", "dense_off", 0): (3, False),
    ("coarsest_160_cells", "default", 1): (3, True),
    ("trunc2_big_level", "default", 1): (3, True), ("trunc2_big_level", "default", 0): (3, True),
    ("trunc3_first_tail_level", "default", 1): (3, False), ("trunc3_first_tail_level", "default", 0): (3, False),
    ("trunc3_big_level", "default", 1): (4, True),
    ("trunc1_layer2d", "default", 1): (1, False), ("trunc1_layer2d", "tail_cells_8", 1): (5, False),
    ("trunc4_inside_tail", "default", 1): (0, False), ("trunc4_inside_tail", "default", 0): (0, False),
}


def variants_of(c):
    return (("default", {}),) + c.variants


def oracle_engine(c, opts=None, dt=None, amp=None):
    """The oracle at the case's state, set up -> (engine, spec, u0, u, J, Sm)."""
    from oracle.engine import OracleEngine
    spec, u0, *_ = c.builder(**c.kw)
    o = OracleEngine(spec, dict(pc="cptr", **(c.opts if opts is None else opts)))
    u = cases.perturbed_state(spec, seed=SEED, amp=c.amp if amp is None else amp)
    o.set_old(u0)
    o.set_dt(c.dt if dt is None else dt)
    o.set_state(u)
    J, Sm = o.jacobian(want_schur=True)
    o.pc.setup(J, Sm)
    return o, spec, u0, u, J, Sm


def oracle_four(o, x):
    return dict(vp=o.pc.amg_p.vcycle(x[0]), vS=o.pc.amg_T.vcycle(x[1]), s1=o.pc.stage1(x), pc=o.pc.apply(x))


def trunc_of(amg):
    return -1 if amg.trunc is None else amg.trunc


_REF = {}


def reference(cid):
    """The oracle's side of a case, computed once: spec, states, x, level tables, truncation levels, the four results."""
    if cid not in _REF:
        c = CASE[cid]
        o, spec, u0, u, _, _ = oracle_engine(c)
        x = np.random.default_rng(11).standard_normal(u.shape)
        P, S = levels_of(o.pc.amg_p), levels_of(o.pc.amg_T)
        assert c.path(P, S), (cid, P, S)
        _REF[cid] = dict(spec=spec, u0=u0, u=u, x=x, opts=dict(pc="cptr", **c.opts), T=(P, S),
                         trunc=(trunc_of(o.pc.amg_p), trunc_of(o.pc.amg_T)), tol=TOL_SINGLE if c.opts.get("amg_single") else TOL,
                         **oracle_four(o, x))
        assert _REF[cid]["trunc"] == c.trunc, (cid, _REF[cid]["trunc"])
    return _REF[cid]


def hip_engine(c, ref, env=None):
    """A fresh engine at the case's state with the Jacobian assembled and the preconditioner set up (under `env`)."""
    from thermalporous_amd.engine import HipEngine
    with setup_env(**(env or {})):
        h = HipEngine(ref["spec"], ref["opts"])
        h.set_old(ref["u0"])
        h.set_dt(c.dt)
        h.set_state(ref["u"])
        h.jacobian()
        h.pc_setup()
    return h


def run_four(h, x, facts=None):
    """Both V-cycles (then `facts`: the tail counters of the two hierarchies so far), stage 1 and the whole preconditioner of x."""
    h.vec_set("x", x)
    h.amg_vcycle(0, "x", 0, "y", 0)
    vp = h.vec_get("y")[0].copy()
    h.amg_vcycle(1, "x", 1, "y", 1)
    vS = h.vec_get("y")[1].copy()
    if facts is not None:
        facts.extend(h.amg_tail_info(w) for w in (0, 1))
    h.stage1_apply("x", "y")
    s1 = h.vec_get("y").copy()
    h.pc_apply("x", "y")
    return dict(vp=vp, vS=vS, s1=s1, pc=h.vec_get("y").copy())


def check_against_oracle(tag, ref, got):
    d = [rel2(got[k], ref[k]) for k in KEYS]
    print("%s: GPU vs oracle: V-cycle p %.3e, V-cycle S~ %.3e, stage 1 %.3e, pc_apply %.3e" % ((tag,) + tuple(d)))
    assert max(d) < ref["tol"], (tag, d)


def run_variant(cid, vid, env):
    """One fresh engine under `env`: the layout, truncation and tail facts asserted, the four results returned."""
    c, ref = CASE[cid], reference(cid)
    h = hip_engine(c, ref, env)
    facts = []
    got = run_four(h, ref["x"], facts)
    after = [h.amg_tail_info(w) for w in (0, 1)]
    for w in (0, 1):
        T = ref["T"][w]
        assert h.amg_info(w)[0] == len(T), (cid, vid, w)
        assert h.amg_layout(w) == (0, [lv[1] for lv in T[:-1]]), (cid, vid, w)
        assert h.amg_trunc(w)[0] == ref["trunc"][w], (cid, vid, w, h.amg_trunc(w))
        lt, dense, napply, nlaunch = tail_facts(T, c.opts, env, ref["trunc"][w])
        if (cid, vid, w) in PINNED:
            assert (lt, dense) == PINNED[(cid, vid, w)]
        f = facts[w]
        assert (f["tail_level"], f["dense"], f["dense_applies"], f["tail_launches"]) == (lt, dense, napply, nlaunch), (cid, vid, w, f)
        assert f["n"] == T[lt][0]
        # stage 1 and pc_apply go on with the same form of the tail
        a = after[w]
        assert (a["dense_applies"] > 0, a["tail_launches"] > 0) == (napply > 0, nlaunch > 0), (cid, vid, w, a)
    h.close()
    return got


_RUNS = {}


def variant(cid, vid):
    """The four results of a case under a variant's environment, computed once."""
    if (cid, vid) not in _RUNS:
        _RUNS[(cid, vid)] = run_variant(cid, vid, dict(variants_of(CASE[cid]))[vid])
    return _RUNS[(cid, vid)]


def default_variant(cid):
    return variant(cid, "default")


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_cycle_shapes_coarse_solves_and_truncation(cid):
    check_against_oracle(cid, reference(cid), default_variant(cid))


VARIANT_RUNS = [(c.id, vid, env) for c in CASES for vid, env in c.variants]


@pytest.mark.parametrize("cid,vid,env", VARIANT_RUNS, ids=["%s-%s" % v[:2] for v in VARIANT_RUNS])
def test_build_switch_variants(cid, vid, env):
    """The per-level kernels in place of the pairs and of the tail, the multilevel tail kernel in place of the dense operator, the
    tail's vectors in global memory: the same cycle, against the oracle and against the default kernels."""
    ref = reference(cid)
    base = default_variant(cid)
    got = variant(cid, vid)
    check_against_oracle("%s/%s" % (cid, vid), ref, got)
    d = [rel2(got[k], base[k]) for k in KEYS]
    print("%s/%s: against the default kernels: V-cycle p %.3e, V-cycle S~ %.3e, stage 1 %.3e, pc_apply %.3e" % ((cid, vid) + tuple(d)))
    assert max(d) < TOL, (cid, vid, d)
    if vid in BITWISE:
        same = variant(cid, BITWISE[vid])
        for k in KEYS:
            assert np.array_equal(got[k], same[k]), (cid, vid, BITWISE[vid], k)


@pytest.mark.parametrize("cid", ["v33", "pre0_post2_paired", "trunc3_big_level"])
def test_vcycle_is_repeatable(cid):
    """The cycle keeps no state between applications: x, another vector, x again -- first and third bitwise equal."""
    c, ref = CASE[cid], reference(cid)
    h = hip_engine(c, ref)
    h.vec_set("x", ref["x"])
    h.vec_set("z", np.random.default_rng(12).standard_normal(ref["x"].shape))
    for w, key in ((0, "vp"), (1, "vS")):
        out = []
        for src in ("x", "z", "x"):
            h.amg_vcycle(w, src, w, "y", w)
            out.append(h.vec_get("y")[w].copy())
        assert np.array_equal(out[0], out[2]), (cid, w)
        assert rel2(out[1], out[0]) > 1e-3
        assert rel2(out[0], ref[key]) < ref["tol"]
    h.close()


def test_trunc_changes_between_setups():
    """One live engine, amg_dom_tau = 0.07: S~ truncated at level 2 (dt 86.4), not at all (dt 8640), at level 2 again.  Each set-up
    resolves the level anew (amg_resolve_trunc), the captured pc_apply graph of the vector pair is not replayed across the change,
    and the dense tail of S~ is formed late, on the way to the first cycle that needs it."""
    from thermalporous_amd.engine import HipEngine
    c = CASE["trunc2_big_level"]
    spec, u0, *_ = c.builder(**c.kw)
    x = np.random.default_rng(11).standard_normal(np.shape(u0))
    h = HipEngine(spec, dict(pc="cptr", **c.opts))
    h.set_old(u0)
    got, seen = [], []
    for dt, amp, trunc in ((DT_DOM, AMP_DOM, 2), (DT, AMP, -1), (DT_DOM, AMP_DOM, 2)):
        o, _, _, u, _, _ = oracle_engine(c, dt=dt, amp=amp)
        assert trunc_of(o.pc.amg_T) == trunc and trunc_of(o.pc.amg_p) == -1
        h.set_dt(dt)
        h.set_state(u)
        h.jacobian()
        h.pc_setup()
        h.vec_set("x", x)
        h.amg_vcycle(1, "x", 1, "y", 1)
        vS = h.vec_get("y")[1].copy()
        h.pc_apply("x", "y")
        pc = h.vec_get("y").copy()
        d = rel2(vS, o.pc.amg_T.vcycle(x[1])), rel2(pc, o.pc.apply(x))
        info = h.amg_tail_info(1)
        print("dt %g: S~ truncated at %d; V-cycle S~ vs oracle %.3e, pc_apply %.3e; %s" % (dt, h.amg_trunc(1)[0], d[0], d[1], info))
        assert h.amg_trunc(1)[0] == trunc and h.amg_trunc(0)[0] == -1
        assert max(d) < TOL, (dt, d)
        got.append((vS, pc))
        seen.append((info["builds"], info["dense_applies"], info["tail_launches"]))
    h.close()
    # T of S~: not formed while the first cycles end above the tail; formed on the way to the first cycle of the second set-up
    # (amg_resolve_trunc) and applied by it and by the captured stage 1; formed once more by the third set-up, whose last
    # resolved shape reached the tail, and never applied after it
    assert seen[0] == (0, 0, 0) and seen[1][0] == 1 and seen[1][1] >= 2 and seen[2] == (2, seen[1][1], 0), seen
    assert rel2(got[1][0], got[0][0]) > 1e-3
    for a, b in zip(got[0], got[2]):
        assert np.array_equal(a, b)


def test_live_option_changes_rebuild_the_hierarchies():
    """tp_set_options drops the hierarchies, the next set-up builds the new plan: each pc_apply is the oracle's with those options,
    and back at the defaults the first result returns bit for bit."""
    from oracle.engine import DEFAULT_OPTS
    from thermalporous_amd.engine import HipEngine
    keys = ("amg_nu", "amg_full_levels", "amg_coarse_pre", "amg_coarse_post", "amg_min_cells")
    base = dict({k: DEFAULT_OPTS[k] for k in keys}, amg_dom_tau=0.0)
    steps = [dict(), dict(amg_nu=3), dict(amg_full_levels=0, amg_coarse_pre=0), dict(amg_min_cells=200), dict()]
    c = case("live", BOX, B11, dict(), lambda P, S: True)
    spec, u0, *_ = c.builder(**c.kw)
    u = cases.perturbed_state(spec, seed=SEED, amp=AMP)
    x = np.random.default_rng(11).standard_normal(u.shape)
    h = HipEngine(spec, dict(pc="cptr", **base))
    h.set_old(u0)
    h.set_dt(DT)
    h.set_state(u)
    h.jacobian()
    h.vec_set("x", x)
    got, nlev = [], []
    for step in steps:
        opts = dict(base, **step)
        o = oracle_engine(c, opts=opts)[0]
        h.set_options(**opts)
        h.pc_setup()
        h.pc_apply("x", "y")
        y = h.vec_get("y").copy()
        d = rel2(y, o.pc.apply(x))
        print("live options %s: pc_apply vs oracle %.3e" % (step, d))
        assert [h.amg_info(w)[0] for w in (0, 1)] == [len(o.pc.amg_p.levels), len(o.pc.amg_T.levels)]
        assert d < TOL, (step, d)
        got.append(y)
        nlev.append(h.amg_info(0)[0])
    h.close()
    assert nlev == [8, 8, 8, 6, 8]
    assert np.array_equal(got[0], got[-1])
    for k in (1, 2, 3):
        assert rel2(got[k], got[0]) > 1e-6, k


PAIR_CHILD_CASES = ("pre0_post2_paired", "default_shape")


def test_pair_switch_child(tmp_path):
    """TP_AMG_PAIR is read once per process: tests/scalar_amg_env_check.py runs the paired case and the default shape with only
    that variable set, in one child process, against the oracle, and hands its vectors back for the comparison with this
    process's paired kernels."""
    z = run_child("scalar_amg_env_check.py", {"TP_AMG_PAIR": "0"}, out=tmp_path/"pair0.npz", timeout=300)
    for cid in PAIR_CHILD_CASES:
        base = default_variant(cid)
        d = [rel2(z["%s/%s" % (cid, k)], base[k]) for k in KEYS]
        print("%s: TP_AMG_PAIR=0 against the default process: V-cycle p %.3e, V-cycle S~ %.3e, stage 1 %.3e, pc_apply %.3e"
              % ((cid,) + tuple(d)))
        for k in KEYS:      # measured on an MI355X: the same bits with and without the pairs
            assert np.array_equal(z["%s/%s" % (cid, k)], base[k]), (cid, k, d)
