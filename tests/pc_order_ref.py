"""numpy reference of the composite preconditioner's stage orders (pc_order), composed from the oracle's own
pieces: TwoStagePC.stage1 (S), TwoStagePC.ilu.solve (I) and spmv_block.  Not collected; imported by tests/test_pc_order_host.py
and tests/test_gpu_pc_order.py.

PCCOMPOSITE multiplicative over a sequence s_1 .. s_m of {S, I}:

    y = 0
    for k = 1..m:   r = x (k = 1) or x - J y (all rows, all columns of y);   y += B_{s_k} r

B_S r = pc.stage1(r) has zero secondary fields, so "y += B_S r" adds into the primary fields only."""
import numpy as np

import cases
import oracle.linalg as la

ORDERS = ("SI", "IS", "ISI", "SIS")

# the small parity systems of the issue's table: (name, builder, grid, options); state perturbed_state(seed=5, amp=0.3), dt 8640
PARITY = [
    ("c4_2ph_cptr", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr")),
    ("c4_2ph_cprQI", "c4_spe10_3d", dict(Nx=9, Ny=10, Nz=5, nphase=2), dict(pc="cpr", decoup="QI")),
    ("c3_1ph_cpr", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="cpr", ilu_tile=(1 << 30, 64, 1))),
    ("c4_2ph_cptramg", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptramg")),
    ("c4_2ph_ilu1_tiles", "c4_spe10_3d", dict(Nx=11, Ny=13, Nz=17, nphase=2), dict(pc="cpr", ilu_levels=1, ilu_tile=(5, 4, 7))),
]
# Krylov iterations of the oracle FGMRES on J d = F per order (SI, IS, ISI, SIS), recorded from the oracle alone
COUNTS = {"c4_2ph_cptr": (12, 11, 10, 9), "c4_2ph_cprQI": (11, 9, 8, 7), "c3_1ph_cpr": (4, 4, 3, 3),
          "c4_2ph_cptramg": (15, 14, 14, 13), "c4_2ph_ilu1_tiles": (15, 11, 10, 9)}
DT = 8640.0


def apply_seq(pc, order, x):
    """The composite of `order` applied to x with the set-up oracle preconditioner pc (oracle.linalg.TwoStagePC)."""
    assert order in ORDERS, order
    y = np.zeros_like(x)
    for k, s in enumerate(order):
        r = x if k == 0 else x - la.spmv_block(pc.J, y)
        y = y + (pc.stage1(r) if s == "S" else pc.ilu.solve(r))
    return y


def stage_rhs_ref(pc, x, y):
    """The stage-1 right-hand sides of r = x - J y: r_q - sum_s d_{q,s} r_s per primary field q (what TwoStagePC.stage1 forms
    from its argument before it solves), shape (npri,) + grid."""
    r = x - la.spmv_block(pc.J, y)
    s = x.shape[0] - 1
    npri = 1 if pc.o["pc"] == "cpr" else 2
    if pc.d is None:
        return r[:npri].copy()
    if pc.o["decoup"] in ("QI_temp", "TI_temp"):
        return np.array([r[0] - pc.d[0][0]*r[1] - pc.d[0][1]*r[2]])
    return np.array([r[q] - pc.d[q]*r[s] for q in range(npri)])


def oracle_system(builder, kw, opts, seed=5, amp=0.3, dt=DT, nslabs=1):
    """(spec, u0, u, oracle engine with its preconditioner set up, J, F) of one parity system."""
    from oracle.engine import OracleEngine
    spec, u0, *_ = getattr(cases, builder)(**kw)
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    o = OracleEngine(spec, dict(opts, nslabs=nslabs) if nslabs > 1 else opts)
    o.set_old(u0)
    o.set_dt(dt)
    o.set_state(u)
    schur = opts["pc"] in ("cptr", "fieldsplit_cd")
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    o.pc.setup(J, Sm)
    F = o.residual()
    return spec, u0, u, o, J, F


def fgmres_seq(o, J, F, order):
    """The oracle FGMRES on J d = F preconditioned by the composite of `order`: (d, its, reason)."""
    d, its, reason, _ = la.fgmres(lambda v: la.spmv_block(J, v), lambda v: apply_seq(o.pc, order, v), F, rtol=o.opts["ksp_rtol"],
                                  maxit=o.opts["ksp_max_it"], restart=o.opts["ksp_restart"])
    return d, its, reason


def check_si_is_apply(pc, x):
    """apply_seq(pc, "SI", x) is the oracle's own TwoStagePC.apply, bit for bit."""
    assert np.array_equal(apply_seq(pc, "SI", x), pc.apply(x))
