"""numpy reference of the composite's temperature stage (pc_ctr), composed from the oracle's own pieces: the
stages of tests/pc_order_ref.py plus one SemiAMG V-cycle on the T-T block of the undecoupled Jacobian.  Not collected; imported by
tests/test_ctr_host.py and tests/test_gpu_ctr.py.

PCCOMPOSITE multiplicative over a sequence of {S, I, T}:

    y = 0
    for k = 1..m:   r = x (k = 1) or x - J y (all rows, all columns of y);   y += B_{s_k} r

B_T r = (0, V(A_TT) r_T[, 0]): "y += B_T r" adds into field 1 only."""
import numpy as np

import oracle.linalg as la
import pc_order_ref as PR

SEQS = ("SIT", "IST", "ISIT", "SIST")
ORDER_OF = {"SIT": "SI", "IST": "IS", "ISIT": "ISI", "SIST": "SIS"}
DT = PR.DT
T2D = (1 << 30, 64, 1)

# the four systems of the table: (name, builder, grid, options); state perturbed_state(seed=5, amp=0.3), dt 8640
TABLE = [
    ("c3_1ph_cpr", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="cpr", ilu_tile=T2D)),
    ("c4_1ph_cprQI", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=1), dict(pc="cpr", decoup="QI")),
    ("c4_2ph_cprQI", "c4_spe10_3d", dict(Nx=9, Ny=10, Nz=5, nphase=2), dict(pc="cpr", decoup="QI")),
    ("c4_2ph_cptr", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr")),
]
# Krylov iterations of the oracle FGMRES on J d = F, recorded from the oracle alone (every run ends with reason 2)
COLUMNS = ("SI", "SIT", "IST", "ISIT", "SIST", "ISI", "SIS")
COUNTS = {"c3_1ph_cpr": (4, 2, 2, 2, 2, 3, 3), "c4_1ph_cprQI": (5, 1, 1, 1, 1, 2, 3),
          "c4_2ph_cprQI": (11, 11, 8, 7, 7, 8, 7), "c4_2ph_cptr": (12, 11, 10, 9, 8, 10, 9)}


def count(name, seq):
    return COUNTS[name][COLUMNS.index(seq)]


def make_ctr_amg(pc):
    """The T stage's hierarchy: a SemiAMG with TwoStagePC's keyword set and the temperature strengths prob.G (as
    TwoStagePC.amg_T has), set up on the T-T block of the UNDECOUPLED Jacobian pc.J."""
    o, prob = pc.o, pc.prob
    n = prob.n
    kw = dict(omega=o["amg_omega"], min_cells=o["amg_min_cells"], nu=o["amg_nu"], full_levels=o.get("amg_full_levels", 99),
              coarse_pre=o.get("amg_coarse_pre"), coarse_post=o.get("amg_coarse_post"), single=o.get("amg_single", False),
              tail_post=o.get("amg_tail_post"), mid_skip=o.get("amg_mid_skip", False), dom_tau=o.get("amg_dom_tau", 0.0))
    amg = la.SemiAMG(n, [prob.G[a] if n[a] > 1 else 0.0 for a in range(3)], **kw)
    amg.setup(pc.J[:, 1, 1])
    return amg


def apply_seq(pc, amgT, seq, x):
    """pc_order_ref.apply_seq extended by the letter T."""
    assert seq in SEQS + PR.ORDERS, seq
    y = np.zeros_like(x)
    for k, s in enumerate(seq):
        r = x if k == 0 else x - la.spmv_block(pc.J, y)
        if s == "T":
            y = y.copy()
            y[1] += amgT.vcycle(r[1])
        else:
            y = y + (pc.stage1(r) if s == "S" else pc.ilu.solve(r))
    return y


def row_rhs_ref(pc, x, y):
    """Row 1 of the block residual x - J y."""
    return (x - la.spmv_block(pc.J, y))[1]


def ctr_apply_ref(amgT, x):
    """CTRStage1PC.apply: y_T = V(A_TT) x_T, every other field zero."""
    y = np.zeros_like(x)
    y[1] = amgT.vcycle(x[1])
    return y


def fgmres_seq(o, amgT, J, F, seq):
    """The oracle FGMRES on J d = F preconditioned by the composite of `seq`: (d, its, reason)."""
    d, its, reason, _ = la.fgmres(lambda v: la.spmv_block(J, v), lambda v: apply_seq(o.pc, amgT, seq, v), F, rtol=o.opts["ksp_rtol"],
                                  maxit=o.opts["ksp_max_it"], restart=o.opts["ksp_restart"])
    return d, its, reason
