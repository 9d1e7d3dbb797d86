"""numpy reference of the Schur factorisation types of the (p,T) split (schur_fact / schur_scale), composed from
the oracle's own pieces: the V-cycles of TwoStagePC's hierarchies, SelfpSchur.vcycle, spmv_scalar on the decoupled blocks and the
decoupling coefficients.  Not collected; imported by tests/test_schur_fact_host.py and tests/test_gpu_schur_fact.py.

PETSc's PCFIELDSPLIT schur, with r0, r1 the stage's right-hand sides after decoupling, K0 = K(A00), KS = K(S):

    full    y0 = K0 r0 ; y1 = KS (r1 - A10 y0) ; y0 = K0 (r0 - A01 y1)
    lower   y0 = K0 r0 ; y1 = KS (r1 - A10 y0)
    upper   y1 = KS r1 ; y0 = K0 (r0 - A01 y1)
    diag    y0 = K0 r0 ; y1 = scale KS r1            (scale: pc_fieldsplit_schur_scale, PETSc's default -1)
"""
import numpy as np

import oracle.linalg as la
import pc_order_ref as PR
from pc_order_ref import DT, ORDERS, oracle_system  # noqa: F401  (re-exported for the tests)

FACTS = ("full", "lower", "upper", "diag")

# the six systems of the measurements: (name, builder, grid, options); state perturbed_state(seed=5, amp=0.3), dt 8640
SYSTEMS = [
    ("c4_2ph_cptr", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr")),
    ("c4_2ph_cptr_a11", "c4_spe10_3d", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr", schur_a11=True)),
    ("c4_2ph_cptrQI", "c4_spe10_3d", dict(Nx=9, Ny=10, Nz=5, nphase=2), dict(pc="cptr", decoup="QI")),
    ("c3_1ph_cd", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="fieldsplit_cd")),
    ("c3_1ph_a11", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="fieldsplit_cd", schur_a11=True)),
    ("c3_1ph_selfp", "c3_spe10_2d", dict(Nx=14, Ny=19, nphase=1), dict(pc="fieldsplit_cd", schur_selfp=True)),
]
# Krylov iterations of the oracle FGMRES on J d = F per factorisation (full, lower, upper, diag with scale -1), recorded from this
# module alone (record_counts below); every solve ends with reason 2
COUNTS = {
    "c4_2ph_cptr": (12, 13, 25, 26),
    "c4_2ph_cptr_a11": (11, 11, 13, 15),
    "c4_2ph_cptrQI": (11, 12, 20, 19),
    "c3_1ph_cd": (6, 7, 8, 17),
    "c3_1ph_a11": (8, 6, 9, 17),
    "c3_1ph_selfp": (7, 8, 10, 18),
}


def stage1_rhs(pc, x):
    """(r0, r1): the right-hand sides TwoStagePC.stage1 forms from its argument."""
    s = x.shape[0] - 1
    if pc.d is None:
        return x[0], x[1]
    return x[0] - pc.d[0]*x[s], x[1] - pc.d[1]*x[s]


def ks_of(pc):
    """K(S) of the set-up preconditioner: SelfpSchur.vcycle under schur_selfp, else the V-cycle of the S~ / A11 hierarchy."""
    return pc.selfp.vcycle if getattr(pc, "selfp", None) is not None else pc.amg_T.vcycle


def stage1_fact(pc, x, fact, scale=-1.0, k0=None):
    """The Schur stage of the set-up oracle preconditioner pc (pc cptr or fieldsplit_cd) applied to x in the factorisation
    `fact`, following TwoStagePC.stage1: zero secondary fields.  k0: K(A00) where it is not one V-cycle (an inner solve)."""
    assert fact in FACTS, fact
    assert pc.o["pc"] in ("cptr", "fieldsplit_cd") and not pc.o.get("fs_additive")
    y = np.zeros_like(x)
    r0, r1 = stage1_rhs(pc, x)
    At, K0, KS = pc.At, k0 or pc.amg_p.vcycle, ks_of(pc)
    if fact == "upper":
        y1 = KS(r1)
        y0 = K0(r0 - la.spmv_scalar(At[:, 0, 1], y1))
    elif fact == "diag":
        y0, y1 = K0(r0), scale*KS(r1)
    else:
        y0 = K0(r0)
        y1 = KS(r1 - la.spmv_scalar(At[:, 1, 0], y0))
        if fact == "full":
            y0 = K0(r0 - la.spmv_scalar(At[:, 0, 1], y1))
    y[0], y[1] = y0, y1
    return y


class FactPC:
    """The oracle preconditioner with its S stage in the factorisation `fact`: what pc_order_ref.apply_seq and ctr_ref.apply_seq
    read (stage1, ilu, J)."""

    def __init__(self, pc, fact, scale=-1.0, k0=None):
        self.o, self.ilu, self.J = pc.o, pc.ilu, pc.J
        self.stage1 = lambda r: stage1_fact(pc, r, fact, scale, k0)


def apply_fact(pc, order, x, fact, scale=-1.0, k0=None):
    """The composite of `order` (pc_order_ref.apply_seq's loop) with every S stage in the factorisation `fact`; pc fieldsplit_cd
    has no second stage: the Schur stage is the preconditioner."""
    if pc.o["pc"] == "fieldsplit_cd":
        return stage1_fact(pc, x, fact, scale, k0)
    return PR.apply_seq(FactPC(pc, fact, scale, k0), order, x)


def fgmres_fact(o, J, F, fact, scale=-1.0, order="SI"):
    """The oracle FGMRES on J d = F preconditioned by apply_fact: (d, its, reason)."""
    d, its, reason, _ = la.fgmres(lambda v: la.spmv_block(J, v), lambda v: apply_fact(o.pc, order, v, fact, scale), F,
                                  rtol=o.opts["ksp_rtol"], maxit=o.opts["ksp_max_it"], restart=o.opts["ksp_restart"])
    return d, its, reason


def check_full_is_oracle(pc, x):
    """fact = "full" is the oracle's own TwoStagePC.stage1 / .apply, bit for bit."""
    assert np.array_equal(stage1_fact(pc, x, "full"), pc.stage1(x))
    assert np.array_equal(apply_fact(pc, "SI", x, "full"), pc.apply(x))


def reference_engine(fact, scale=-1.0):
    """An engine class for the model classes' _engine_factory: the oracle engine whose linear solves are preconditioned by
    apply_fact (the oracle itself knows the full factorisation only and ignores the key)."""
    from oracle.engine import OracleEngine

    class FactEngine(OracleEngine):
        def __init__(self, spec, opts=None):
            super().__init__(spec, opts)
            pc = self.pc
            pc.apply = lambda x: apply_fact(pc, "SI", x, fact, scale)
    return FactEngine


def record_counts():
    """{name: (its under full, lower, upper, diag)} of SYSTEMS, as committed in COUNTS."""
    out = {}
    for name, builder, kw, opts in SYSTEMS:
        *_, o, J, F = oracle_system(builder, kw, opts)
        res = [fgmres_fact(o, J, F, f) for f in FACTS]
        assert all(r[2] == 2 for r in res), (name, res)
        out[name] = tuple(int(r[1]) for r in res)
    return out


if __name__ == "__main__":
    for k, v in record_counts().items():
        print('    "%s": %r,' % (k, v))
