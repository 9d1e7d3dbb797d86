"""ctypes binding of libthermalporous_hip.so -- the compute engine behind SinglePhase/TwoPhase.solve().

This is the FFI stub a maintainer of the reference would add: the reference reaches
its native hot path through petsc4py/Firedrake at ``self.solver.solve()``
(/root/reference/thermalporous/thermalmodel.py:165); here the same call lands in ``tp_newton_solve``.
There is NO CPU fallback: without the HIP library or without a GPU the engine raises.

Slab layout: each rank owns planes [off2, off2+n2) along internal axis 2 and stores every cell array
with one halo plane per side (include/thermalporous_hip.h).
"""
import ctypes as C
import math
import os

import numpy as np

from .boundary import KINDS, pack_values
from .physicalparameters import SATFN_NUMBERS, check_satfn, satfn_is_default

_LIB = None
_LIBPATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libthermalporous_hip.so")


class EngineError(RuntimeError):
    pass


class tp_grid(C.Structure):
    _fields_ = [("n0", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("gn2", C.c_int32), ("off2", C.c_int32),
                ("h", C.c_double*3), ("gaxis", C.c_int32), ("nphase", C.c_int32), ("rank", C.c_int32),
                ("nranks", C.c_int32)]


class tp_params(C.Structure):
    _names = ("ko", "kw", "kr", "c_v_w", "c_v_o", "c_r", "rho_r", "p_inj", "p_prod", "T_inj", "T_prod", "API",
              "p_ref", "g", "S_o", "U", "rate")
    _fields_ = [(k, C.c_double) for k in _names]


class tp_source(C.Structure):
    _fields_ = [("cell", C.c_int64), ("kind", C.c_int32), ("constant_rate", C.c_int32), ("wt", C.c_double),
                ("bhp", C.c_double), ("max_rate", C.c_double), ("WI", C.c_double)]


class tp_options(C.Structure):
    _fields_ = [("pc_kind", C.c_int32), ("decoup", C.c_int32), ("ksp_rtol", C.c_double), ("ksp_atol", C.c_double),
                ("ksp_max_it", C.c_int32), ("ksp_restart", C.c_int32), ("snes_rtol", C.c_double),
                ("snes_atol", C.c_double), ("snes_stol", C.c_double), ("snes_max_it", C.c_int32),
                ("amg_omega", C.c_double), ("amg_nu", C.c_int32), ("amg_min_cells", C.c_int32),
                ("ilu_t1", C.c_int32), ("ilu_t2", C.c_int32), ("ilu_t0", C.c_int32),
                ("amg_full_levels", C.c_int32), ("amg_coarse_pre", C.c_int32), ("amg_coarse_post", C.c_int32),
                ("amg_mid_skip", C.c_int32), ("amg_tail_post", C.c_int32), ("amg_single", C.c_int32), ("schur_a11", C.c_int32), ("amg_gather_cells", C.c_int32),
                ("schur_fact", C.c_int32), ("schur_scale", C.c_double), ("amg_dom_tau", C.c_double),
                ("ilu_levels", C.c_int32), ("pc_ctr", C.c_int32), ("fs_additive", C.c_int32), ("pc_order", C.c_int32),
                ("ksp_reorth", C.c_int32), ("ksp_reorth_eta", C.c_double),
                ("ksp_ew", C.c_int32), ("ew_rtol0", C.c_double), ("ew_rtolmax", C.c_double), ("ew_gamma", C.c_double),
                ("ew_alpha", C.c_double), ("ew_alpha2", C.c_double), ("ew_threshold", C.c_double), ("ilu_whole", C.c_int32),
                ("amg_gs_levels", C.c_int32), ("amg_gs_sweeps", C.c_int32),
                ("ilu_block", C.c_int32*3), ("ilu_single", C.c_int32),
                ("ls_kind", C.c_int32), ("ls_order", C.c_int32), ("ls_max_it", C.c_int32), ("ls_alpha", C.c_double),
                ("ls_maxstep", C.c_double), ("ls_minlambda", C.c_double), ("ls_max_change", C.c_double*3),
                ("amg_line_levels", C.c_int32),
                ("ksp_basis_single", C.c_int32), ("ksp_single_floor", C.c_double), ("ksp_kind", C.c_int32),
                ("s1_ksp", C.c_int32), ("s1_max_it", C.c_int32), ("s1_rtol", C.c_double), ("s1_atol", C.c_double)]


class tp_solve_info(C.Structure):
    _fields_ = [("nits", C.c_int32), ("lits", C.c_int32), ("reason", C.c_int32), ("last_ksp_reason", C.c_int32),
                ("fnorm0", C.c_double), ("fnorm", C.c_double), ("vcycles", C.c_int32)]


class tp_satfn(C.Structure):
    _fields_ = [("relperm", C.c_int32), ("capillary", C.c_int32), ("Sr_o", C.c_double), ("Sr_w", C.c_double),
                ("n_o", C.c_double), ("n_w", C.c_double), ("kro_max", C.c_double), ("krw_max", C.c_double),
                ("lmbda", C.c_double), ("p_ct", C.c_double), ("pc_se_min", C.c_double)]


class tp_well(C.Structure):
    _fields_ = [("kind", C.c_int32), ("shut", C.c_int32), ("rate", C.c_double), ("bhp_limit", C.c_double), ("z_ref", C.c_double),
                ("first", C.c_int32), ("count", C.c_int32)]


class tp_perf(C.Structure):
    _fields_ = [("cell", C.c_int64), ("WI", C.c_double), ("z", C.c_double)]


class tp_well_state(C.Structure):
    _fields_ = [("bhp", C.c_double), ("mode", C.c_int32), ("rounds", C.c_int32), ("rate", C.c_double), ("water_rate", C.c_double),
                ("oil_rate", C.c_double), ("rho", C.c_double), ("nopen", C.c_int32), ("reserved", C.c_int32)]


WELL_KINDS = {"prod": 0, "inj": 1, 0: 0, 1: 1}
WELL_MODES = {0: "shut", 1: "rate", 2: "bhp"}

# every symbol include/thermalporous_hip.h declares (tests check that the library exports them all)
API_SYMBOLS = (
    "tp_last_error", "tp_version", "tp_create", "tp_destroy", "tp_set_options", "tp_comm_unique_id", "tp_comm_init",
    "tp_local_group_create", "tp_local_group_destroy", "tp_comm_init_local",
    "tp_set_field", "tp_finalize_fields", "tp_set_sources", "tp_set_state", "tp_get_state", "tp_set_old_state",
    "tp_set_dt", "tp_get_old_state", "tp_restore_state", "tp_saturation_range", "tp_clamp_saturation",
    "tp_residual", "tp_jacobian", "tp_get_residual", "tp_export_jacobian", "tp_export_schur",
    "tp_well_rates", "tp_vec_create", "tp_vec_create_batch", "tp_vec_dot_batch", "tp_vec_axpy_batch", "tp_vec_norm2", "tp_set_ksp_monitor", "tp_vec_set", "tp_vec_get", "tp_vec_copy_residual", "tp_spmv", "tp_pc_setup",
    "tp_pc_apply", "tp_stage1_update", "tp_stage1_apply", "tp_ilu0_factor", "tp_ilu0_solve", "tp_ilu_layout", "tp_amg_setup",
    "tp_amg_vcycle", "tp_schur_apply", "tp_fgmres", "tp_newton_solve", "tp_time_kernel", "tp_amg_info", "tp_amg_layout", "tp_amg_trunc",
    "tp_inner_stats", "tp_amg_tail_info", "tp_ilu_factor_bytes", "tp_amg_line_info", "tp_bcgs", "tp_ksp_info",
    "tp_ksp_basis_info", "tp_fvec_create_batch", "tp_fvec_store", "tp_fvec_get", "tp_fvec_dot_batch", "tp_fvec_axpy_batch",
    "tp_ls_info", "tp_ls_history", "tp_ls_step_stats", "tp_ls_trial", "tp_amg_gs_info", "tp_vec_orth_step", "tp_ksp_reorth_info",
    "tp_stage_rhs", "tp_ew_next_rtol", "tp_ew_info", "tp_ew_history", "tp_ctr_rhs", "tp_ctr_apply", "tp_ctr_info",
    "tp_schur_info", "tp_set_boundary", "tp_boundary_flux", "tp_set_spacing", "tp_spacing_info",
    "tp_set_saturation_functions", "tp_saturation_info",
    "tp_set_wells", "tp_set_well_control", "tp_well_info", "tp_well_perf_rates", "tp_well_factors",
    "tp_switch_count", "tp_switch_entry",
)

DEFAULT_OPTS = dict(
    pc="cpr", decoup="No",
    pc_order="SI",          # order of the composite's stages, S = the CPR / CPTR / system-AMG stage, I = bjacobi + block-ILU: "SI" (the
                            # presets' order) | "IS" | "ISI" | "SIS" -- PCCOMPOSITE multiplicative, a block residual over all fields between
                            # two stages (pc_composite_pcs "bjacobi,fieldsplit", ...; check_pc_order_options).  Not pc fieldsplit_cd / bilu
    pc_ctr=False,           # True: one more stage T behind the last stage of pc_order (SIT, IST, ISIT, SIST), y_T += V(A_TT) [x - J y]_T, one
                            # V-cycle on the T-T block of the undecoupled Jacobian (the reference's cprctr composites, CTRStage1PC).  pc cpr
                            # and cptr only, one slab (check_pc_ctr_options)
    ksp_rtol=1e-7, ksp_atol=1e-50, ksp_max_it=200, ksp_restart=200,
    ksp="fgmres",           # outer Krylov method: "fgmres" (restarted, ksp_restart) | "bcgs": right-preconditioned BiCGStab, seven vectors
                            # plus the shared scratch w2 whatever the iteration count, two preconditioner applications per iteration (tp_options.ksp_kind)
    ksp_basis_single=False, # FGMRES only: the bases V and Z stored in fp32, compact (compressed-basis GMRES), all arithmetic fp64: half the
                            # Krylov workspace and half the bytes Gram-Schmidt moves; convergence only on a recomputed true residual
    ksp_single_floor=1e-7,  # theta of ksp_basis_single, in (2^-24, 1): a restart cycle ends once its recurrence residual has fallen
                            # to theta times the true residual it started from (check_ksp_basis_options)
    ksp_reorth="never",     # FGMRES, fp64 bases: a second classical Gram-Schmidt pass (CGS2) per iteration -- "never" | "ifneeded" (when
                            # the first pass left less than ksp_reorth_eta of the vector's length) | "always"; decided and predicated
                            # on the device, no further host wait (ksp_gmres_cgs_refinement_type; check_ksp_reorth_options)
    ksp_reorth_eta=2.0**-0.5,   # eta of "ifneeded", in (0, 1): refine when ||w - V h|| < eta ||w|| (the DGKS / Rutishauser value)
    snes_rtol=1e-8, snes_atol=1e-50, snes_stol=1e-8, snes_max_it=15,
    amg_omega=0.9,          # damped-Jacobi weight (round 3: 0.8 -> 0.9 buys 3 % fewer Krylov iterations on C4 at equal cycle cost, +4 % Newton steps/s
                            # over 80 time steps, measured twice; 0.88-0.9 is a plateau, 0.95 starts to fail solves, 1.0 loses 40 %; C1-C3 neutral)
    amg_min_cells=64, amg_nu=2, amg_full_levels=3, amg_coarse_pre=0, amg_coarse_post=1, amg_mid_skip=True, amg_tail_post=2, amg_single=False,
    amg_dom_tau=0.25,       # relaxation-only truncation of diagonally dominant AMG hierarchies (oracle/linalg.py:SemiAMG)
    amg_line_levels=0,      # L: line-Jacobi along internal axis 0 (Thomas solve per line) instead of point Jacobi on the first L levels of
                            # the scalar hierarchies that lie above the single-workgroup tail (L <= amg_full_levels).  0: off.  One slab,
                            # fp64 operators, not pc cptramg, not schur_selfp (check_amg_line_options)
    amg_gs_levels=0,        # L: red-black Gauss-Seidel (no damping, amg_omega unused) instead of damped Jacobi on the first L levels of the
                            # scalar hierarchies that lie above the single-workgroup tail (L <= amg_full_levels); such a level is V(g, g) with
    amg_gs_sweeps=1,        # g = 1..4 sweeps per leg: forward (red, black) before the coarse correction, backward (black, red) after it.
                            # L = 0: off (g must then be 1).  One slab, fp64 operators, not amg_line_levels, pc cptramg or schur_selfp
                            # (check_amg_gs_options)
    # multi-GPU: AMG levels with more cells than this stay distributed over the slabs.  Cost model: a V(2,2)
    # level streams ~6 sweeps x 104 B per cell (5.5 TB/s on one GPU) and needs 6 halo exchanges when distributed; with N
    # slabs it saves (1 - 1/N) of its streaming time and pays 6 x t_exchange (~10 us per grouped RCCL send/recv): the
    # break-even is ~0.6 M cells, so C4's level 0 (1.12 M cells) is distributed, its level 1 (0.56 M) is gathered
    amg_gather_cells=600000,
    schur_a11=False,
    fs_additive=False,      # pc_fieldsplit_type additive on (p,T): pc_fieldsplit_diag (singlephase.py:371-375)
    schur_selfp=False,      # pc_fieldsplit_schur_precondition selfp (pc_fieldsplit_selfp, singlephase.py:322-330)
    schur_fact="full",      # factorisation of the Schur split on (p,T) (pc_fieldsplit_schur_fact_type): "full" (the presets': K(A00) twice,
                            # K(S) once) | "lower" (y0 = K0 r0, y1 = KS (r1 - A10 y0)) | "upper" (y1 = KS r1, y0 = K0 (r0 - A01 y1)) | "diag"
                            # (y0 = K0 r0, y1 = schur_scale KS r1): one K(A00) each.  pc cptr and fieldsplit_cd, not fs_additive
                            # (check_schur_fact_options)
    schur_scale=-1.0,       # "diag" only: the factor on K(S) r1 (pc_fieldsplit_schur_scale, PETSc's default -1); must stay -1 otherwise
    ilu_tile=None,          # None: see default_ilu_tile (3-D: whole axis-0 lines x a balanced t1 x t2; 2-D: ~24 x 32 cells)
    ilu_levels=0,           # sub_1_sub_pc_factor_levels: 0 (block-ILU(0)) or 1 (block-ILU(1), pc_cprilu1_gmres)
    bjacobi_blocks=None,    # -sub_1_pc_bjacobi_blocks N: N blocks over the whole grid; overrides ilu_tile.  One tile per block when
                            # such tiles fit a wavefront (tiles_for_blocks), else boxes of several tiles (blocks_for_count -> ilu_block)
    ilu_block=None,         # bjacobi block as a box (B0, B1, B2) of cells, independent of ilu_tile (1 << 30: the whole extent):
                            # block-ILU(0) inside each box, its tiles swept one block-local tile-diagonal per launch; restarts
                            # at every slab.  None: every tile is a block
    ilu_single=False,       # the ILU(0) factor stream stored in fp32, everything else fp64 (as amg_single for the AMG): half the
                            # factor's memory; the default per-tile ILU(0) only (not with ilu_levels 1, ilu_whole, multi-tile ilu_block)
    ilu_whole=False,        # one bjacobi block per rank: block-ILU(0) of the whole slab (= bjacobi_blocks 1 on one GPU, PETSc's
                            # default bjacobi on several); ilu_tile is then only the unit of the diagonal-by-diagonal sweep
    # inner solve of the stage-1 pressure block K(A00) (pc cptramg: of the (p,T) system block), the V-cycle as its
    # preconditioner, every scalar on the device (include/thermalporous_hip.h: tp_options.s1_ksp)
    s1_ksp="preonly",       # "preonly": one V-cycle | "richardson": s1_max_it V-cycles from x0 = 0 | "fgmres": GMRES(s1_max_it <= 32)
    s1_max_it=1,
    s1_rtol=0.0, s1_atol=0.0,   # fgmres: latch on the recurrence residual <= max(s1_rtol*||rhs||, s1_atol); 0, 0 = fixed count
    # line search of the Newton solver (include/thermalporous_hip.h: tp_options.ls_kind; check_linesearch_options)
    linesearch="basic",     # "basic": every correction at full length | "bt": Armijo backtracking (snes_linesearch_type bt)
    ls_order=3,             # bt: 2 quadratic | 3 cubic interpolation of the next trial length
    ls_alpha=1e-4,          # bt: Armijo parameter in (0, 0.5)
    ls_max_it=40,           # bt: most trials per Newton iteration
    ls_maxstep=1e8,         # bt: first trial length <= ls_maxstep / ||dx||
    ls_minlambda=1e-12,     # bt: absolute smallest trial length, in [0, 1)
    ls_max_change=None,     # bt: (dp, dT, dS) caps on the change of p, T, S_o per Newton iteration (<= 0: no cap); None: off
    # Eisenstat-Walker inexact Newton (include/thermalporous_hip.h: tp_options.ksp_ew; check_ew_options): the tolerance of every
    # linear solve of a Newton solve chosen from the nonlinear residuals, ksp_rtol kept as its floor (snes_ksp_ew)
    ksp_ew=False,           # False / 0: every linear solve to ksp_rtol | 1 | 2: the version (True: 2, PETSc's default)
    ew_rtol0=0.3,           # eta of the first linear solve, in [0, 1)
    ew_rtolmax=0.9,         # cap on eta, in [0, 1); ksp_rtol may not exceed it
    ew_gamma=1.0,           # version 2: eta = gamma (||F_k|| / ||F_k-1||)^alpha, gamma in [0, 1]
    ew_alpha=(1.0 + math.sqrt(5.0))/2.0,    # version 2: alpha in (1, 2]
    ew_alpha2=(1.0 + math.sqrt(5.0))/2.0,   # version 1: the safeguard's exponent, in (1, 2]
    ew_threshold=0.1,       # the safeguard acts when its term exceeds this, in (0, 1)
)
# the keys a PETSc-style solver_parameters dict may carry straight through to the engine (solver_options.engine_options)
BUILD_KEYS = ("amg_omega", "amg_nu", "amg_min_cells", "amg_full_levels", "amg_coarse_pre", "amg_coarse_post", "amg_mid_skip",
              "amg_tail_post", "amg_single", "ilu_single", "amg_line_levels", "amg_gs_levels", "amg_gs_sweeps",
              "amg_gather_cells", "amg_dom_tau", "ilu_tile", "ilu_levels", "ilu_whole", "ilu_block",
              "s1_ksp", "s1_max_it", "s1_rtol", "s1_atol", "ksp_basis_single", "ksp_single_floor", "ksp_reorth", "ksp_reorth_eta",
              "pc_order", "pc_ctr", "schur_fact", "schur_scale", "linesearch", "ls_order", "ls_alpha", "ls_max_it", "ls_maxstep",
              "ls_minlambda", "ls_max_change", "ksp_ew", "ew_rtol0", "ew_rtolmax", "ew_gamma", "ew_alpha", "ew_alpha2", "ew_threshold")
_LS = {"basic": 0, "bt": 1}
_LS_KEYS = ("ls_order", "ls_alpha", "ls_max_it", "ls_maxstep", "ls_minlambda", "ls_max_change")
_EW_KEYS = ("ew_rtol0", "ew_rtolmax", "ew_gamma", "ew_alpha", "ew_alpha2", "ew_threshold")


def _opt(o, k):
    """o[k], or the default of a key the dict does not carry."""
    return o.get(k, DEFAULT_OPTS[k])


def _is_number(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def ew_version(v):
    """ksp_ew as the version in effect: False / 0 -> 0 (off), True -> 2, 1 | 2 -> itself; 3 is PETSc's third version, not
    implemented; anything else is a ValueError."""
    if v is None or v is False or (isinstance(v, np.bool_) and not v):
        return 0
    if v is True or (isinstance(v, np.bool_) and v):
        return 2
    if _is_number(v) and float(v) == int(v):
        if int(v) == 3:
            raise NotImplementedError("ksp_ew = 3 (snes_ksp_ew_version 3) is not implemented: it needs the line search's predicted "
                                      "and actual reduction; versions 1 and 2 are")
        if int(v) in (0, 1, 2):
            return int(v)
    raise ValueError("ksp_ew = %r: False / 0 (off), 1, 2 or True (= 2)" % (v,))


def check_ew_options(o):
    """ksp_ew and the ew_* keys (tp_options.ksp_ew ...): ranges (PETSc's) with the option on; off, every ew_* key must keep its
    default -- a value that would be ignored is refused."""
    ver = ew_version(_opt(o, "ksp_ew"))
    vals = {k: _opt(o, k) for k in _EW_KEYS}
    if ver == 0:
        for k in _EW_KEYS:
            if isinstance(vals[k], (bool, np.bool_)) or vals[k] != DEFAULT_OPTS[k]:
                raise ValueError("%s = %r with ksp_ew off: the key belongs to Eisenstat-Walker (it would be ignored)" % (k, vals[k]))
        return
    for k, v in vals.items():
        if not _is_number(v) or float(v) != float(v):
            raise ValueError("%s = %r: a number" % (k, v))
    for k in ("ew_rtol0", "ew_rtolmax"):
        if not 0.0 <= float(vals[k]) < 1.0:
            raise ValueError("%s = %r: a number in [0, 1)" % (k, vals[k]))
    if not 0.0 <= float(vals["ew_gamma"]) <= 1.0:
        raise ValueError("ew_gamma = %r: a number in [0, 1]" % (vals["ew_gamma"],))
    for k in ("ew_alpha", "ew_alpha2"):
        if not 1.0 < float(vals[k]) <= 2.0:
            raise ValueError("%s = %r: a number in (1, 2]" % (k, vals[k]))
    if not 0.0 < float(vals["ew_threshold"]) < 1.0:
        raise ValueError("ew_threshold = %r: a number in (0, 1)" % (vals["ew_threshold"],))
    if float(_opt(o, "ksp_rtol")) > float(vals["ew_rtolmax"]):
        raise ValueError("ksp_rtol = %r exceeds ew_rtolmax = %r: ksp_rtol is the floor of the Eisenstat-Walker tolerance and "
                         "would lie above its cap" % (_opt(o, "ksp_rtol"), vals["ew_rtolmax"]))


def check_linesearch_options(o):
    """linesearch and the ls_* keys (tp_options.ls_kind ...): ranges under "bt"; under "basic" every ls_* key must keep its
    default -- a value that would be ignored is refused."""
    kind = _opt(o, "linesearch")
    if kind not in _LS:
        raise NotImplementedError("linesearch = %r: 'basic' or 'bt'" % (kind,))
    mc = o.get("ls_max_change")
    if mc is not None:
        mc = tuple(mc)
        if len(mc) != 3 or not all(_is_number(v) and float(v) == float(v) for v in mc):
            raise ValueError("ls_max_change = %r: None or a (dp, dT, dS) triple of numbers (<= 0: no cap on that field)" % (o["ls_max_change"],))
    if kind == "basic":
        for k in _LS_KEYS:
            v = _opt(o, k)
            if k == "ls_max_change":
                if mc is not None and any(float(x) > 0 for x in mc):
                    raise ValueError("ls_max_change = %r with linesearch = 'basic': the key belongs to the bt search" % (v,))
            elif v != DEFAULT_OPTS[k]:
                raise ValueError("%s = %r with linesearch = 'basic': the key belongs to the bt search" % (k, v))
        return
    order, it = _opt(o, "ls_order"), _opt(o, "ls_max_it")
    if isinstance(order, (bool, np.bool_)) or order not in (2, 3):
        raise ValueError("ls_order = %r: 2 (quadratic) or 3 (cubic)" % (order,))
    if not _is_number(it) or int(it) != it or it < 1:
        raise ValueError("ls_max_it = %r: a count >= 1" % (it,))
    a, ms, ml = _opt(o, "ls_alpha"), _opt(o, "ls_maxstep"), _opt(o, "ls_minlambda")
    if not _is_number(a) or not 0.0 < float(a) < 0.5:
        raise ValueError("ls_alpha = %r: a number in (0, 0.5)" % (a,))
    if not _is_number(ms) or not float(ms) > 0.0:
        raise ValueError("ls_maxstep = %r: a number > 0" % (ms,))
    if not _is_number(ml) or not 0.0 <= float(ml) < 1.0:
        raise ValueError("ls_minlambda = %r: a number in [0, 1)" % (ml,))

def default_ilu_tile(n, nslabs=1, ncu=256):
    """bjacobi tile (t0, t1, t2) for a grid of internal extents n = (n0, n1, n2) cut into `nslabs` slabs along axis 2.
    2-D: 32 columns (measured on C3 60x220: 64-wide tiles cost 123 wavefront steps for 60 cells of depth, 32-wide ones
    91 steps and +0.5 % Krylov iterations) x pieces of ~24 cells of the axis-0 lines (below).  3-D: whole axis-0 lines
    (the thin, strongly coupled direction; the sweeps are bandwidth bound there and shorter tiles only add fill/drain steps) x the t1 x t2 (32..64 columns, each side
    4..16) that minimises the sweep time of the busiest CU: one wavefront = one CU streams a tile's
    (n0 + t1 + t2 - 2) steps x t1*t2 lanes of factor data at the per-CU HBM rate, and `ncu` CUs work at a time --
    cost = ceil(tiles / ncu) * steps * lanes * (1 + |t1 - t2| / 100)  (elongated tiles cut more couplings per cell);
    ties go to the larger tile.  C4 (85 x 60 x 220): 6 x 9 -> 250 full tiles on 256 CUs, 54 lanes x 98 steps, instead of
    224 tiles of 8 x 8 (64 lanes x 99 steps, the 8th tile across half empty): 17 % fewer bytes through the busiest CU."""
    n0, n1, n2 = (int(v) for v in n)
    if n2 == 1:
        # 2-D sweeps are bound by their NUMBER OF STEPS (t0 + t1 - 1 dependent wavefront steps of ~0.3 us, a handful of
        # waves on the whole chip), not by bytes: cutting the lines into pieces of ~24 cells makes C1 (400 x 400) 67 %
        # faster at +8 % Krylov iterations (71 -> 119 Newton steps/s) and C3 (60 x 220) 12 % faster at equal counts
        return (-(-n0//max(1, -(-n0//24))), 32, 1)
    n2l = -(-n2//max(1, int(nslabs)))
    best = None
    for t1 in range(min(4, n1), min(16, n1) + 1):
        for t2 in range(min(4, n2l), min(16, n2l) + 1):
            lanes = t1*t2
            if lanes > 64 or (lanes < 32 and (t1 < min(16, n1) or t2 < min(16, n2l))):
                continue
            tiles = -(-n1//t1)*-(-n2l//t2)
            cost = -(-tiles//ncu)*(n0 + t1 + t2 - 2)*lanes*(1.0 + 0.01*abs(t1 - t2))
            key = (cost, -lanes, abs(t1 - t2))
            if best is None or key < best[0]:
                best = (key, (1 << 30, t1, t2))
    if best is None:
        return (1 << 30, min(n1, 8), min(n2l, 8))
    return best[1]


def whole_ilu_tile(n, nslabs=1):
    """Sweep unit (t0, t1, t2) of the whole-slab ILU(0) (``ilu_whole``): the tiles no longer cut couplings, they are swept
    one tile-diagonal T0 + T1 + T2 = d per launch.  3-D: the balanced t1 x t2 of default_ilu_tile, and the axis-0 lines cut
    into pieces of ~16 cells -- a diagonal of the 3-D tile grid holds up to nt0*nt1 tiles instead of nt1, and a launch
    lasts t0 + t1 + t2 - 2 wavefront steps instead of n0 + t1 + t2 - 2 (C4: 39 launches of ~29 steps per direction instead
    of 34 of 98).  2-D: the 24 x 32 tiles of the default."""
    n0, n1, n2 = (int(v) for v in n)
    t = default_ilu_tile(n, nslabs=nslabs)
    if n2 == 1:
        return t
    return (-(-n0//max(1, -(-n0//16))), t[1], t[2])


def block_ilu_tile(block):
    """Sweep unit (t0, t1, t2) for bjacobi blocks of extents `block` (``ilu_block``): the rule of whole_ilu_tile applied to
    ONE block, which is swept exactly as a whole slab of that size is -- every block contributes its tiles of block-local
    diagonal d to launch d, so the launch count follows the block's tile grid and the tiles per launch the number of blocks."""
    return whole_ilu_tile(tuple(int(v) for v in block), nslabs=1)


def blocks_for_count(n, nblocks):
    """Box (B0, B1, B2) that cuts the grid n into exactly `nblocks` bjacobi blocks of ANY size (``-sub_1_pc_bjacobi_blocks``):
    the rule of tiles_for_blocks without the one-wavefront limit -- whole axis-0 lines first, then the most compact box.
    Raises NotImplementedError when no box tiling gives that count."""
    return tiles_for_blocks(n, nblocks, max_cols=None)


def check_ilu_single_options(o, exc=EngineError, whole_is="", ext=None):
    """ilu_single against the stage-2 variants that keep doubles: the fp32 factor stream exists for the default per-tile
    block-ILU(0) only (tp_options.ilu_single), no silent doubles.  ext: the extents of a slab, with which the rule that depends on
    the grid -- an ilu_block of several tiles, on resolved options -- is checked as well."""
    if not o.get("ilu_single"):
        return
    if int(_opt(o, "ilu_levels")) != 0:
        raise exc("ilu_single with ilu_levels = %r: the fp32 factor is implemented for block-ILU(0)" % (o["ilu_levels"],))
    if o.get("ilu_whole"):
        raise exc("ilu_single with ilu_whole%s: the fp32 factor is implemented for one tile per bjacobi block" % whole_is)
    if ext is not None and o.get("ilu_block") is not None:
        box = [min(o["ilu_block"][a], ext[a]) for a in range(3)]
        if any(-(-box[a]//max(1, min(int(o["ilu_tile"][a]), box[a]))) > 1 for a in range(3)):
            raise exc("ilu_single with an ilu_block of several tiles (block %r, tile %r): the fp32 factor is "
                      "implemented for one tile per bjacobi block" % (tuple(box), tuple(o["ilu_tile"])))


def resolve_ilu_options(opts, n, nranks=1):
    """Stage-2 layout options (ilu_tile, ilu_whole, ilu_block) of an engine on grid n = (n0, n1, n2) cut into `nranks` slabs,
    from the user's options (a copy is returned).  ``bjacobi_blocks = N``: N = nranks is one block per rank (ilu_whole); on one
    rank, N tiles when a tile of that size fits one wavefront, else N boxes of several tiles (ilu_block, with the sweep tile
    of block_ilu_tile); on several slabs any other count is refused.  An explicit ilu_block is taken as given."""
    o = dict(opts)
    nranks = int(nranks)
    if o.get("bjacobi_blocks") is not None:
        # PETSc counts blocks over ALL ranks and needs at least one per rank: N blocks on N slabs = one per rank
        if int(o["bjacobi_blocks"]) == nranks:
            o["ilu_whole"] = True
        elif nranks > 1:
            raise EngineError("bjacobi_blocks counts blocks over the whole grid: on multi-slab runs only one block per "
                              "rank (bjacobi_blocks = number of slabs, or ilu_whole) or an explicit ilu_tile / ilu_block")
        else:
            try:
                o["ilu_tile"] = tiles_for_blocks(n, o["bjacobi_blocks"], max_cols=64)
            except NotImplementedError:
                o["ilu_block"] = blocks_for_count(n, o["bjacobi_blocks"])
                o["ilu_tile"] = None
    blk = o.get("ilu_block")
    if blk is not None:
        blk = tuple(int(v) for v in blk)
        if len(blk) != 3 or min(blk) < 1:
            raise ValueError("ilu_block is a triple of extents >= 1 (1 << 30: the whole extent)")
        if o.get("ilu_whole"):
            raise EngineError("ilu_whole (one block per rank) and ilu_block exclude one another")
        o["ilu_block"] = blk
    if o.get("ilu_tile") is None:
        n2l = -(-int(n[2])//max(1, nranks))
        if blk is not None:
            o["ilu_tile"] = block_ilu_tile((min(blk[0], int(n[0])), min(blk[1], int(n[1])), min(blk[2], n2l)))
        else:
            o["ilu_tile"] = (whole_ilu_tile if o.get("ilu_whole") else default_ilu_tile)(n, nslabs=nranks)
    check_ilu_single_options(o, whole_is=" (one block per rank, bjacobi_blocks = number of slabs)",
                             ext=(int(n[0]), int(n[1]), -(-int(n[2])//max(1, nranks))))
    return o


def tiles_for_blocks(n, nblocks, max_cols=64):
    """Tile (t0, t1, t2) that cuts the grid n = (n0, n1, n2) into exactly `nblocks` boxes = bjacobi blocks
    (``-sub_1_pc_bjacobi_blocks``, /root/reference/tests/test_homo_wells.py:112,125).  PETSc's blocks are contiguous row
    ranges of its field-major DMPlex ordering, which has no counterpart here; the build's blocks are boxes of whole
    cells, whole axis-0 lines when possible.  A GPU tile is swept by one wavefront: at most `max_cols` = 64 columns
    (t1*t2); None lifts the limit (CPU oracle).  Raises NotImplementedError when no such tiling exists."""
    n0, n1, n2 = (int(v) for v in n)
    nblocks = int(nblocks)
    if nblocks < 1:
        raise ValueError("bjacobi_blocks must be >= 1")
    best = None
    if nblocks == 1 and max_cols is not None and n1*n2 > max_cols:
        raise NotImplementedError("one block over a grid of more than %d columns is not a single tile: the GPU engine realises "
                                  "it as ilu_whole (whole-slab ILU(0) swept tile-diagonal by tile-diagonal)" % max_cols)
    for k2 in range(1, min(n2, nblocks) + 1):
        if nblocks % k2:
            continue
        rem = nblocks//k2
        for k1 in range(1, min(n1, rem) + 1):
            if rem % k1:
                continue
            k0 = rem//k1
            if k0 > n0:
                continue
            t = [-(-n0//k0), -(-n1//k1), -(-n2//k2)]
            if (-(-n0//t[0]), -(-n1//t[1]), -(-n2//t[2])) != (k0, k1, k2):
                continue
            if max_cols is not None and t[1]*t[2] > max_cols:
                continue
            score = (k0 != 1, t[0]*t[1] + t[1]*t[2] + t[0]*t[2])      # whole lines first, then the most compact box
            if best is None or score < best[0]:
                best = (score, tuple(t))
    if best is None:
        raise NotImplementedError(
            "sub_1_pc_bjacobi_blocks = %d cannot be realised on a %dx%dx%d grid with bjacobi tiles of at most %s columns "
            "(one wavefront sweeps a tile; whole-grid ILU(0) needs n1*n2 <= 64 here).  Leave the key out for the "
            "engine's default tiles, or pass ilu_tile." % (nblocks, n0, n1, n2, max_cols))
    return best[1]


def check_amg_line_options(o, nranks=1, exc=EngineError):
    """amg_line_levels (tp_options.amg_line_levels) against the options it excludes: refused naming both, never ignored."""
    L = _opt(o, "amg_line_levels")
    if isinstance(L, bool) or int(L) != L or L < 0:
        raise ValueError("amg_line_levels = %r: an integer >= 0" % (L,))
    if L == 0:
        return
    if L > int(o["amg_full_levels"]):
        raise ValueError("amg_line_levels = %d exceeds amg_full_levels = %d: line levels are V(nu,nu) levels, never pure-transfer "
                         "or paired ones" % (L, o["amg_full_levels"]))
    if o.get("amg_single"):
        raise exc("amg_line_levels with amg_single: the line factors are kept in fp64")
    if o.get("pc") == "cptramg":
        raise exc("amg_line_levels with pc cptramg (pc_kind 3): line relaxation is implemented for the scalar hierarchies")
    if o.get("schur_selfp"):
        raise exc("amg_line_levels with schur_selfp (schur_a11 = 2): not implemented")
    if int(nranks) > 1:
        raise exc("amg_line_levels with nranks = %d: line relaxation is implemented for one slab" % int(nranks))


def check_amg_gs_options(o, nranks=1, exc=EngineError):
    """amg_gs_levels / amg_gs_sweeps (tp_options) against their ranges and the options they exclude: refused naming both, never
    ignored."""
    L, g = _opt(o, "amg_gs_levels"), _opt(o, "amg_gs_sweeps")
    if isinstance(L, bool) or int(L) != L or L < 0:
        raise ValueError("amg_gs_levels = %r: an integer >= 0" % (L,))
    if isinstance(g, bool) or int(g) != g or not 1 <= g <= 4:
        raise ValueError("amg_gs_sweeps = %r: an integer in 1..4" % (g,))
    if L == 0:
        if g != 1:
            raise ValueError("amg_gs_sweeps = %d with amg_gs_levels = 0: the sweep count would be ignored" % g)
        return
    if L > int(o["amg_full_levels"]):
        raise ValueError("amg_gs_levels = %d exceeds amg_full_levels = %d: Gauss-Seidel levels are V(g,g) levels, never "
                         "pure-transfer or paired ones" % (L, o["amg_full_levels"]))
    if _opt(o, "amg_line_levels"):
        raise exc("amg_gs_levels with amg_line_levels: one smoother per level, choose one")
    if o.get("amg_single"):
        raise exc("amg_gs_levels with amg_single: the red-black sweeps are implemented for fp64 operators")
    if o.get("pc") == "cptramg":
        raise exc("amg_gs_levels with pc cptramg (pc_kind 3): red-black Gauss-Seidel is implemented for the scalar hierarchies")
    if o.get("schur_selfp"):
        raise exc("amg_gs_levels with schur_selfp (schur_a11 = 2): not implemented")
    if int(nranks) > 1:
        raise exc("amg_gs_levels with nranks = %d: red-black Gauss-Seidel is implemented for one slab" % int(nranks))


def check_ksp_basis_options(o):
    """ksp_basis_single / ksp_single_floor (tp_options) against the range of theta and the method that has no basis."""
    th = _opt(o, "ksp_single_floor")
    # (checked whether or not ksp_basis_single is on: a value that could never be used is a mistake in the options either way;
    # the library itself, which C callers may hand a zeroed field, checks it only with the option on)
    if isinstance(th, (bool, np.bool_)) or not isinstance(th, (int, float, np.integer, np.floating)) or not 2.0**-24 < float(th) < 1.0:
        raise ValueError("ksp_single_floor = %r: a number in (2^-24, 1)" % (th,))
    if o.get("ksp_basis_single") and _opt(o, "ksp") == "bcgs":
        raise NotImplementedError("ksp_basis_single with ksp = 'bcgs' (ksp_type fbcgs): BiCGStab keeps no Krylov basis to store "
                                  "in fp32; ksp_basis_single is an option of the restarted FGMRES")


_REORTH = {"never": 0, "ifneeded": 1, "always": 2}
_PC_ORDER = {"SI": 0, "IS": 1, "ISI": 2, "SIS": 3}


def check_pc_order_options(o):
    """pc_order (tp_options) against its values and the preconditioners that have only one of the two stages: refused naming
    both, never ignored."""
    order = _opt(o, "pc_order")
    if not isinstance(order, str) or order not in _PC_ORDER:
        raise ValueError("pc_order = %r: 'SI', 'IS', 'ISI' or 'SIS'" % (order,))
    if order == "SI":
        return
    if o.get("pc") == "fieldsplit_cd":
        raise NotImplementedError("pc_order = %r with pc = 'fieldsplit_cd' (pc_kind 2): that preconditioner has no second stage "
                                  "to order" % (order,))
    if o.get("pc") == "bilu":
        raise NotImplementedError("pc_order = %r with pc = 'bilu' (pc_kind 4): that preconditioner has no first stage to order"
                                  % (order,))


def check_pc_ctr_options(o, nranks=1):
    """pc_ctr (tp_options) against its values, the preconditioners that are no composite with a T stage behind it, and the slab
    count: refused naming both, never ignored."""
    v = _opt(o, "pc_ctr")
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("pc_ctr = %r: False or True" % (v,))
    if not v:
        return
    why = {"fieldsplit_cd": "(pc_kind 2): that preconditioner is no composite to append a stage to",
           "cptramg": "(pc_kind 3): the temperature stage is implemented behind pc cpr and cptr",
           "bilu": "(pc_kind 4): that preconditioner is no composite to append a stage to"}
    if o.get("pc") in why:
        raise NotImplementedError("pc_ctr with pc = %r %s" % (o["pc"], why[o["pc"]]))
    if int(nranks) > 1:
        raise NotImplementedError("pc_ctr with nranks = %d: the temperature stage is implemented for one slab" % int(nranks))


_SCHUR_FACT = {"full": 0, "lower": 1, "upper": 2, "diag": 3}


def check_schur_fact_options(o):
    """schur_fact / schur_scale (tp_options) against their values and the preconditioners that have no Schur factorisation on
    (p,T) to choose: refused naming both, never ignored."""
    fact = _opt(o, "schur_fact")
    if not isinstance(fact, str) or fact not in _SCHUR_FACT:
        raise ValueError("schur_fact = %r: 'full', 'lower', 'upper' or 'diag'" % (fact,))
    scale = _opt(o, "schur_scale")
    if not _is_number(scale) or not math.isfinite(float(scale)):
        raise ValueError("schur_scale = %r: a finite number" % (scale,))
    if fact != "diag" and float(scale) != DEFAULT_OPTS["schur_scale"]:
        raise ValueError("schur_scale = %r with schur_fact = %r: the scale belongs to schur_fact = 'diag' (it would be silently "
                         "ignored)" % (scale, fact))
    if fact == "full":
        return
    why = {"cpr": "(pc_kind 0): one V-cycle on the pressure block, no Schur split",
           "cptramg": "(pc_kind 3): one system V-cycle on the (p,T) blocks, no Schur split",
           "bilu": "(pc_kind 4): bjacobi + ILU alone, no Schur split"}
    if o.get("pc") in why:
        raise NotImplementedError("schur_fact = %r with pc = %r %s" % (fact, o["pc"], why[o["pc"]]))
    if o.get("fs_additive"):
        raise NotImplementedError("schur_fact = %r with fs_additive (pc_fieldsplit_type additive, pc_fieldsplit_diag): PETSc's "
                                  "additive split is no Schur factorisation; schur_fact = 'diag' with schur_scale is the Schur one"
                                  % (fact,))


def check_ksp_reorth_options(o):
    """ksp_reorth / ksp_reorth_eta (tp_options) against the range of eta and the configurations that have no fp64 basis."""
    eta = _opt(o, "ksp_reorth_eta")
    # (checked whether or not the refinement is on, as ksp_single_floor is)
    if not _is_number(eta) or not 0.0 < float(eta) < 1.0:
        raise ValueError("ksp_reorth_eta = %r: a number in (0, 1)" % (eta,))
    mode = _opt(o, "ksp_reorth")
    if mode not in _REORTH:
        raise ValueError("ksp_reorth = %r: 'never', 'ifneeded' or 'always'" % (mode,))
    if mode == "never":
        return
    if _opt(o, "ksp") == "bcgs":
        raise NotImplementedError("ksp_reorth = %r with ksp = 'bcgs' (ksp_type fbcgs): BiCGStab keeps no Krylov basis to "
                                  "orthogonalise against; ksp_reorth is an option of the restarted FGMRES" % (mode,))
    if o.get("ksp_basis_single"):
        raise NotImplementedError("ksp_reorth = %r with ksp_basis_single: a basis rounded to fp32 cannot be orthonormal below "
                                  "2^-24, so a second Gram-Schmidt pass buys nothing; ksp_reorth needs the fp64 bases" % (mode,))


def check_options(o, nranks=1, exc=EngineError):
    """Every check of an option against its range and against the options it excludes, in one fixed order (exc: what the AMG
    smoother checks raise for a combination that is not implemented)."""
    check_amg_line_options(o, nranks, exc)
    check_amg_gs_options(o, nranks, exc)
    check_ksp_basis_options(o)
    check_ksp_reorth_options(o)
    check_pc_order_options(o)
    check_pc_ctr_options(o, nranks)
    check_schur_fact_options(o)
    check_linesearch_options(o)
    check_ew_options(o)


def check_boundary_slabs(boundary, nranks=1):
    """Dirichlet sides (spec["boundary"], HipEngine.set_boundary) against the slab count: refused naming both."""
    if boundary and int(nranks) > 1:
        raise NotImplementedError("a boundary (sides %s) with nranks = %d: Dirichlet sides are implemented for one slab"
                                  % (sorted(boundary), int(nranks)))


def check_wells_slabs(wells, nranks=1, local_group=None, comm_bootstrap=None):
    """Completed wells (spec["wells"], HipEngine.set_wells) against the slab count: refused naming both."""
    if wells and (int(nranks) > 1 or local_group is not None or comm_bootstrap is not None):
        raise NotImplementedError("wells (%s) with nranks = %d or a communicator: completed wells are implemented for one slab"
                                  % (", ".join(str(w.get("name", i)) for i, w in enumerate(wells)), int(nranks)))


def check_wells(wells, ncells):
    """spec["wells"] as the library will check it, with the well's name in every message: a list of dicts with name, kind
    ("prod" | "inj"), rate (>= 0), bhp (the limit), cells (flat internal indices), WI (> 0), z (elevations), optional z_ref (the
    highest perforation's elevation by default) and shut.  Returns the list with arrays and defaults filled in."""
    out, seen = [], {}
    for i, w in enumerate(wells or []):
        name = str(w.get("name", "well%d" % i))
        if w.get("kind") not in WELL_KINDS:
            raise ValueError("well %r: kind = %r: 'prod' or 'inj'" % (name, w.get("kind")))
        cells = np.asarray(w["cells"], dtype=np.int64).reshape(-1)
        WI = np.asarray(w["WI"], dtype=float).reshape(-1)
        z = np.asarray(w["z"], dtype=float).reshape(-1)
        if cells.size == 0:
            raise ValueError("well %r has no perforation" % name)
        if not (cells.size == WI.size == z.size):
            raise ValueError("well %r: %d cells, %d WI, %d z: one of each per perforation" % (name, cells.size, WI.size, z.size))
        rate, bhp = float(w["rate"]), float(w["bhp"])
        z_ref = float(z.max() if w.get("z_ref") is None else w["z_ref"])
        if not (np.isfinite([rate, bhp, z_ref]).all() and np.isfinite(WI).all() and np.isfinite(z).all()):
            raise ValueError("well %r: rate, bhp, z_ref, WI and z must be finite numbers" % name)
        if rate < 0.0:
            raise ValueError("well %r: rate = %r: the total rate target, >= 0" % (name, rate))
        if not (WI > 0.0).all():
            raise ValueError("well %r: WI = %r at perforation %d: the connection index, > 0" % (name, float(WI[WI <= 0.0][0]), int(np.argmax(WI <= 0.0))))
        if cells.min() < 0 or cells.max() >= int(ncells):
            raise ValueError("well %r: cell %d lies outside the box of %d cells" % (name, int(cells[(cells < 0) | (cells >= ncells)][0]), int(ncells)))
        for c in cells.tolist():
            if c in seen:
                raise ValueError("well %r: cell %d is already perforated by well %r: a cell may carry one perforation" % (name, c, seen[c]))
            seen[c] = name
        if name in [o["name"] for o in out]:
            raise ValueError("two wells are called %r" % name)
        out.append({"name": name, "kind": "inj" if WELL_KINDS[w["kind"]] else "prod", "rate": rate, "bhp": bhp, "z_ref": z_ref,
                    "shut": bool(w.get("shut", False)), "cells": cells, "WI": WI, "z": z})
    return out


def check_spacing_slabs(hs, nranks=1, local_group=None, comm_bootstrap=None):
    """Graded widths (spec["hs"]) against slabs: refused, naming both, before any context exists."""
    if hs is None:
        return
    if int(nranks) > 1 or local_group is not None or comm_bootstrap is not None:
        raise NotImplementedError("a graded grid (spec[\"hs\"], geo.set_spacing) with nranks = %d%s: per-axis cell widths are "
                                  "implemented for one slab without a communicator"
                                  % (int(nranks), " and a slab group" if local_group is not None else ""))


def check_spacing(hs, n):
    """spec["hs"] against the grid n = (n0, n1, n2): three arrays of positive finite widths in internal axis order."""
    if len(hs) != 3:
        raise ValueError("spec[\"hs\"] holds %d arrays: one per internal axis, three" % len(hs))
    out = []
    for a in range(3):
        w = np.ascontiguousarray(hs[a], dtype=float).reshape(-1)
        if w.size != int(n[a]):
            raise ValueError("spec[\"hs\"][%d] has %d widths but the grid has %d cells along internal axis %d" % (a, w.size, n[a], a))
        if not np.isfinite(w).all() or (w <= 0.0).any():
            raise ValueError("spec[\"hs\"][%d]: the widths must be positive and finite" % a)
        out.append(w)
    return tuple(out)


_CAPILLARY = {None: 0, "linear": 1, "brooks_corey": 2}


def pack_satfn(sat):
    """A saturation-function setting (physicalparameters.check_satfn's dict) as the library's struct.  The library knows the
    linear curves (relperm 0) and Corey's (1): "brooks_corey" goes in as Corey with n_o = n_w = (2 + 3 lmbda)/lmbda."""
    d = check_satfn(sat)
    n_o, n_w = d["n_o"], d["n_w"]
    if d["relperm"] == "brooks_corey":
        n_o = n_w = (2.0 + 3.0*d["lmbda"])/d["lmbda"]
    return tp_satfn(relperm=0 if d["relperm"] == "linear" else 1, capillary=_CAPILLARY[d["capillary"]], Sr_o=d["Sr_o"],
                    Sr_w=d["Sr_w"], n_o=n_o, n_w=n_w, kro_max=d["kro_max"], krw_max=d["krw_max"], lmbda=d["lmbda"],
                    p_ct=d["p_ct"], pc_se_min=d["pc_se_min"])


_PC = {"cpr": 0, "cptr": 1, "fieldsplit_cd": 2, "cptramg": 3, "bilu": 4}
_DECOUP = {"No": 0, "QI": 1, "TI": 2, "QI_temp": 3, "TI_temp": 4}
_S1_KSP = {"preonly": 0, "richardson": 1, "fgmres": 2}
_KSP = {"fgmres": 0, "bcgs": 1}


def load_library(path=None):
    """dlopen the in-tree HIP library; fail loudly if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or _LIBPATH
    if not os.path.exists(p):
        raise EngineError("libthermalporous_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    lib = C.CDLL(p)
    lib.tp_last_error.restype = C.c_char_p
    for name in API_SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        if name != "tp_last_error":
            fn.restype = C.c_int
    if path is None:
        _LIB = lib
    return lib


# TP_* environment variables read in Python, not by the library: no entries of switch_table()
PYTHON_SIDE_SWITCHES = {
    "TP_LOCAL_DEVICE": "pin every rank to one GPU index (engine.py, parallel.py)",
    "TP_CPU_THREADS": "OpenMP threads of oracle/cport (tests, bench.py's CPU leg)",
}


def switch_table():
    """The library's TP_* runtime switches (csrc/tp_switches.hpp) as a list of dicts with the keys name, kind
    ("flag" | "int" | "real"), default, when ("process" | "setup") and effect.  Needs no GPU."""
    lib = load_library()
    out = []
    for i in range(lib.tp_switch_count()):
        f = [C.c_char_p() for _ in range(5)]
        if lib.tp_switch_entry(i, *[C.byref(x) for x in f]) != 0:
            raise EngineError(lib.tp_last_error().decode())
        out.append(dict(zip(("name", "kind", "default", "when", "effect"), (x.value.decode() for x in f))))
    return out


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def slab_range(gn2, rank, nranks):
    """Planes [lo, hi) of internal axis 2 owned by `rank` (as even as possible, low ranks get the extras)."""
    base, rem = divmod(gn2, nranks)
    lo = rank*base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class HipEngine:
    """Same interface as oracle.engine.OracleEngine; all arithmetic on the GPU."""
    supports_satfn = True          # spec["satfn"] is honoured (thermalmodel.init_solver refuses engines that do not say so)
    supports_wells = True          # spec["wells"] likewise

    def __init__(self, spec, opts=None, rank=0, nranks=1, device=None, comm_bootstrap=None, local_group=None):
        check_boundary_slabs(spec.get("boundary"), nranks)       # (host-side: before the library and any context)
        check_spacing_slabs(spec.get("hs"), nranks, local_group, comm_bootstrap)
        check_wells_slabs(spec.get("wells"), nranks, local_group, comm_bootstrap)
        self.lib = load_library()
        self.spec = spec
        self.opts = dict(DEFAULT_OPTS)
        self.opts.update(opts or {})
        self.opts = resolve_ilu_options(self.opts, spec["n"], nranks)
        check_options(self.opts, nranks)
        self.nph = int(spec["nphase"])
        self.b = self.nph + 1
        n0, n1, gn2 = (int(v) for v in spec["n"])
        self.rank, self.nranks = int(rank), int(nranks)
        if self.nranks > 1 and gn2 < self.nranks:
            raise EngineError("more slabs than planes along the slab axis")
        self.lo, self.hi = slab_range(gn2, self.rank, self.nranks)
        self.n = (n0, n1, self.hi - self.lo)
        self.gn = (n0, n1, gn2)
        self.np_ = n0*n1
        self.ntot = self.np_*(self.n[2] + 2)
        g = tp_grid(n0, n1, self.n[2], gn2, self.lo, (C.c_double*3)(*[float(h) for h in spec["h"]]),
                    int(spec["gaxis"]), self.nph, self.rank, self.nranks)
        prm = tp_params(*[float(spec["prm"][k]) for k in tp_params._names])
        self._opt = self._make_options(self.opts)
        self.ctx = C.c_void_p()
        if device is None:
            device = int(os.environ.get("TP_LOCAL_DEVICE", os.environ.get("LOCAL_RANK", "0"))) if (self.nranks > 1 and local_group is None) else 0
        self._ck(self.lib.tp_create(C.byref(g), C.byref(prm), C.byref(self._opt), int(device), C.byref(self.ctx)))
        if self.nranks > 1 and local_group is not None:
            # N engines in N threads of this process sharing one GPU (validation of the slab algorithm)
            self._ck(self.lib.tp_comm_init_local(self.ctx, local_group))
        elif self.nranks > 1 or comm_bootstrap is not None:
            # (nranks == 1 with an explicit bootstrap: a one-rank RCCL communicator, used by the tests to run the
            # library's RCCL calls for real on a one-GPU box)
            if comm_bootstrap is None:
                raise EngineError("multi-slab engine needs comm_bootstrap(make_id) -> 128-byte id")
            ident = comm_bootstrap(self._unique_id)
            self._ck(self.lib.tp_comm_init(self.ctx, C.c_char_p(bytes(ident))))
        # graded grid (spacing.py; include/thermalporous_hip.h: tp_set_spacing): the widths go in before the fields are
        # finalised, so that the transmissibilities are formed once, from them
        self.spacing = None                    # the widths per internal axis in force, or None on a uniform grid
        if spec.get("hs") is not None:
            self.set_spacing(spec["hs"], finalize=False)
        # fields (slab + halo planes; halo of a physical boundary replicates the boundary plane)
        for name, arr in (("phi", spec["phi"]), ("kT", spec["kT"]), ("K0", spec["K"][0]), ("K1", spec["K"][1]),
                          ("K2", spec["K"][2])):
            a = self._with_halo(np.asarray(arr, dtype=float))
            self._ck(self.lib.tp_set_field(self.ctx, name.encode(), _dptr(a), C.c_int64(a.size)))
        self._ck(self.lib.tp_finalize_fields(self.ctx))
        # saturation functions (physicalparameters.py; include/thermalporous_hip.h: tp_set_saturation_functions): pointwise in
        # the closures, so every slab's context takes the same setting
        self.satfn = None                      # the setting in force (check_satfn's dict), or None for the linear / no-p_c default
        if spec.get("satfn") is not None:
            self.set_saturation_functions(spec["satfn"])
        self._set_sources(spec.get("sources"))
        self.wells = []                        # completed wells in force (check_wells' dicts; spec["wells"] layout)
        if spec.get("wells"):
            self.set_wells(spec["wells"])
        self.boundary = {}                   # side id -> the entry in force (spec["boundary"] layout)
        for side, e in sorted((spec.get("boundary") or {}).items()):
            self.set_boundary(side, e["kind"], p=e["p"], T=e["T"], S=e.get("S"))
        self.last = {}
        self._vec_ids = {}
        self._fbatch_ids = {}

    # ---- plumbing ---------------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise EngineError(self.lib.tp_last_error().decode())

    def _unique_id(self):
        buf = C.create_string_buffer(128)
        self._ck(self.lib.tp_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def _make_options(o):
        """The options as the library's struct: every field by name, a key the dict does not carry at its default."""
        # (but amg_dom_tau: a dict without the key packs 0, no truncation, not the engine's default of 0.25)
        o = {**DEFAULT_OPTS, "amg_dom_tau": 0.0, **o}
        t = o["ilu_tile"]
        return tp_options(
            pc_kind=_PC[o["pc"]], decoup=_DECOUP[o["decoup"]], ksp_rtol=o["ksp_rtol"], ksp_atol=o["ksp_atol"],
            ksp_max_it=o["ksp_max_it"], ksp_restart=o["ksp_restart"], snes_rtol=o["snes_rtol"], snes_atol=o["snes_atol"],
            snes_stol=o["snes_stol"], snes_max_it=o["snes_max_it"], amg_omega=o["amg_omega"], amg_nu=o["amg_nu"],
            amg_min_cells=o["amg_min_cells"], ilu_t1=int(min(t[1], 64)), ilu_t2=int(min(t[2], 64)),
            ilu_t0=0 if t[0] >= (1 << 30) else int(t[0]), amg_full_levels=int(o["amg_full_levels"]),
            amg_coarse_pre=int(o["amg_coarse_pre"]), amg_coarse_post=int(o["amg_coarse_post"]),
            amg_mid_skip=int(bool(o["amg_mid_skip"])), amg_tail_post=int(o["amg_tail_post"]), amg_single=int(bool(o["amg_single"])),
            schur_a11=2 if o["schur_selfp"] else int(bool(o["schur_a11"])), amg_gather_cells=int(o["amg_gather_cells"]),
            schur_fact=_SCHUR_FACT[o["schur_fact"]], schur_scale=float(o["schur_scale"]), amg_dom_tau=float(o["amg_dom_tau"]),
            ilu_levels=int(o["ilu_levels"]), pc_ctr=int(bool(o["pc_ctr"])), fs_additive=int(bool(o["fs_additive"])),
            pc_order=_PC_ORDER[o["pc_order"]], ksp_reorth=_REORTH[o["ksp_reorth"]], ksp_reorth_eta=float(o["ksp_reorth_eta"]),
            ksp_ew=ew_version(o["ksp_ew"]), **{k: float(o[k]) for k in _EW_KEYS}, ilu_whole=int(bool(o["ilu_whole"])),
            amg_gs_levels=int(o["amg_gs_levels"]), amg_gs_sweeps=int(o["amg_gs_sweeps"]),
            ilu_block=(C.c_int32*3)(*[int(min(int(v), 1 << 30)) for v in (o["ilu_block"] or (0, 0, 0))]),
            ilu_single=int(bool(o["ilu_single"])), ls_kind=_LS[o["linesearch"]], ls_order=int(o["ls_order"]),
            ls_max_it=int(o["ls_max_it"]), ls_alpha=float(o["ls_alpha"]), ls_maxstep=float(o["ls_maxstep"]),
            ls_minlambda=float(o["ls_minlambda"]),
            ls_max_change=(C.c_double*3)(*[float(v) for v in (o["ls_max_change"] or (0.0, 0.0, 0.0))]),
            amg_line_levels=int(o["amg_line_levels"]), ksp_basis_single=int(bool(o["ksp_basis_single"])),
            ksp_single_floor=float(o["ksp_single_floor"]), ksp_kind=HipEngine._ksp_kind(o), s1_ksp=_S1_KSP[o["s1_ksp"]],
            s1_max_it=int(o["s1_max_it"]), s1_rtol=float(o["s1_rtol"]), s1_atol=float(o["s1_atol"]))

    @staticmethod
    def _ksp_kind(o):
        k = _opt(o, "ksp")
        if k not in _KSP:
            raise ValueError("ksp = %r: 'fgmres' or 'bcgs'" % (k,))
        return _KSP[k]

    def set_options(self, **kw):
        check_options({**self.opts, **kw}, self.nranks)
        self.opts.update(kw)
        self._opt = self._make_options(self.opts)
        self._ck(self.lib.tp_set_options(self.ctx, C.byref(self._opt)))

    def _with_halo(self, a):
        """Global internal array (gn2, n1, n0) -> this slab with halo planes, flat, C-contiguous."""
        a = a.reshape(self.gn[2], self.gn[1], self.gn[0])
        lo, hi = self.lo, self.hi
        idx = np.clip(np.arange(lo - 1, hi + 1), 0, self.gn[2] - 1)
        return np.ascontiguousarray(a[idx]).reshape(-1)

    def _fields_with_halo(self, u):
        u = np.asarray(u, dtype=float).reshape(self.b, self.gn[2], self.gn[1], self.gn[0])
        return np.ascontiguousarray(np.stack([self._with_halo(u[f]) for f in range(self.b)])).reshape(-1)

    def _strip_halo(self, flat, nf):
        a = np.asarray(flat).reshape(nf, self.n[2] + 2, self.n[1], self.n[0])
        return a[:, 1:-1]

    def _set_sources(self, src):
        if not src or len(src["cell"]) == 0:
            self._ck(self.lib.tp_set_sources(self.ctx, 0, None))
            self.src_index = np.zeros(0, dtype=int)
            return
        cells = np.asarray(src["cell"], dtype=np.int64)
        plane = cells // self.np_
        mine = np.nonzero((plane >= self.lo) & (plane < self.hi))[0]
        self.src_index = mine                      # positions (in the global entry list) of my entries
        arr = (tp_source*max(1, len(mine)))()
        for k, i in enumerate(mine):
            local = int(cells[i] - self.lo*self.np_ + self.np_)
            arr[k] = tp_source(local, int(src["kind"][i]), int(src["const"][i]), float(src["wt"][i]),
                               float(src["bhp"][i]), float(src["max_rate"][i]), float(src["WI"][i]))
        self._ck(self.lib.tp_set_sources(self.ctx, len(mine), arr))
        # the library sorts entries by cell (stable): reproduce the permutation for rate read-back
        self._src_order = np.argsort(cells[mine], kind="stable")

    # ---- graded grid (spacing.py; include/thermalporous_hip.h: tp_set_spacing) --------------------------
    def set_spacing(self, hs, finalize=True):
        """Cell widths per internal axis (three arrays of n0, n1, n2 positive numbers), or None for the uniform grid of
        spec["h"].  The library recomputes the interior and boundary transmissibilities at tp_finalize_fields, which this
        call issues unless `finalize` is False."""
        check_spacing_slabs(hs, self.nranks)
        if hs is None:
            self._ck(self.lib.tp_set_spacing(self.ctx, None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0)))
            self.spacing = None
        else:
            w = check_spacing(hs, self.gn)
            self._ck(self.lib.tp_set_spacing(self.ctx, _dptr(w[0]), C.c_int64(w[0].size), _dptr(w[1]), C.c_int64(w[1].size),
                                             _dptr(w[2]), C.c_int64(w[2].size)))
            self.spacing = w
        if finalize:
            self._ck(self.lib.tp_finalize_fields(self.ctx))

    def spacing_info(self):
        """tp_spacing_info: dict(graded, hmin, hmax) with the smallest and largest width per internal axis."""
        graded = C.c_int32(0)
        lo, hi = np.zeros(3), np.zeros(3)
        self._ck(self.lib.tp_spacing_info(self.ctx, C.byref(graded), _dptr(lo), _dptr(hi)))
        return dict(graded=bool(graded.value), hmin=tuple(lo), hmax=tuple(hi))

    # ---- saturation functions (physicalparameters.py; include/thermalporous_hip.h: tp_set_saturation_functions) ----
    def set_saturation_functions(self, sat):
        """Relative permeabilities and capillary pressure of the two-phase model: a dict with the keys of
        PhysicalParameters.satfn_dict() (missing keys at their defaults), or None for the linear curves without capillary
        pressure.  Any time between two solves; the library recomputes the old state's accumulation."""
        if sat is None:
            self._ck(self.lib.tp_set_saturation_functions(self.ctx, None))
            self.satfn = None
            return
        d = check_satfn(sat)
        if self.nph != 2 and not satfn_is_default(d):
            raise NotImplementedError("relperm = %r, capillary = %r on a single-phase engine: saturation functions need a "
                                      "saturation, which only the two-phase model has" % (d["relperm"], d["capillary"]))
        st = pack_satfn(d)
        self._ck(self.lib.tp_set_saturation_functions(self.ctx, C.byref(st)))
        self.satfn = None if satfn_is_default(d) else d

    def saturation_info(self):
        """tp_saturation_info: dict(active, relperm ("linear" | "corey"), capillary, and the numbers as the library holds them:
        a "brooks_corey" relperm reads back as "corey" with its exponents)."""
        st, active = tp_satfn(), C.c_int32(0)
        self._ck(self.lib.tp_saturation_info(self.ctx, C.byref(st), C.byref(active)))
        out = {k: float(getattr(st, k)) for k in SATFN_NUMBERS}
        out.update(active=bool(active.value), relperm=("linear", "corey")[st.relperm],
                   capillary={v: k for k, v in _CAPILLARY.items()}[st.capillary])
        return out

    # ---- Dirichlet sides (boundary.py; include/thermalporous_hip.h: tp_set_boundary) -------------------
    def _side_shape(self, side):
        a = int(side)//2
        lo, hi = [k for k in range(3) if k != a]
        return (self.n[hi], self.n[lo])

    def set_boundary(self, side, kind, p=None, T=None, S=None):
        """Set, replace or (kind "none") remove the Dirichlet state of internal side 2*a + d, any time between two solves.
        kind: "open" | "thermal" | "none"; p, T, S: the ghost state in internal layout, scalars or arrays of shape (n_hi, n_lo)
        over the other two internal axes (the entries of spec["boundary"]).  T is required; p defaults to p_ref and is
        replaced by it for "thermal" (no flow: it cannot matter); S (two-phase) is required for "open" and defaults to S_o
        for "thermal"."""
        check_boundary_slabs({side: kind}, self.nranks)
        if isinstance(side, (bool, np.bool_)) or int(side) != side or not 0 <= int(side) <= 5:
            raise ValueError("boundary side %r: the internal side id 2*a + d in 0..5" % (side,))
        side = int(side)
        if kind not in KINDS:
            raise ValueError("boundary kind %r: 'open', 'thermal' or 'none'" % (kind,))
        if kind == "none":
            self._ck(self.lib.tp_set_boundary(self.ctx, side, 0, None, C.c_int64(0)))
            self.boundary.pop(side, None)
            return
        if T is None:
            raise ValueError("boundary side %d, kind %r: the ghost temperature T is required" % (side, kind))
        shape, prm = self._side_shape(side), self.spec["prm"]
        if self.nph == 2 and S is None:
            if kind == "open":
                raise ValueError("boundary side %d: S is required for a two-phase open boundary" % side)
            S = prm["S_o"]
        if p is None or kind == "thermal":
            p = prm["p_ref"]
        e = {"kind": kind}
        for name, v in (("p", p), ("T", T)) + ((("S", S),) if self.nph == 2 else ()):
            a = np.asarray(v, dtype=float)
            if a.ndim and a.size != shape[0]*shape[1]:
                raise ValueError("%s on boundary side %d has %d entries: a scalar or %d faces (shape %r)"
                                 % (name, side, a.size, shape[0]*shape[1], shape))
            e[name] = np.broadcast_to(a, shape).copy() if a.ndim == 0 else a.reshape(shape).copy()
        e.setdefault("S", None)
        vals = pack_values(e, self.nph)
        self._ck(self.lib.tp_set_boundary(self.ctx, side, KINDS[kind], _dptr(vals), C.c_int64(shape[0]*shape[1])))
        self.boundary[side] = e

    def boundary_flux(self):
        """(6, b): per internal side and equation, the sum of what the side's faces added to the residual at the last assembly
        (tp_boundary_flux): the residual's sign -- positive leaves the domain -- and the equation's own scaling; zero rows
        for the sides that are not set."""
        out = np.zeros((6, self.b))
        self._ck(self.lib.tp_boundary_flux(self.ctx, _dptr(out)))
        return out

    # ---- engine interface ---------------------------------------------------------------------------
    def set_state(self, u):
        a = self._fields_with_halo(u)
        self._ck(self.lib.tp_set_state(self.ctx, _dptr(a)))

    def get_state(self):
        """This rank's owned part of the state, shape (b, n2_local, n1, n0)."""
        out = np.empty(self.b*self.ntot)
        self._ck(self.lib.tp_get_state(self.ctx, _dptr(out)))
        return self._strip_halo(out, self.b).copy()

    def set_old(self, u=None):
        if u is None:
            self._ck(self.lib.tp_set_old_state(self.ctx, None))
        else:
            a = self._fields_with_halo(u)
            self._ck(self.lib.tp_set_old_state(self.ctx, _dptr(a)))

    def set_dt(self, dt):
        self._ck(self.lib.tp_set_dt(self.ctx, C.c_double(float(dt))))

    def get_old_state(self):
        out = np.empty(self.b*self.ntot)
        self._ck(self.lib.tp_get_old_state(self.ctx, _dptr(out)))
        return self._strip_halo(out, self.b).copy()

    def restore_state(self):
        self._ck(self.lib.tp_restore_state(self.ctx))

    def saturation_range(self):
        lo, hi = C.c_double(), C.c_double()
        self._ck(self.lib.tp_saturation_range(self.ctx, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def clamp_saturation(self):
        self._ck(self.lib.tp_clamp_saturation(self.ctx))

    def residual(self, u=None):
        if u is not None:
            self.set_state(u)
        nrm = C.c_double()
        self._ck(self.lib.tp_residual(self.ctx, C.byref(nrm)))
        out = np.empty(self.b*self.ntot)
        self._ck(self.lib.tp_get_residual(self.ctx, _dptr(out)))
        self.last_fnorm = nrm.value
        return self._strip_halo(out, self.b).copy()

    def jacobian(self, u=None, want_schur=False):
        if u is not None:
            self.set_state(u)
        if want_schur and self.opts["pc"] not in ("cptr", "fieldsplit_cd"):
            raise EngineError("S~ is assembled only for pc='cptr' / 'fieldsplit_cd'")
        self._ck(self.lib.tp_jacobian(self.ctx))
        b = self.b
        out = np.empty(7*b*b*self.ntot)
        self._ck(self.lib.tp_export_jacobian(self.ctx, _dptr(out)))
        J = self._strip_halo(out, 7*b*b).reshape(7, b, b, self.n[2], self.n[1], self.n[0]).copy()
        if want_schur:
            s = np.empty(7*self.ntot)
            self._ck(self.lib.tp_export_schur(self.ctx, _dptr(s)))
            return J, self._strip_halo(s, 7).copy()
        return J

    def well_rates(self):
        n = len(self.src_index)
        if n == 0:
            return {}
        r, w, o = (np.zeros(n) for _ in range(3))
        self._ck(self.lib.tp_well_rates(self.ctx, _dptr(r), _dptr(w), _dptr(o)))
        inv = np.empty(n, dtype=int)
        inv[self._src_order] = np.arange(n)
        return {"rate": r[inv], "water_rate": w[inv], "oil_rate": o[inv]}

    # ---- completed wells (completedwells.py; include/thermalporous_hip.h: tp_set_wells) ----------------
    def set_wells(self, wells):
        """The completed wells (spec["wells"]: check_wells' list of dicts), or None / [] to remove them."""
        check_wells_slabs(wells, self.nranks)
        ws = check_wells(wells, self.gn[0]*self.gn[1]*self.gn[2])
        if not ws:
            self._ck(self.lib.tp_set_wells(self.ctx, 0, None, 0, None))
            self.wells = []
            return
        nperf = sum(w["cells"].size for w in ws)
        warr, parr = (tp_well*len(ws))(), (tp_perf*nperf)()
        k = 0
        for i, w in enumerate(ws):
            warr[i] = tp_well(WELL_KINDS[w["kind"]], int(w["shut"]), w["rate"], w["bhp"], w["z_ref"], k, w["cells"].size)
            for c, wi, z in zip(w["cells"], w["WI"], w["z"]):
                parr[k] = tp_perf(int(c) + self.np_, float(wi), float(z))       # (one slab: local = global + the halo plane)
                k += 1
        self._ck(self.lib.tp_set_wells(self.ctx, len(ws), warr, nperf, parr))
        self.wells = ws

    def _well_index(self, well):
        if isinstance(well, str):
            names = [w["name"] for w in self.wells]
            if well not in names:
                raise KeyError("no well called %r (wells: %s)" % (well, ", ".join(names) or "none"))
            return names.index(well)
        return int(well)

    def set_well_control(self, well, rate=None, bhp=None, shut=None):
        """New targets of one well (by name or index) between two time steps; None keeps what is in force."""
        i = self._well_index(well)
        if not 0 <= i < len(self.wells):
            raise IndexError("well %r: the engine has %d wells" % (well, len(self.wells)))
        w = self.wells[i]
        rate = w["rate"] if rate is None else float(rate)
        bhp = w["bhp"] if bhp is None else float(bhp)
        shut = w["shut"] if shut is None else bool(shut)
        self._ck(self.lib.tp_set_well_control(self.ctx, i, C.c_double(rate), C.c_double(bhp), int(shut)))
        w.update(rate=rate, bhp=bhp, shut=shut)

    def well_info(self):
        """Per well, from the last assembly: name, kind, bhp, mode ("shut" | "rate" | "bhp"), rate, water_rate, oil_rate (sums
        over the perforations; production negative), rho (the head density), rounds (active-set rounds), nopen."""
        n = len(self.wells)
        if n == 0:
            return []
        st = (tp_well_state*n)()
        self._ck(self.lib.tp_well_info(self.ctx, st))
        return [{"name": w["name"], "kind": w["kind"], "bhp": s.bhp, "mode": WELL_MODES[s.mode], "rate": s.rate,
                 "water_rate": s.water_rate, "oil_rate": s.oil_rate, "rho": s.rho, "rounds": s.rounds, "nopen": s.nopen}
                for w, s in zip(self.wells, st)]

    def _perf_split(self, a):
        out, k = [], 0
        for w in self.wells:
            out.append(a[..., k:k + w["cells"].size].copy())
            k += w["cells"].size
        return out

    def well_perf_rates(self):
        """Per well a dict of arrays over its perforations: rate, water_rate, oil_rate of the last assembly."""
        n = sum(w["cells"].size for w in self.wells)
        if n == 0:
            return []
        r, wt, o = (np.zeros(n) for _ in range(3))
        self._ck(self.lib.tp_well_perf_rates(self.ctx, _dptr(r), _dptr(wt), _dptr(o)))
        return [{"rate": a, "water_rate": b, "oil_rate": c}
                for a, b, c in zip(self._perf_split(r), self._perf_split(wt), self._perf_split(o))]

    def well_factors(self):
        """Per well (c, b), arrays (b, perforations): the rank-1 term c b^T of the last Jacobian assembly (zeros in BHP mode)."""
        n = sum(w["cells"].size for w in self.wells)
        if n == 0:
            return []
        c, b = np.zeros((self.b, n)), np.zeros((self.b, n))
        self._ck(self.lib.tp_well_factors(self.ctx, _dptr(c), _dptr(b)))
        return list(zip(self._perf_split(c), self._perf_split(b)))

    # device vectors for the PC plug-in API / tests
    def vec(self, name):
        if name not in self._vec_ids:
            i = C.c_int32()
            self._ck(self.lib.tp_vec_create(self.ctx, C.byref(i)))
            self._vec_ids[name] = i.value
        return self._vec_ids[name]

    def vec_set(self, name, x):
        a = self._fields_with_halo(x)
        self._ck(self.lib.tp_vec_set(self.ctx, self.vec(name), _dptr(a)))

    def vec_get(self, name):
        out = np.empty(self.b*self.ntot)
        self._ck(self.lib.tp_vec_get(self.ctx, self.vec(name), _dptr(out)))
        return self._strip_halo(out, self.b).copy()

    def vec_batch(self, prefix, n):
        """n vectors '<prefix>0'..'<prefix>{n-1}' in one allocation (a Krylov basis): VecMDot/VecMAXPY run in one pass."""
        if prefix + "0" not in self._vec_ids:
            i = C.c_int32()
            self._ck(self.lib.tp_vec_create_batch(self.ctx, int(n), C.byref(i)))
            for k in range(n):
                self._vec_ids[prefix + str(k)] = i.value + k
        return self._vec_ids[prefix + "0"]

    def dot_batch(self, prefix, n, w):
        out = np.zeros(n)
        self._ck(self.lib.tp_vec_dot_batch(self.ctx, self.vec_batch(prefix, n), int(n), self.vec(w), _dptr(out)))
        return out

    def axpy_batch(self, prefix, n, coef, w):
        coef = np.ascontiguousarray(coef, dtype=float)
        self._ck(self.lib.tp_vec_axpy_batch(self.ctx, self.vec_batch(prefix, n), int(n), _dptr(coef), self.vec(w)))

    def norm2(self, x):
        out = C.c_double()
        self._ck(self.lib.tp_vec_norm2(self.ctx, self.vec(x), C.byref(out)))
        return out.value

    def set_ksp_monitor(self, fn):
        """fn(its, rnorm, field_norms) at every iteration of the outer Krylov method (the reference's ksp_monitor_residuals monitor,
        thermalmodel.py:44-74); None removes it."""
        proto = C.CFUNCTYPE(None, C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_int32, C.c_void_p)
        if fn is None:
            self._monitor_cb = None
            self._ck(self.lib.tp_set_ksp_monitor(self.ctx, C.cast(None, proto), None))
            return
        self._monitor_cb = proto(lambda its, rn, fnp, nf, user: fn(int(its), float(rn), [fnp[i] for i in range(nf)]))
        self._ck(self.lib.tp_set_ksp_monitor(self.ctx, self._monitor_cb, None))

    def spmv(self, x, y):
        self._ck(self.lib.tp_spmv(self.ctx, self.vec(x), self.vec(y)))

    def pc_setup(self):
        self._ck(self.lib.tp_pc_setup(self.ctx))

    def pc_apply(self, x, y):
        self._ck(self.lib.tp_pc_apply(self.ctx, self.vec(x), self.vec(y)))

    def stage1_apply(self, x, y):
        self._ck(self.lib.tp_stage1_apply(self.ctx, self.vec(x), self.vec(y)))

    def stage_rhs(self, x, y, out):
        """out_q = [x - J y]_q - d_q [x - J y]_s on the primary fields q (tp_stage_rhs): the right-hand side of a later S stage of
        the composite (pc_order), one kernel; the other fields of `out` are not written."""
        self._ck(self.lib.tp_stage_rhs(self.ctx, self.vec(x), self.vec(y), self.vec(out)))

    def ctr_rhs(self, x, y, out):
        """Field 1 of `out` = [x - J y]_1 (tp_ctr_rhs): the right-hand side of the composite's temperature stage (pc_ctr), one
        kernel that reads only row 1 of the Jacobian; the other fields of `out` are not written."""
        self._ck(self.lib.tp_ctr_rhs(self.ctx, self.vec(x), self.vec(y), self.vec(out)))

    def ctr_apply(self, x, y):
        """y_1 = V(A_TT) x_1, every other field of y zero (tp_ctr_apply): the temperature stage of pc_ctr on its own."""
        self._ck(self.lib.tp_ctr_apply(self.ctx, self.vec(x), self.vec(y)))

    def ctr_info(self):
        """The temperature stage (tp_ctr_info): whether pc_ctr is in effect, the levels of its A_TT hierarchy, its set-ups and the
        T-stage applications launched since the engine was created."""
        out = (C.c_int32*4)()
        self._ck(self.lib.tp_ctr_info(self.ctx, out))
        return dict(enabled=bool(out[0]), levels=out[1], setups=out[2], applies=out[3])

    def schur_info(self):
        """The Schur split on (p,T) (tp_schur_info): the factorisation and scale in force and the applications of the pressure
        solver K(A00) and of the Schur solver K(S) issued or replayed since the last pc_setup."""
        fact, scale, k0, ks = C.c_int(), C.c_double(), C.c_long(), C.c_long()
        self._ck(self.lib.tp_schur_info(self.ctx, C.byref(fact), C.byref(scale), C.byref(k0), C.byref(ks)))
        return dict(fact={v: k for k, v in _SCHUR_FACT.items()}[fact.value], scale=scale.value, k0_applies=k0.value, ks_applies=ks.value)

    def ilu_factor(self):
        self._ck(self.lib.tp_ilu0_factor(self.ctx))

    def ilu_solve(self, x, y):
        self._ck(self.lib.tp_ilu0_solve(self.ctx, self.vec(x), self.vec(y)))

    def schur_apply(self, x, y):
        self._ck(self.lib.tp_schur_apply(self.ctx, self.vec(x), self.vec(y)))

    def vec_axpby(self, out, a, x, b, y):
        """out = a*x + b*y through the host (test/plug-in convenience, not on the hot path)."""
        self.vec_set(out, a*self._full(self.vec_get(x)) + b*self._full(self.vec_get(y)))

    def _full(self, owned):
        """Owned slab part -> global-shaped array (single-slab engines only)."""
        if self.nranks != 1:
            raise EngineError("host-side vector algebra is only available on single-slab engines")
        return owned

    def amg_vcycle(self, which, b, fb, x, fx):
        self._ck(self.lib.tp_amg_vcycle(self.ctx, which, fb, self.vec(b), fx, self.vec(x)))

    def fgmres(self, b, x):
        its, reason, rn = C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self.lib.tp_fgmres(self.ctx, self.vec(b), self.vec(x), C.byref(its), C.byref(reason), C.byref(rn)))
        return its.value, reason.value, rn.value

    def bcgs(self, b, x):
        """Right-preconditioned BiCGStab from x0 = 0 (tp_bcgs): (iterations, KSP reason, recurrence residual norm)."""
        its, reason, rn = C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self.lib.tp_bcgs(self.ctx, self.vec(b), self.vec(x), C.byref(its), C.byref(reason), C.byref(rn)))
        return its.value, reason.value, rn.value

    def ksp_info(self):
        """The outer Krylov method in effect and its workspace (tp_ksp_info)."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_ksp_info(self.ctx, out))
        return dict(kind=out[0], bytes=out[1], bcgs_vectors=out[2], pc_programs=out[3])

    def ksp_basis_info(self):
        """The fp32 FGMRES bases of ksp_basis_single (tp_ksp_basis_info): whether the option is in effect, the capacity of each
        basis in vectors, the stride between two stored vectors in entries, the fp64 staging vectors, and the restart cycles and
        true-residual evaluations of the last such solve."""
        out = (C.c_int64*6)()
        self._ck(self.lib.tp_ksp_basis_info(self.ctx, out))
        return dict(single=bool(out[0]), capacity=out[1], stride=out[2], staging=out[3], cycles=out[4], true_residuals=out[5])

    def ksp_reorth_info(self):
        """The Gram-Schmidt refinement of ksp_reorth (tp_ksp_reorth_info): the mode in effect, the orthogonalisation steps since
        the engine was created, and the second passes executed / enqueued but skipped by the device flag."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_ksp_reorth_info(self.ctx, out))
        return dict(mode=("never", "ifneeded", "always")[out[0]], steps=out[1], refined=out[2], skipped=out[3])

    def orth_step(self, prefix, k, w, mode="never", eta=2.0**-0.5):
        """One Gram-Schmidt step of the outer FGMRES on user vectors (tp_vec_orth_step): w is orthogonalised in place against the
        first k vectors of batch `prefix` (which must hold them already: vec_batch); returns (h[0..k), final ||w||^2, whether
        the second pass ran)."""
        if mode not in _REORTH:
            raise ValueError("mode = %r: 'never', 'ifneeded' or 'always'" % (mode,))
        if prefix + str(int(k) - 1) not in self._vec_ids:
            raise EngineError("batch %r holds fewer than %d vectors" % (prefix, k))
        h, n2, ran = np.zeros(int(k)), C.c_double(), C.c_int32()
        self._ck(self.lib.tp_vec_orth_step(self.ctx, self._vec_ids[prefix + "0"], int(k), self.vec(w), _REORTH[mode], C.c_double(float(eta)),
                                           _dptr(h), C.byref(n2), C.byref(ran)))
        return h, n2.value, bool(ran.value)

    # compact fp32 vector batches: the kernels of ksp_basis_single on their own (tp_fvec_*)
    def fvec_batch(self, name, n):
        """A batch of n compact float vectors (b * owned cells entries each, field-major, no halo planes)."""
        if name not in self._fbatch_ids:
            i = C.c_int32()
            self._ck(self.lib.tp_fvec_create_batch(self.ctx, int(n), C.byref(i)))
            self._fbatch_ids[name] = (i.value, int(n))
        if self._fbatch_ids[name][1] < n:
            raise EngineError("float batch %r holds %d vectors" % (name, self._fbatch_ids[name][1]))
        return self._fbatch_ids[name][0]

    def fvec_store(self, name, i, x):
        """Slot i <- vector x rounded to fp32; x itself becomes the widened stored value (the solver's round-and-store kernel)."""
        self._ck(self.lib.tp_fvec_store(self.ctx, self.fvec_batch(name, i + 1), int(i), self.vec(x)))

    def fvec_get(self, name, i):
        """Slot i as a float32 array of shape (b, n2_local, n1, n0)."""
        out = np.empty(self.b*self.np_*self.n[2], dtype=np.float32)
        self._ck(self.lib.tp_fvec_get(self.ctx, self.fvec_batch(name, i + 1), int(i), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out.reshape(self.b, self.n[2], self.n[1], self.n[0])

    def fdot_batch(self, name, n, w):
        out = np.zeros(n)
        self._ck(self.lib.tp_fvec_dot_batch(self.ctx, self.fvec_batch(name, n), int(n), self.vec(w), _dptr(out)))
        return out

    def faxpy_batch(self, name, n, coef, w):
        coef = np.ascontiguousarray(coef, dtype=float)
        self._ck(self.lib.tp_fvec_axpy_batch(self.ctx, self.fvec_batch(name, n), int(n), _dptr(coef), self.vec(w)))

    def copy_residual_to(self, name):
        self._ck(self.lib.tp_vec_copy_residual(self.ctx, self.vec(name)))

    def time_kernel(self, which, reps):
        ms = C.c_double()
        self._ck(self.lib.tp_time_kernel(self.ctx, which, reps, C.byref(ms)))
        return ms.value

    def amg_info(self, which=0):
        nl, oc = C.c_int32(), C.c_double()
        self._ck(self.lib.tp_amg_info(self.ctx, which, C.byref(nl), C.byref(oc)))
        return nl.value, oc.value

    def amg_trunc(self, which=0):
        """(level at which hierarchy `which` ends with relaxation only, -1 = full V-cycle; level-0 dominance ratio)."""
        lv, r0 = C.c_int32(), C.c_double()
        self._ck(self.lib.tp_amg_trunc(self.ctx, which, C.byref(lv), C.byref(r0)))
        return lv.value, r0.value

    def amg_tail_info(self, which=0):
        """The tail (levels of <= 1024 cells) of hierarchy `which`: whether the cycles apply it as one dense operator, its first
        level and that level's cells, and how many dense operators were formed / dense applications / multilevel tail
        kernels were launched or captured since the hierarchy was built."""
        out = (C.c_int64*6)()
        self._ck(self.lib.tp_amg_tail_info(self.ctx, which, out))
        return dict(dense=bool(out[0]), tail_level=out[1], n=out[2], builds=out[3], dense_applies=out[4], tail_launches=out[5])

    def amg_line_info(self, which=0):
        """Line relaxation of hierarchy `which` (tp_amg_line_info): line levels in effect, lines per workgroup and n0 of level 0,
        device bytes of the factor streams."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_amg_line_info(self.ctx, which, out))
        return dict(levels=out[0], group=out[1], n0=out[2], bytes=out[3])

    def amg_gs_info(self, which=0):
        """Red-black Gauss-Seidel of hierarchy `which` (tp_amg_gs_info): GS levels in effect, sweeps per leg, red and black cells of
        level 0 (all zero when the option is off or no level qualifies)."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_amg_gs_info(self.ctx, which, out))
        return dict(levels=out[0], sweeps=out[1], red=out[2], black=out[3])

    def amg_layout(self, which=0):
        """(number of slab-distributed top levels, coarsening axis of every level)."""
        nd, na = C.c_int32(), C.c_int32()
        axes = (C.c_int32*64)()
        self._ck(self.lib.tp_amg_layout(self.ctx, which, C.byref(nd), axes, 64, C.byref(na)))
        return nd.value, [axes[i] for i in range(min(na.value, 64))]

    def ilu_layout(self):
        """The stage-2 layout that was built (tp_ilu_layout): block extents, blocks, tiles, block-local tile-diagonals, the
        most tiles in one launch, launches per sweep direction."""
        out = (C.c_int32*8)()
        self._ck(self.lib.tp_ilu_layout(self.ctx, out))
        return dict(block=(out[0], out[1], out[2]), nblocks=out[3], ntiles=out[4], ndiag=out[5], max_tiles_per_launch=out[6],
                    launches=out[7])

    def ilu_factor_bytes(self):
        """Device bytes of the stage-2 factor streams, forward plus backward (tp_ilu_factor_bytes)."""
        out = C.c_int64()
        self._ck(self.lib.tp_ilu_factor_bytes(self.ctx, C.byref(out)))
        return out.value

    def inner_stats(self):
        """Inner solves (s1_ksp != preonly) since the last pc_setup: (applies, iterations used, ended above tolerance)."""
        a, i, u = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.tp_inner_stats(self.ctx, C.byref(a), C.byref(i), C.byref(u)))
        return a.value, i.value, u.value

    def ls_info(self):
        """The line search (tp_ls_info): kind in effect, device bytes of its workspace, residual evaluations (= trials) of the last
        Newton solve's searches and the non-finite ones among them."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_ls_info(self.ctx, out))
        return dict(kind=out[0], bytes=out[1], evaluations=out[2], nonfinite=out[3])

    def ls_history(self, cap=256):
        """Per Newton iteration of the last solve (tp_ls_history): accepted lambda, ||F|| after it, trials spent.  Empty after a
        basic solve."""
        lam, fn = np.zeros(cap), np.zeros(cap)
        tr = np.zeros(cap, dtype=np.int32)
        n = C.c_int32()
        self._ck(self.lib.tp_ls_history(self.ctx, int(cap), _dptr(lam), _dptr(fn), tr.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        k = min(n.value, cap)
        return dict(n=n.value, lam=lam[:k].copy(), fnorm=fn[:k].copy(), trials=[int(t) for t in tr[:k]])

    def ls_step_stats(self, dx):
        """(||dx||^2, [max|dx_f| per field]) of vector `dx` over owned cells of all slabs (tp_ls_step_stats)."""
        out = np.zeros(4)
        self._ck(self.lib.tp_ls_step_stats(self.ctx, self.vec(dx), _dptr(out)))
        return out[0], out[1:1 + self.b].copy()

    def ls_trial(self, u0, dx, lam, out):
        """out = u0 - lam*dx on owned cells (tp_ls_trial); the halo planes of `out` are not written."""
        self._ck(self.lib.tp_ls_trial(self.ctx, self.vec(u0), self.vec(dx), C.c_double(float(lam)), self.vec(out)))

    def ew_info(self):
        """Eisenstat-Walker (tp_ew_info): the version in effect (0: off), Newton solves run under it since the engine was created,
        linear solves among them, and those whose tolerance the safeguard raised."""
        out = (C.c_int64*4)()
        self._ck(self.lib.tp_ew_info(self.ctx, out))
        return dict(version=out[0], newton_solves=out[1], linear_solves=out[2], safeguarded=out[3])

    def ew_history(self, cap=256):
        """Per linear solve of the last Newton solve (tp_ew_history): its tolerance eta, ||F|| where the system was formed, the
        residual norm the Krylov solver returned, its iterations and KSP reason.  Empty after a solve with ksp_ew off."""
        eta, fn, rho = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        kits, kre = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        n = C.c_int32()
        ip = C.POINTER(C.c_int32)
        self._ck(self.lib.tp_ew_history(self.ctx, int(cap), _dptr(eta), _dptr(fn), _dptr(rho), kits.ctypes.data_as(ip),
                                        kre.ctypes.data_as(ip), C.byref(n)))
        k = min(n.value, cap)
        return dict(n=n.value, rtol=eta[:k].copy(), fnorm=fn[:k].copy(), lresid=rho[:k].copy(), kits=[int(v) for v in kits[:k]],
                    kreason=[int(v) for v in kre[:k]])

    @staticmethod
    def ew_next_rtol(opts, k, fnorm, fnorm_last=0.0, lresid_last=0.0, rtol_last=0.0):
        """The Eisenstat-Walker chooser on its own (tp_ew_next_rtol): the tolerance of linear solve k from engine options `opts`
        (ksp_ew, the ew_* keys, ksp_rtol; anything missing at its default) and the norms.  No engine and no GPU needed."""
        o = {**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8), **opts}
        check_ew_options(o)
        t = HipEngine._make_options(o)
        out = C.c_double()
        lib = load_library()
        if lib.tp_ew_next_rtol(C.byref(t), C.c_int32(int(k)), C.c_double(float(fnorm)), C.c_double(float(fnorm_last)),
                               C.c_double(float(lresid_last)), C.c_double(float(rtol_last)), C.byref(out)) != 0:
            raise EngineError(lib.tp_last_error().decode())
        return out.value

    def newton_solve(self):
        info = tp_solve_info()
        self._ck(self.lib.tp_newton_solve(self.ctx, C.byref(info)))
        self.last = dict(nits=info.nits, lits=info.lits, reason=info.reason, fnorm=info.fnorm, fnorm0=info.fnorm0,
                         ksp_reason=info.last_ksp_reason, vcycles=info.vcycles, ls_trials=self.ls_info()["evaluations"])
        if self.opts.get("ksp_ew"):
            self.last["ew_rtol"] = [float(v) for v in self.ew_history()["rtol"]]
        return self.last

    def close(self):
        if self.ctx:
            self.lib.tp_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
