/* thermalporous_hip.h -- C ABI of the MI355X hot path (libthermalporous_hip.so).
 *
 * Drop-in boundary for the reference's hot path (tlroy/thermalporous): everything below
 * `self.solver.solve()` (thermalporous/thermalmodel.py:165), which in the reference is executed by
 * TSFC/PyOP2-generated kernels, PETSc SNES/KSP/PC/Mat and hypre.  The reference is pure Python and
 * reaches that code through petsc4py / Firedrake; the binding a maintainer would add is the ctypes
 * stub shown in INTEGRATION.md (thermalporous_amd/engine.py is that stub).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = usage/allocation/HIP/RCCL error (text from
 *     tp_last_error), >0 is never returned; solver outcomes are reported through out-parameters
 *     using PETSc's numbering of SNES/KSP converged (>0) / diverged (<0) reasons, so the Python
 *     side can raise ConvergenceError exactly where Firedrake does (thermalmodel.py:170,210).
 *   - all arithmetic is IEEE float64; indices int32/int64.
 *   - "internal" axis order: axis 0 fastest in memory, axis 2 is the slab axis of the 1-D
 *     multi-GPU decomposition.  Cell arrays passed through this API hold the rank's slab WITH
 *     one halo plane on each side along axis 2:  ntot = n0*n1*(n2+2), owned cell (i0,i1,i2) at
 *     i0 + n0*i1 + n0*n1*(i2+1).  Vectors are field-major: b planes of ntot doubles
 *     (p, T[, S_o]) -- the same field-major ordering as the reference's V*V*V mixed space.
 *   - Jacobian storage ("stencil-of-blocks"): 7*b*b planes of ntot doubles,
 *     plane ((s*b + r)*b + c), stencil slot s: 0 diag, 1 -a0, 2 +a0, 3 -a1, 4 +a1, 5 -a2, 6 +a2.
 *   - not thread-safe per context; one host thread drives one context (= one GPU).
 *   - host pointers are never retained after return.
 */
#ifndef THERMALPOROUS_HIP_H
#define THERMALPOROUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tp_ctx tp_ctx;

/* Grid of this rank's slab.  Replaces geo.Nx/Ny/Nz/Dx/Dy/Dz + the DQ0 space
 * (rectanglegeo.py:28-34,64-65, boxgeo.py:31-44,85-86). */
typedef struct tp_grid {
    int32_t n0, n1, n2;      /* owned cells along internal axes (n2 = this rank's planes)     */
    int32_t gn2, off2;       /* global extent along axis 2 and this rank's first global plane */
    double  h[3];            /* cell sizes along internal axes                                */
    int32_t gaxis;           /* internal axis on which gravity acts (physical z), -1 = none   */
    int32_t nphase;          /* 1: unknowns (p,T)   2: unknowns (p,T,S_o)                     */
    int32_t rank, nranks;    /* slab index / number of slabs (one process per GPU)            */
} tp_grid;

/* physicalparameters.py:9-35 (scalars only; closure laws are compiled into the kernels). */
typedef struct tp_params {
    double ko, kw, kr, c_v_w, c_v_o, c_r, rho_r, p_inj, p_prod, T_inj, T_prod, API, p_ref, g,
           S_o, U, rate;
} tp_params;

/* One per-cell source entry: a well (wellcase.py:78-108,171-266) or heater (heatercase.py:63-77)
 * restricted to one cell; wt = delta_i*|E_i| (sums to 1 over a well).  cell = LOCAL index into
 * the slab-with-halo array. */
typedef struct tp_source {
    int64_t cell;
    int32_t kind;            /* 0 producer, 1 injector, 2 heater */
    int32_t constant_rate;   /* flow_rate_constant variants (wellcase.py:201-202,237-266) */
    double  wt, bhp, max_rate, WI;
} tp_source;

/* Solver options = the subset of the PETSc options dicts the hot path honours
 * (singlephase.py:289-354, twophase.py:416-433,531-597). */
typedef struct tp_options {
    int32_t pc_kind;         /* 0 = pc_cpr (CPRStage1PC + bjacobi/ILU0), 1 = pc_cptr (CPTRStage1PC
                                with fieldsplit Schur FULL, V(App), V(S~)), 2 = pc_fieldsplit_cd
                                (single-phase: fieldsplit Schur FULL on (p,T) with V(App) and the
                                ConvDiffSchurPC V(S~), no second stage; singlephase.py:309-319),
                                3 = pc_cptramg[_QI|_TI] (CPTRStage1PC with ONE system-AMG V-cycle on the 2x2-block
                                (p,T) operator Atilde_00 + bjacobi/ILU0; twophase.py:552-566),
                                4 = pc_bilu (bjacobi + ILU(ilu_levels) alone; twophase.py:758-762, singlephase.py:402-406) */
    int32_t decoup;          /* 0 "No", 1 "QI", 2 "TI", 3 "QI_temp", 4 "TI_temp" (option key sub_0_cpr_decoup;
                                the _temp variants decouple both T and S: two-phase pc_cpr only) */
    double  ksp_rtol, ksp_atol;
    int32_t ksp_max_it, ksp_restart;
    double  snes_rtol, snes_atol, snes_stol;
    int32_t snes_max_it;
    double  amg_omega;       /* damped-Jacobi weight of the AMG smoother */
    int32_t amg_nu;          /* pre/post smoothing sweeps */
    int32_t amg_min_cells;   /* coarsest-grid size (dense solve) */
    int32_t ilu_t1, ilu_t2;  /* bjacobi tile extent along axes 1,2 (t1*t2 <= 64: one wavefront per tile) */
    int32_t ilu_t0;          /* tile extent along axis 0 (<= 0: the whole line) */
    int32_t amg_full_levels; /* V(nu,nu) on the first amg_full_levels levels ... */
    int32_t amg_coarse_pre, amg_coarse_post;  /* ... V(coarse_pre, coarse_post) below (coarse_post >= 1) */
    int32_t amg_mid_skip;    /* 1: every second level between the full levels and the <= 1024-cell levels is a pure
                                transfer level (no smoothing): two coarsening directions per smoothing level there */
    int32_t amg_tail_post;   /* post-sweeps on the levels of <= 1024 cells (they run inside one workgroup, where a
                                sweep costs ~2 us: small grids live entirely there and want the stronger cycle) */
    int32_t amg_single;      /* 1: AMG operators/weights stored in fp32 (vectors and arithmetic stay fp64) */
    int32_t schur_a11;       /* what preconditions the Schur complement of pc_kind 1/2 (pc_fieldsplit_schur_precondition):
                                0 = the convection-diffusion operator S~ (ConvDiffSchurPC / ConvDiffSchurTwoPhasesPC);
                                1 = a11: A_11, the T-T block after decoupling (pc_fieldsplit_a11, pc_cptr_a11);
                                2 = selfp (pc_kind 2, one GPU): Sp = A11 - A10 diag(A00)^-1 A01 (pc_fieldsplit_selfp,
                                    singlephase.py:322-330): V-cycle of the hierarchy of Sp's 7-point collapse (far
                                    entries lumped onto the diagonal) + one damped-Jacobi sweep on the exact Sp */
    int32_t amg_gather_cells;/* multi-GPU: AMG levels with more cells than this stay distributed over the slabs
                                (halo exchange per sweep); smaller ones are gathered and replicated on every
                                rank.  < 0: replicate the whole hierarchy.  Ignored on one GPU. */
    /* Factorisation of the Schur split on (p,T) of pc_kind 1 and 2 (pc_fieldsplit_schur_fact_type, pc_fieldsplit_schur_scale;
     * DESIGN.md 4.6h).  NOTE for ABI readers: the two fields stand HERE, between amg_gather_cells and amg_dom_tau (the tests of
     * earlier options pin the order of the fields further down): schur_fact fills the four bytes of padding that preceded
     * amg_dom_tau, every field from amg_dom_tau on moved by 8 and sizeof(tp_options) grew by 8; recompile callers.
     * With r0, r1 the stage's right-hand sides, K0 = K(A00) (one V-cycle, or the s1_ksp inner solve) and KS = K(S) (the S~ cycle,
     * the A11 cycle of schur_a11 1, the cycle + Jacobi sweep of schur_a11 2):
     *   0 full   y0 = K0 r0 ; y1 = KS (r1 - A10 y0) ; y0 = K0 (r0 - A01 y1)      K0 twice, KS once
     *   1 lower  y0 = K0 r0 ; y1 = KS (r1 - A10 y0)                              K0 once,  KS once
     *   2 upper  y1 = KS r1 ; y0 = K0 (r0 - A01 y1)                              K0 once,  KS once
     *   3 diag   y0 = K0 r0 ; y1 = schur_scale KS r1                             K0 once,  KS once
     * Every S stage of pc_order uses the same factorisation.  Refused, naming both options, unless 0: pc_kind 0, 3, 4 (no Schur
     * split) and fs_additive (PETSc's additive split is no Schur factorisation). */
    int32_t schur_fact;      /* 0 full (default: the launch sequence is unchanged), 1 lower, 2 upper, 3 diag */
    double  schur_scale;     /* schur_fact 3: the factor on KS r1 (PETSc's default -1); finite, and -1 (or 0, a zeroed field) otherwise */
    double  amg_dom_tau;     /* relaxation-only truncation: the first V(nu,nu) level whose operator has
                                max_i sum_{j!=i}|a_ij| / |a_ii| <= amg_dom_tau ends the cycle with two damped-Jacobi
                                sweeps (no coarse-grid correction: damped Jacobi already contracts by
                                1 - omega (1 - tau) per sweep there; BoomerAMG's max_row_sum rule for diagonally dominant
                                rows).  Hits the temperature operator S~ of pc_cptr, never the pressure.  0: off. */
    int32_t ilu_levels;      /* stage 2 fill level: 0 = block-ILU(0) (sub_1_sub_pc_factor_levels 0, the presets' default),
                                1 = block-ILU(1) (pc_cprilu1_gmres, twophase.py:653-668): 13-block rows, the sweeps
                                take 4 steps of skew per axis-2 plane and 2 per axis-1 line instead of 1 and 1 */
    /* Temperature stage of the composite (the reference's cprctr composites, CTRStage1PC).  NOTE for ABI readers:
     * the field stands HERE, between ilu_levels and fs_additive (the tests of earlier options pin the order of every field from
     * fs_additive on): every field from fs_additive on moved and sizeof(tp_options) grew by 8; recompile callers.
     * 1 appends one stage T behind the last stage of pc_order (SIT, IST, ISIT, SIST): r = x - J y over all b columns of y,
     * y_T += V(A_TT) r_T, one V-cycle of a scalar hierarchy set up on the T-T block of the UNDECOUPLED Jacobian (the composite's
     * own operator), coarsened by the conduction strengths vol / h^2; every other field of y stays as it is.  The hierarchy follows
     * the amg_* options like the other scalar ones; the s1_* inner solves do not apply to it.
     * Scope limits (refused naming both options, never ignored; the context stays usable): pc_kind 0 and 1 only (not 2, 3, 4);
     * one slab / rank only. */
    int32_t pc_ctr;          /* 0 (default: the launch sequence is unchanged), 1 */
    int32_t fs_additive;     /* pc_kind 2: 1 = PCFIELDSPLIT additive on (p,T) -- y_p = V(A_pp) x_p, y_T = V(A_TT) x_T, no coupling
                                (pc_fieldsplit_diag, singlephase.py:371-375) -- instead of Schur FULL */
    /* Order of the composite's stages (pc_composite_pcs).  NOTE for ABI readers: the field stands HERE, between
     * fs_additive and ksp_reorth (the tests of earlier options pin the order of every field from ksp_reorth on).  It fills the four
     * bytes of padding that preceded ksp_reorth_eta: ksp_reorth moved by 4 bytes, no other field moved and sizeof(tp_options) is
     * unchanged; recompile callers.
     * PCCOMPOSITE multiplicative over a sequence s_1 .. s_m of the two stages S (CPR / CPTR / the system V-cycle) and I (bjacobi +
     * block-ILU): y = 0; for k = 1..m: r = x - J y (k = 1: r = x), y += B_{s_k} r.  The residual is taken over all b rows and all b
     * columns of y.  B_I r is the configured stage-2 solve (one factorisation per set-up, shared by both I stages of 2); B_S r is
     * what tp_stage1_apply computes for r: as a later stage it ADDS into y's primary fields and leaves the secondary ones alone.
     * Refused, naming both options, with pc_kind 2 (no second stage) and 4 (no first stage) unless 0. */
    int32_t pc_order;        /* 0 SI (default: the launch sequence is unchanged), 1 IS, 2 ISI, 3 SIS */
    /* Gram-Schmidt refinement of the outer FGMRES (ksp_gmres_cgs_refinement_type).  NOTE for ABI readers: the
     * two fields stand HERE, between fs_additive and ilu_whole, not at the struct's tail (the tests of earlier options pin the
     * order of every field from ilu_whole on): every field from ilu_whole on moved and sizeof(tp_options) grew; recompile callers.
     * One orthogonalisation step is h = V^T w ; w <- w - V h ; n1 = ||w||^2 (classical Gram-Schmidt in one pass).  A SECOND pass
     * c = V^T w ; w <- w - V c ; h <- h + c ; n2 = ||w||^2 follows when a flag on the device is set: by ksp_reorth 2 always, by
     * ksp_reorth 1 when n1 < eta^2 (||h||^2 + n1) with every sum finite (the vector lost more than 1 - eta of its length: the
     * DGKS / Rutishauser rule).  The host neither decides nor waits: the second pass's kernels are always enqueued and return
     * at once when the flag is clear, and everything the loop reads afterwards (the k coefficients, ||w||^2) holds the final
     * values in the same places.  FGMRES with fp64 bases only: refused with ksp_kind 1 and with ksp_basis_single. */
    int32_t ksp_reorth;      /* 0 never (default: the launch sequence is unchanged), 1 if needed, 2 always */
    double  ksp_reorth_eta;  /* eta in (0, 1) (default 2^-1/2): the rule of ksp_reorth 1; range-checked whenever ksp_reorth is not 0 */
    /* Eisenstat-Walker inexact Newton (snes_ksp_ew): tp_newton_solve chooses the relative tolerance eta_k of its k-th
     * linear solve from the nonlinear residuals instead of solving every system to ksp_rtol.  NOTE for ABI readers: the seven fields
     * stand HERE, between ksp_reorth_eta and ilu_whole, not at the struct's tail (the tests of earlier options pin the order of every
     * field from ilu_whole on, and that of pc_order, ksp_reorth, ksp_reorth_eta before): every field from ilu_whole on moved and
     * sizeof(tp_options) grew; recompile callers.
     * With ||F_k|| the residual norm where system k is formed, rho_k the residual norm the Krylov solver returned for it:
     *   k == 0:     eta = ew_rtol0
     *   version 1:  eta = | ||F_k|| - rho_{k-1} | / ||F_{k-1}|| ;            s = pow(eta_{k-1}, ew_alpha2)
     *   version 2:  eta = ew_gamma pow(||F_k|| / ||F_{k-1}||, ew_alpha) ;    s = ew_gamma pow(eta_{k-1}, ew_alpha)
     *   k > 0:      if s > ew_threshold: eta = max(eta, s)                   (safeguard)
     *   always:     eta = min(eta, ew_rtolmax); eta = max(eta, ksp_rtol)     (cap, then floor)
     * and solve k stops at max(eta_k ||F_k||, ksp_atol).  One deliberate difference from PETSc: the configured ksp_rtol stays as a
     * FLOOR (PETSc overwrites it); the two differ only where the formula asks for more digits than the user ever wanted.  ksp_rtol >
     * ew_rtolmax is refused.  PETSc's version 3 is not implemented.  The option lives in tp_newton_solve only: tp_fgmres and tp_bcgs
     * called on their own use ksp_rtol.  Every ew_* field must keep its default (or 0) while ksp_ew is 0 (refused, never ignored). */
    int32_t ksp_ew;          /* 0 off (default: the launch sequence and every result are unchanged), 1 or 2: the version */
    double  ew_rtol0;        /* eta_0 in [0, 1) (snes_ksp_ew_rtol0; default 0.3) */
    double  ew_rtolmax;      /* the cap in [0, 1), >= ksp_rtol (snes_ksp_ew_rtolmax; default 0.9) */
    double  ew_gamma;        /* in [0, 1] (snes_ksp_ew_gamma; default 1) */
    double  ew_alpha;        /* in (1, 2] (snes_ksp_ew_alpha; default (1 + sqrt 5) / 2) */
    double  ew_alpha2;       /* in (1, 2] (snes_ksp_ew_alpha2; default (1 + sqrt 5) / 2) */
    double  ew_threshold;    /* in (0, 1) (snes_ksp_ew_threshold; default 0.1) */
    int32_t ilu_whole;       /* 1: ONE bjacobi block per rank = block-ILU(0) of the whole slab, PETSc's default bjacobi and the
                                reference's `sub_1_pc_bjacobi_blocks: 1` (tests/test_homo_wells.py:112, pc_cptr_a11
                                twophase.py:612): couplings between the tiles are kept; the tiles (ilu_t0 x ilu_t1 x ilu_t2,
                                now only the unit of the sweep) are swept one tile-diagonal T0+T1+T2 per launch.  ILU(0) only. */
    /* Red-black Gauss-Seidel on the top levels of the scalar hierarchies (pressure, S~ / A_11).  NOTE for ABI readers: the two
     * fields stand HERE, between ilu_whole and ilu_block (the tests of earlier options pin the order of every field from ilu_block
     * on): every field from ilu_block on moved and sizeof(tp_options) grew; recompile callers.
     * Level l is a GS level when l < amg_gs_levels and it has more than 1024 cells (above the single-workgroup tail); every other
     * level keeps damped Jacobi.  Cell (i0, i1, i2) of a level is red when i0 + i1 + i2 is even; a half-sweep of one colour sets
     * x_i <- x_i + (b_i - (A x)_i) / a0_i on its cells (no damping: amg_omega is not used); forward sweep = red then black,
     * backward = black then red.  A GS level is V(g, g), g = amg_gs_sweeps: g forward sweeps from the zero guess, residual,
     * coarse correction, g backward sweeps; as the relaxation-only level of amg_dom_tau it returns B^g F^g 0.
     * Scope limits of this implementation (refused naming both options, never ignored; the context stays usable): one slab only;
     * not with amg_line_levels > 0, amg_single, pc_kind 3 or schur_a11 = 2. */
    int32_t amg_gs_levels;   /* L >= 0, <= amg_full_levels.  0 (default): off, the point-Jacobi launch sequence */
    int32_t amg_gs_sweeps;   /* g in 1..4 (default 1); must be 1 while amg_gs_levels is 0 */
    int32_t ilu_block[3];    /* bjacobi block = a BOX of ilu_block[0] x [1] x [2] whole cells (internal axis order), independent of the
                                sweep tile: `sub_1_pc_bjacobi_blocks N` for blocks larger than one tile (tests/test_homo_wells.py:112,125,
                                twophase.py:612).  Blocks start at the slab's origin (the last one along an axis is the ragged one);
                                couplings inside a block are kept, those across block faces dropped.  Every block is cut into
                                its own ilu_t0 x ilu_t1 x ilu_t2 tiles (partial tile at the block's upper end) and swept one
                                block-local tile-diagonal per launch, all blocks in the same launch.  All zero: off (every
                                tile is a block); otherwise an entry <= 0 or beyond the slab means the whole extent.  Blocks
                                no larger than the tile are the per-tile path with the tile clipped to the block.  ilu_whole
                                is the case block = slab and excludes this field.  ILU(0) only for multi-tile blocks. */
    int32_t ilu_single;      /* 1: the block-ILU(0) factor stream stored in fp32 (the factorisation, the sweeps' arithmetic and
                                every vector stay fp64): half the factor's memory and 43 % fewer bytes per sweep.  The default
                                per-tile ILU(0) only: not with ilu_levels 1, ilu_whole or an ilu_block of several tiles */
    /* Line search of tp_newton_solve (snes_linesearch_type).  NOTE for ABI readers: these fields stand HERE, between
     * ilu_single and amg_line_levels, not at the struct's tail (the tests of earlier options pin the order of every field from
     * amg_line_levels on): every field from amg_line_levels on moved and sizeof(tp_options) grew; recompile callers.
     * ls_kind 0 `basic` (the default): every Krylov correction is applied at full length; the launch sequence is unchanged.
     * ls_kind 1 `bt`: Armijo backtracking.  From iterate u0 with residual F0 and correction dx, trial t sets u = u0 - lambda dx
     * and accepts when ||F(u)||^2 is finite and <= (1 - 2 ls_alpha lambda) ||F0||^2; a rejected trial shrinks lambda by the
     * minimiser of the quadratic (ls_order 2, or only one finite rejected trial) or cubic (ls_order 3) interpolant clamped to
     * [0.1, 0.5] lambda, a non-finite trial halves it.  The slope is taken as -||F0||^2 (exact for an exact linear solve, within
     * ksp_rtol otherwise: no mat-vec is spent on it).  The first trial uses the fused residual+Jacobian assembly, later trials
     * the residual only, and an iteration accepted after several trials re-assembles the Jacobian once at the accepted state.
     * A search that fails (ls_max_it trials, or lambda < ls_minlambda) restores u0 and ends the solve with reason -6
     * (SNES_DIVERGED_LINE_SEARCH).  Every bt field below must keep its default while ls_kind is 0 (refused, never ignored). */
    int32_t ls_kind;         /* 0 basic, 1 bt */
    int32_t ls_order;        /* 2 quadratic, 3 cubic (snes_linesearch_order; default 3) */
    int32_t ls_max_it;       /* most trials per Newton iteration, >= 1 (snes_linesearch_max_it; default 40) */
    double  ls_alpha;        /* Armijo parameter in (0, 0.5) (snes_linesearch_alpha; default 1e-4) */
    double  ls_maxstep;      /* first trial: lambda <= ls_maxstep / ||dx||_2, > 0 (snes_linesearch_maxstep; default 1e8) */
    double  ls_minlambda;    /* ABSOLUTE smallest lambda in [0, 1) (snes_linesearch_minlambda; default 1e-12) */
    double  ls_max_change[3];/* first trial: lambda <= ls_max_change[f] / max|dx_f| per field (p, T, S_o); <= 0: off (default) */
    int32_t amg_line_levels; /* L >= 0: the first L levels of the scalar hierarchies (pressure, S~ / A_11) smooth with line-Jacobi
                                along internal axis 0, x <- x + amg_omega T^-1 (b - A x), T = the tridiagonal part of the level's
                                operator along that axis (one Thomas solve per line), instead of damped point Jacobi.  A level
                                is a line level when it is above the single-workgroup tail, among the first L levels and has
                                n0 >= 2; L <= amg_full_levels.  0 (default): off, the point-Jacobi launch sequence.  One slab
                                only; not with amg_single, pc_kind 3 or schur_a11 = 2 (refused, never ignored) */
    int32_t ksp_basis_single;/* 1: the two FGMRES bases V and Z stored in fp32 (compressed-basis GMRES): compact vectors of the owned
                                entries, half the Krylov workspace and half the bytes Gram-Schmidt moves; every sum, the iterate,
                                the residual and the preconditioner stay fp64.  z_j is rounded BEFORE J is applied to it, so only
                                the rounding of v_{j+1} perturbs the Arnoldi relation.  A restart cycle also ends when its
                                recurrence residual has fallen to ksp_single_floor times the true residual it started from, and
                                convergence is declared only on a recomputed true residual ||b - J x||, which is the rnorm
                                returned.  FGMRES only: refused with ksp_kind 1.  0 (default): the fp64 bases.  NOTE for ABI readers:
                                this field and ksp_single_floor were added HERE, before ksp_kind, not at the struct's tail: every
                                field from ksp_kind on moved by 16 bytes and sizeof(tp_options) grew; recompile callers */
    double  ksp_single_floor;/* theta of ksp_basis_single, 2^-24 < theta < 1 (1e-7): what one cycle may reduce the residual by
                                before the rounded basis has lost its orthogonality.  Ignored when ksp_basis_single is 0 */
    int32_t ksp_kind;        /* outer Krylov method of tp_newton_solve: 0 = restarted FGMRES (the default: ksp_type fgmres, or gmres with
                                ksp_pc_side right), 1 = right-preconditioned (flexible) BiCGStab (ksp_type fbcgs, or bcgs with
                                ksp_pc_side right): a short recurrence on seven vectors plus the shared scratch w2 (what tp_ksp_info
                                reports), two preconditioner applications per iteration, every scalar on the device; ksp_restart has no effect on it */
    /* Inner solve of the stage-1 PRESSURE block K(A00) (pc_kind 0, 1, 2) or of the (p,T) SYSTEM block (pc_kind 3): what PETSc
     * does when the sub-solver's ksp_type is not preonly.  The V-cycle becomes the (right) preconditioner of a small
     * Krylov method whose every scalar stays on the device, so it lives inside the captured pc_apply graph:
     *   s1_ksp 0 preonly     one V-cycle (the default; the launch sequence is unchanged)
     *          1 richardson  s1_max_it V-cycles as a stationary iteration from x0 = 0: x <- x + V(r - A x)
     *                        (pc_hypre_boomeramg_max_iter k, or ksp_type richardson + ksp_max_it k)
     *          2 fgmres      right-preconditioned GMRES(s1_max_it) without restart, 1 <= s1_max_it <= 32
     * Exactly s1_max_it iterations are always LAUNCHED; convergence (recurrence residual <= max(s1_rtol ||rhs||, s1_atol),
     * or a happy breakdown) is latched on the device at iteration j*, and the result is the iterate GMRES returns when it
     * stops at j*: the later iterations are wasted work, not different arithmetic.  The Schur / temperature solves stay one
     * V-cycle.  Several GPUs: needs the replicated stage-1 hierarchy (amg_gather_cells < 0, or a grid small enough to be
     * gathered); with slab-distributed top levels tp_pc_setup fails. */
    int32_t s1_ksp, s1_max_it;
    double  s1_rtol, s1_atol;
} tp_options;

/* Result of one nonlinear solve (SNES iteration number / linear iterations / reason:
 * thermalmodel.py:327-336). */
typedef struct tp_solve_info {
    int32_t nits, lits, reason;     /* reason: SNES numbering; <0 diverged */
    int32_t last_ksp_reason;
    double  fnorm0, fnorm;
    int32_t vcycles;
} tp_solve_info;

const char *tp_last_error(void);
int tp_version(void);
/* The TP_* runtime switches (environment variables) the library reads, DESIGN.md 10: their number, and switch i as five
 * static strings -- environment name, kind ("flag" | "int" | "real"), default as documented, when it is read ("process":
 * once per process | "setup": at every preconditioner set-up) and a one-line effect.  No context, no GPU. */
int tp_switch_count(void);
int tp_switch_entry(int i, const char **name, const char **kind, const char **dflt, const char **when, const char **effect);

/* lifetime ------------------------------------------------------------------------------------ */
int tp_create(const tp_grid *grid, const tp_params *prm, const tp_options *opt, int device, tp_ctx **out);
int tp_destroy(tp_ctx *ctx);
int tp_set_options(tp_ctx *ctx, const tp_options *opt);
/* multi-GPU: rank 0 calls tp_comm_unique_id, the 128 bytes are broadcast by the host launcher
 * (torch.distributed), then every rank calls tp_comm_init (RCCL ncclCommInitRank). */
int tp_comm_unique_id(void *id128);
int tp_comm_init(tp_ctx *ctx, const void *id128);
/* in-process slab group: N contexts driven by N host threads on ONE GPU exchange through device copies
 * instead of RCCL (same call sequence) -- validates the slab algorithm where only one GPU exists. */
int tp_local_group_create(int32_t nranks, void **group);
int tp_local_group_destroy(void *group);
int tp_comm_init_local(tp_ctx *ctx, void *group);

/* problem data: geo fields (homogeneousgeo.py:13-20, SPE10model*.py) -- arrays of ntot doubles
 * (slab + halo planes); name in {"phi","K0","K1","K2","kT"}.  tp_finalize_fields builds the face
 * transmissibilities H(K)|e|/Delta_h (singlephase.py:98-103). */
int tp_set_field(tp_ctx *ctx, const char *name, const double *host, int64_t n);
int tp_finalize_fields(tp_ctx *ctx);
int tp_set_sources(tp_ctx *ctx, int32_t n, const tp_source *entries);   /* wells/heaters: wellcase.py:78-108,171-266,
                                                                           heatercase.py:63-77, sourceterms.py:77-84,155-269 */
/* Dirichlet sides of the box (every side is closed to flow and heat until one is set).  side = 2*a + d in
 * internal axes: a the axis, d = 0 its low-index side, d = 1 its high-index side.  kind: 0 none (removes the side; values may be
 * NULL), 1 open (flow and conduction to the ghost state), 2 thermal (conduction only: the ghost pressure cannot change any output
 * bit).  values: the ghost state (p_b, T_b[, S_b]) per boundary face, field-major, b * nfaces doubles; a face is numbered over
 * the other two internal axes, the lower axis fastest, so nfaces is n1*n2, n0*n2 or n0*n1.  The face is an interior face to a ghost
 * cell half a cell away that has the cell's own porosity and static conductivity: same upwinding, gravity and harmonic
 * conduction; only R, the diagonal block of J and the diagonal of S~ gain terms.  Callable any time after tp_finalize_fields; a
 * later call replaces the side, so the values may change between time steps.  Checked: the side and kind ranges, nfaces against
 * the grid, finite values, S_b in [0, 1].  One slab only: with nranks > 1 the call fails, naming the boundary and nranks.
 * tp_boundary_flux: out[side*b + r] = the sum over the faces of `side` of what they added to equation r of R at the last
 * assembly (tp_residual, tp_jacobian, or the last one of tp_newton_solve): the residual's sign, positive leaves the domain, and
 * the equation's own scaling; summed on the host in face order; 0 for a side that is not set.  6*b doubles. */
int tp_set_boundary(tp_ctx *ctx, int32_t side, int32_t kind, const double *values, int64_t nfaces);
int tp_boundary_flux(tp_ctx *ctx, double *out);
/* Graded tensor-product grid: one width per cell index along each internal axis instead of tp_grid.h.  h0, h1,
 * h2: host arrays of n0, n1, n2 doubles, whose lengths must be the grid's extents (a 2-D grid passes h2 = {1}); all three
 * pointers NULL: back to the uniform grid of tp_grid.h.  Cell volume |E_c| = h0[i0] h1[i1] h2[i2]; a face along a between the
 * cells P (lower index) and M has area |e| = |E_P|/h_a[i_P], half distances d = h_a/2 and c = d/|e| on each side:
 * T^K = K_P K_M/(c_P K_M + c_M K_P), gam = g (d_P + d_M)/2 on the gravity axis, conduction H = k_P k_M/(c_P k_M + c_M k_P); a
 * boundary face (tp_set_boundary) has both half distances h_a/4 of its cell.  Equal widths reproduce the uniform formulas up to
 * rounding; with no spacing set every result is bit for bit that of the uniform code.  Checked: the lengths, finite positive
 * widths.  The call marks the fields as not finalised: tp_finalize_fields recomputes the interior and boundary transmissibilities
 * (and drops the AMG hierarchies, whose conduction strengths become the mean of |e|/(d_P + d_M) over an axis's interior faces).
 * tp_grid.h stays the mean widths and is read by nothing once spacing is set.  One slab only: the call fails on a context with a
 * communicator or an in-process slab group (or nranks > 1), and tp_comm_init / tp_comm_init_local fail on a context with spacing.
 * tp_spacing_info: *graded = 1 if spacing is set, and per internal axis the smallest and largest width (tp_grid.h when uniform). */
int tp_set_spacing(tp_ctx *ctx, const double *h0, int64_t n0, const double *h1, int64_t n1, const double *h2, int64_t n2);
int tp_spacing_info(tp_ctx *ctx, int32_t *graded, double *hmin, double *hmax);
/* Saturation functions of the two-phase model (off by default: kr_o = S_o, kr_w = 1 - S_o and one pressure for
 * both phases, physicalparameters.py:92-98, the only form the reference executes; its Brooks-Corey members :100-152 are dead code).
 * With D = 1 - Sr_o - Sr_w, Se_o = (S_o - Sr_o)/D, Se_w = (1 - S_o - Sr_w)/D:
 *   relperm 1 (Corey):    kr_o = kro_max Se_o^n_o for 0 < Se_o < 1, 0 at and below 0, kro_max at and above 1; kr_w alike on Se_w
 *                         with krw_max, n_w; the derivatives are exactly 0 at and beyond either end (Brooks-Corey is Corey with
 *                         n_o = n_w = (2 + 3 lmbda)/lmbda: the caller translates, engine.pack_satfn);
 *   capillary 1 (linear): p_c = p_ct (1 - min(max(Se_w, 0), 1));
 *   capillary 2 (Brooks-Corey): p_c = p_ct s^(-1/lmbda), s = min(max(Se_w, pc_se_min), 1);
 * p_c = p_o - p_w with p_o = p the unknown (twophase.py:104-106).  p_w = p - p_c(S_o) is where water's density is evaluated in the
 * accumulation (new and old), the water mobility and water's gravity head, and the water driving force is p_w+ - p_w- -
 * gam (rho_w+ + rho_w-); oil, kT, the weights and the tie rules do not change; a Dirichlet ghost state goes through the same
 * closures.  Wells keep drawdown and densities at p; a producer's total mobility and phase split use kr_a(S_o)/mu_a.  The 7-point
 * block structure of J and S~ is unchanged.  NULL, or relperm 0 with capillary 0: back to the default, whose results are bit for
 * bit those of a context that never heard of this call.  Checked, each failure naming the key: relperm in 0..1, capillary in
 * 0..2, every number finite, Sr_o >= 0, Sr_w >= 0, Sr_o + Sr_w < 1, n_o >= 1, n_w >= 1, kro_max > 0, krw_max > 0, lmbda > 0,
 * p_ct >= 0, 0 < pc_se_min <= 1; a non-default setting on a single-phase context fails (no saturation).  Callable any time
 * between two solves, on every slab's context alike (the setting is pointwise); the accumulation of the old state is recomputed.
 * tp_saturation_info: the setting in force (the defaults below when none) and *active = 1 unless it is the default. */
typedef struct tp_satfn {
    int32_t relperm;         /* 0 linear (default), 1 Corey                                    */
    int32_t capillary;       /* 0 none (default), 1 linear, 2 Brooks-Corey                     */
    double  Sr_o, Sr_w;      /* residual oil, connate water (0, 0)                             */
    double  n_o, n_w;        /* Corey exponents (2, 2)                                         */
    double  kro_max, krw_max; /* end points (1, 1)                                             */
    double  lmbda;           /* Brooks-Corey pore-size index of p_c (2)                        */
    double  p_ct;            /* capillary entry pressure, MPa (0)                              */
    double  pc_se_min;       /* floor of Se_w in the Brooks-Corey p_c (0.05)                   */
} tp_satfn;
int tp_set_saturation_functions(tp_ctx *ctx, const tp_satfn *sat);
int tp_saturation_info(tp_ctx *ctx, tp_satfn *out, int32_t *active);

/* Completed wells (tp_version >= 101): a well perforates many cells, shares ONE bottom-hole pressure along its
 * bore, sees the hydrostatic head between its perforations, and is operated at a TOTAL rate until its BHP limit is reached, then
 * at that limit.  Beside tp_set_sources, whose entries keep a private bhp per cell; a cell may carry legacy entries (a heater) and
 * one perforation.  With u_k the state of perforation k's cell:
 *   a_k     = WI_k lambda_k      lambda: what a tp_source entry of the kind multiplies its drawdown by -- producer lambda_o +
 *                                lambda_w (kr/mu of the saturation functions in force), single-phase 1/mu_o(T_k); injector
 *                                1/mu_w(T_k), single-phase 1/mu_o(T_k)
 *   theta_k = p_k - rho_w g (z_ref - z_k)   z up, g = tp_params.g; no head on a grid without a gravity axis.  rho_w is FROZEN over
 *                                a time step: computed whenever the old state is set -- producer: sum_k WI_k (lambda_o rho_o +
 *                                lambda_w rho_w) / sum_k WI_k lambda_t over all its perforations (0 if none is mobile); injector:
 *                                the injected fluid at (p_old of the perforation nearest to z_ref, T_inj)
 *   q_k     = -a_k (theta_k - bhp) on open perforations (producer: theta_k > bhp, injector: theta_k < bhp), 0 on closed ones: no
 *                                cross-flow.  Production is negative, as in tp_well_rates.
 * Rate mode: bhp solves sum_k q_k = -Q (producer) or +Q (injector) by active-set rounds -- all perforations open, bhp = (sum_open
 * a_k theta_k -+ Q) / sum_open a_k, close what that bhp shuts, repeat until nothing changes; a closed perforation stays closed.
 * BHP mode, bhp = bhp_limit with open/closed decided against it, when the rate-mode bhp violates the limit (a producer's minimum,
 * an injector's maximum) or no mobile perforation is open.  rate = 0 or shut != 0: the well adds nothing.
 * A perforation adds to R what a tp_source entry of its kind adds for the rate q_k with wt = 1 (the cell's own normalised delta),
 * and its derivative AT FIXED bhp to the diagonal block of J and to S~.  In rate mode bhp depends on every perforated cell: the
 * exact Jacobian is J + c b^T per well, c_k = dR_k/dbhp, b_j = dbhp/du_j, b numbers each per perforation, zeros on closed ones.
 * tp_newton_solve, tp_fgmres, tp_bcgs and tp_spmv apply J + sum_w c_w b_w^T; the preconditioner, tp_export_jacobian and every
 * tp_time_kernel product keep the 7-point part.  A well of ONE perforation has no off-diagonal term: its c b^T is added to the
 * diagonal block and its exported factors are zero.
 * tp_set_wells: wells[w] owns perfs[first .. first + count); nwells = 0 removes all wells (the results are then bit for bit those
 * of a context that never had one).  cell: the local index of tp_source.cell; z, z_ref: elevations in the units of tp_grid.h.
 * Checked, each failure naming the well and perforation: kind 0/1, finite numbers, WI > 0, rate >= 0, cells inside the box, no cell
 * and no entry of perfs used twice.  One slab only: with nranks > 1 the call fails, and tp_comm_init / tp_comm_init_local fail on a
 * context with wells.  Callable any time between two solves; an old state that is already set gives the head densities at once.
 * tp_set_well_control: new rate, bhp_limit and shut flag of one well, between two time steps (rho_w is not recomputed).
 * tp_well_info: nwells entries describing the last assembly (tp_residual, tp_jacobian, the last one of tp_newton_solve).
 * tp_well_perf_rates: per entry of perfs the total, water and oil rate of that assembly (two-phase producers split by mobility;
 * a two-phase injector's rate is water, every single-phase rate is oil); any pointer may be NULL.
 * tp_well_factors: c and b of the last Jacobian assembly, b * nperfs doubles each, entry [r * nperfs + k] = component r (of R for
 * c, of u for b) at perforation k; all zero in BHP mode. */
typedef struct tp_well {
    int32_t kind;            /* 0 producer, 1 injector                                          */
    int32_t shut;            /* != 0: contributes nothing                                       */
    double  rate;            /* Q >= 0: total volumetric rate target, units of tp_source.max_rate */
    double  bhp_limit;       /* a producer's minimum, an injector's maximum BHP                 */
    double  z_ref;           /* datum elevation of the BHP                                      */
    int32_t first, count;    /* its perforations: perfs[first .. first + count)                 */
} tp_well;
typedef struct tp_perf {
    int64_t cell;            /* local index into the slab-with-halo array                       */
    double  WI;              /* connection index, > 0                                           */
    double  z;               /* elevation of the cell centre                                    */
} tp_perf;
typedef struct tp_well_state {
    double  bhp;
    int32_t mode;            /* 0 shut or rate 0, 1 rate, 2 BHP                                 */
    int32_t rounds;          /* active-set rounds of the last assembly                          */
    double  rate, water_rate, oil_rate;   /* sums over the perforations                         */
    double  rho;             /* the head density in force                                       */
    int32_t nopen, reserved; /* open perforations                                               */
} tp_well_state;
int tp_set_wells(tp_ctx *ctx, int32_t nwells, const tp_well *wells, int32_t nperfs, const tp_perf *perfs);
int tp_set_well_control(tp_ctx *ctx, int32_t well, double rate, double bhp_limit, int32_t shut);
int tp_well_info(tp_ctx *ctx, tp_well_state *out);
int tp_well_perf_rates(tp_ctx *ctx, double *rate, double *water_rate, double *oil_rate);
int tp_well_factors(tp_ctx *ctx, double *c, double *b);

/* state u, old state u_ (thermalmodel.py:93-94,296), time step (thermalmodel.py:13). */
int tp_set_state(tp_ctx *ctx, const double *u_host);      /* b*ntot doubles */
int tp_get_state(tp_ctx *ctx, double *u_host);
int tp_set_old_state(tp_ctx *ctx, const double *u_host);  /* NULL: u_ <- u */
int tp_set_dt(tp_ctx *ctx, double dt);
int tp_get_old_state(tp_ctx *ctx, double *u_host);
int tp_restore_state(tp_ctx *ctx);                          /* u <- u_  (thermalmodel.py:179: u.assign(u_)) */
/* two-phase saturation guard of the time loop (thermalmodel.py:193-229): min/max of S_o over the owned
 * cells of this rank, and the clamp to [0,1]; both on the device. */
int tp_saturation_range(tp_ctx *ctx, double *smin, double *smax);
int tp_clamp_saturation(tp_ctx *ctx);

/* assembly: F(u) and J = dF/du (what TSFC/PyOP2 kernels + MatSetValues do in the reference for the forms
 * singlephase.py:60-273 / twophase.py:67-411 behind self.solver.solve(), thermalmodel.py:165). */
int tp_residual(tp_ctx *ctx, double *norm2);               /* R <- F(u); ||F||_2 over all ranks */
int tp_jacobian(tp_ctx *ctx);                              /* R, J (and S~ for pc_cptr) <- at u */
int tp_get_residual(tp_ctx *ctx, double *host);            /* b*ntot */
int tp_export_jacobian(tp_ctx *ctx, double *host);         /* 7*b*b*ntot: the 7-point part; the wells' rank-1 terms: tp_well_factors */
int tp_export_schur(tp_ctx *ctx, double *host);            /* 7*ntot: ConvDiffSchur*PC operator */
int tp_well_rates(tp_ctx *ctx, double *rate, double *water_rate, double *oil_rate); /* per entry */

/* device vectors (work vectors for the PC plug-in API; ids are small ints) */
int tp_vec_create(tp_ctx *ctx, int32_t *id);
int tp_vec_set(tp_ctx *ctx, int32_t id, const double *host);
int tp_vec_get(tp_ctx *ctx, int32_t id, double *host);
int tp_vec_copy_residual(tp_ctx *ctx, int32_t id);        /* vec <- R */

/* operators (PETSc MatMult AIJ / PCApply in the reference: option dicts singlephase.py:303-354,
 * twophase.py:478-482,531-597) */
/* KSPMonitorSet analogue for the reference's per-field residual monitor (option key ksp_monitor_residuals,
 * thermalmodel.py:44-74: ksp.buildResidual() split by field).  When set, every FGMRES iteration builds the current
 * iterate x_j = Z y_j, the true residual b - J x_j (one extra SpMV) and its 2-norm per field, and calls
 * cb(its, recurrence_rnorm, field_norms[nfields], user).  Debug aid: costs about one Krylov iteration per call.
 * NULL removes the monitor. */
typedef void (*tp_ksp_monitor_fn)(int32_t its, double rnorm, const double *field_norms, int32_t nfields, void *user);
int tp_set_ksp_monitor(tp_ctx *ctx, tp_ksp_monitor_fn cb, void *user);

/* PETSc Vec kernels of one Krylov iteration (SURVEY.md 8b minimum list; KSP fgmres, twophase.py:426-432):
 *   tp_vec_create_batch  n vectors in ONE allocation (ids first..first+n-1): a Krylov basis
 *   tp_vec_dot_batch     out[i] = <v_{first+i}, w>, i < n   (VecMDot: one pass over w, one host sync)
 *   tp_vec_axpy_batch    w += sum_i coef[i] v_{first+i}     (VecMAXPY: one pass over w)
 *   tp_vec_norm2         ||x||_2                            (VecNorm)
 * Reductions run over owned cells only and are summed over the slabs (RCCL all-reduce) in multi-GPU runs. */
int tp_vec_create_batch(tp_ctx *ctx, int32_t n, int32_t *first_id);
int tp_vec_dot_batch(tp_ctx *ctx, int32_t first, int32_t n, int32_t w, double *out);
int tp_vec_axpy_batch(tp_ctx *ctx, int32_t first, int32_t n, const double *coef, int32_t w);
int tp_vec_norm2(tp_ctx *ctx, int32_t x, double *out);
/* One Gram-Schmidt step of the outer FGMRES on user vectors (the kernels of tp_options.ksp_reorth, testable alone, and the
 * orthogonalisation for callers who drive their own Krylov method over the kernels above): basis = the vectors first..first+k-1
 * of one batch, w = any vector outside them.  mode 0 | 1 | 2 and eta as ksp_reorth / ksp_reorth_eta (the context's options are
 * not read).  On return w holds the orthogonalised vector (NOT normalised), h[0..k) the coefficients (h + c after a second
 * pass), *norm2 the final ||w||^2 and *refined 1 if the second pass ran, else 0.  The step counts in tp_ksp_reorth_info. */
int tp_vec_orth_step(tp_ctx *ctx, int32_t first, int32_t k, int32_t w, int32_t mode, double eta, double *h, double *norm2,
                     int32_t *refined);
/* The same kernels on a compact fp32 batch (the storage of ksp_basis_single; exported so that they can be tested alone):
 *   tp_fvec_create_batch  n float vectors of b * owned cells entries (field-major, no halo planes) at the basis stride
 *   tp_fvec_store         slot i <- (float) x, and x <- (double) slot i in the same pass: the solver's round-and-store kernel
 *   tp_fvec_get           slot i -> host, b * owned cells floats
 *   tp_fvec_dot_batch     out[i] = <slot_i, w>, i < n, fp64 sums of widened entries
 *   tp_fvec_axpy_batch    w += sum_i coef[i] slot_i, i < n */
int tp_fvec_create_batch(tp_ctx *ctx, int32_t n, int32_t *batch);
int tp_fvec_store(tp_ctx *ctx, int32_t batch, int32_t i, int32_t x);
int tp_fvec_get(tp_ctx *ctx, int32_t batch, int32_t i, float *host);
int tp_fvec_dot_batch(tp_ctx *ctx, int32_t batch, int32_t n, int32_t w, double *out);
int tp_fvec_axpy_batch(tp_ctx *ctx, int32_t batch, int32_t n, const double *coef, int32_t w);
int tp_spmv(tp_ctx *ctx, int32_t x, int32_t y);            /* y = J x, plus sum_w c_w (b_w . x) when wells are set: the Krylov operator */
int tp_pc_setup(tp_ctx *ctx);                              /* PCSetUp: decoupling, AMG setup, ILU factor */
int tp_pc_apply(tp_ctx *ctx, int32_t x, int32_t y);        /* composite multiplicative (stage1, ILU0) */
int tp_stage1_update(tp_ctx *ctx);                         /* CPRStage1PC/CPTRStage1PC.update (preconditioners.py:875,1545) */
int tp_stage1_apply(tp_ctx *ctx, int32_t x, int32_t y);    /* ....apply (preconditioners.py:881,1550) */
int tp_ilu0_factor(tp_ctx *ctx);                           /* sub_1: bjacobi + ILU(0) numeric factorisation (singlephase.py:348-349) */
int tp_ilu0_solve(tp_ctx *ctx, int32_t x, int32_t y);
/* The stage-1 right-hand side of a LATER S stage of the composite (tp_options.pc_order), one kernel: for every primary field q
 * out_q = [x - J y]_q - sum_s d_{q,s} [x - J y]_s, with the decoupling coefficients d of the last tp_pc_setup (none for decoupling
 * "No").  y is read in all b fields (several slabs: its halo planes are exchanged first); only the npri primary planes of `out`
 * are written, owned cells only.  x, y and out must be three different vectors.  pc_kind 0, 1 or 3. */
int tp_stage_rhs(tp_ctx *ctx, int32_t x, int32_t y, int32_t out);
/* The temperature stage of the composite (tp_options.pc_ctr).  All three fail with a message while pc_ctr is 0 or
 * the preconditioner is not set up.
 * tp_ctr_rhs: row 1 of the block residual in one kernel, out_1 = x_1 - sum_s sum_k J[s][1][k] y_k(neighbour s): only the b * slots
 * Jacobian planes of row 1 are read, y in all b fields; field 1 of `out` is written (owned cells), its other planes are left
 * untouched.  x, y and out must be three different vectors.
 * tp_ctr_apply: y_1 = V(A_TT) x_1, every other field of y zero (CTRStage1PC.apply).  x and y must differ.
 * tp_ctr_info: out = {pc_ctr in effect, levels of the A_TT hierarchy (0: not built), its set-ups since tp_create, T-stage
 * applications launched since tp_create (one per tp_pc_apply / Krylov application, speculative ones included, and per tp_ctr_apply)}. */
int tp_ctr_rhs(tp_ctx *ctx, int32_t x, int32_t y, int32_t out);
int tp_ctr_apply(tp_ctx *ctx, int32_t x, int32_t y);
int tp_ctr_info(tp_ctx *ctx, int32_t out[4]);
/* The Schur split on (p,T) (tp_options.schur_fact): the factorisation and scale in force, and how often the
 * pressure solver K(A00) and the Schur solver K(S) were applied since the last tp_pc_setup.  Counted on the host where a stage-1
 * sequence is issued or replayed (tp_pc_apply and every Krylov application, speculative ones included; tp_stage1_apply): per
 * Schur stage (2, 1) under full and (1, 1) under the other three.  pc_kind 0: (1, 0) per stage; fs_additive: (1, 1); pc_kind 3
 * and 4 count nothing.  Any output pointer may be null. */
int tp_schur_info(tp_ctx *ctx, int *fact, double *scale, long *k0_applies, long *ks_applies);
/* the stage-2 layout that was built from the options (read-only; sets the layout up if no factorisation has yet):
 * out = {B0, B1, B2, number of bjacobi blocks, number of tiles, block-local tile-diagonals, most tiles in one launch,
 * launches per sweep direction}.  One tile per block (the default): B = the tile, blocks = tiles, 1, tiles, 1. */
int tp_ilu_layout(tp_ctx *ctx, int32_t out[8]);
/* device bytes of the stage-2 factor streams, forward plus backward, for the options in force (sets the layout up if no
 * factorisation has yet): the (tile, step) chunks the sweeps read, row padding included; halved by ilu_single */
int tp_ilu_factor_bytes(tp_ctx *ctx, int64_t *bytes);
int tp_amg_setup(tp_ctx *ctx, int32_t which);              /* v_cycle dict (singlephase.py:303-307); 0: pressure operator, 1: S~ */
/* which: 0 pressure hierarchy, 1 S~ hierarchy, 2 the (p,T) system hierarchy of pc_cptramg (fields 0,1 of b -> x) */
int tp_amg_vcycle(tp_ctx *ctx, int32_t which, int32_t field_b, int32_t b, int32_t field_x, int32_t x);
int tp_schur_apply(tp_ctx *ctx, int32_t x, int32_t y);     /* ConvDiffSchur*PC.apply: one V-cycle on S~, field 1 */

/* Inner solves (s1_ksp != 0) since the last tp_pc_setup: how many ran, the sum of the iterations they USED (the latch
 * iteration j* of each fgmres solve, s1_max_it per richardson solve), and how many fgmres solves ended at s1_max_it above
 * their tolerance (with s1_rtol = s1_atol = 0 that is every one).  The counters live on the device, are updated by the
 * inner solve's own kernels, and are copied out only by this call (one stream synchronisation).  All zero with preonly.
 * They count every preconditioner application that was LAUNCHED: the pipelined FGMRES loop issues the next application
 * before it knows whether the current iteration is the last, so a linear solve usually carries one application more
 * than it has iterations (tp_solve_info.vcycles is corrected for those on the host; device counters cannot be). */
int tp_inner_stats(tp_ctx *ctx, int64_t *applies, int64_t *its, int64_t *unconverged);

/* Krylov / Newton (PETSc KSP fgmres + SNES newtonls in the reference: twophase.py:416-433, singlephase.py:289-301;
 * reasons use PETSc's numbering so that the host raises ConvergenceError where Firedrake does, thermalmodel.py:170) */
int tp_fgmres(tp_ctx *ctx, int32_t b, int32_t x, int32_t *its, int32_t *reason, double *rnorm);
/* Right-preconditioned BiCGStab from x0 = 0 with the same preconditioner and operator (ksp_type fbcgs); mirrors tp_fgmres and
 * runs whatever tp_options.ksp_kind says.  its counts BiCGStab iterations (two preconditioner applications each); reason:
 * 2 converged (also b = 0, with 0 iterations), -3 ksp_max_it reached, -5 breakdown ((r^,r) = 0, (r^,v) = 0, or J M s = 0 for an
 * s above the tolerance), -9 NaN or Inf.  After -5 and -9 x holds the last iterate that was formed from finite numbers. */
int tp_bcgs(tp_ctx *ctx, int32_t b, int32_t x, int32_t *its, int32_t *reason, double *rnorm);
/* out = {ksp_kind in effect, device bytes of Krylov workspace currently allocated (the FGMRES bases V and Z -- under
 * ksp_basis_single the two fp32 bases and the fp64 staging vectors -- and the BiCGStab vectors; the scratch vectors every method shares with the preconditioner are not counted), number of BiCGStab work vectors
 * allocated (0 before the first BiCGStab solve), pc_apply programs recorded since the last set-up that invalidated them and
 * still replayable (a set-up that leaves addresses and options alone keeps them): 2 for a context that runs BiCGStab only} */
int tp_ksp_info(tp_ctx *ctx, int64_t out[4]);
/* The FGMRES bases under ksp_basis_single: out = {1 if the option is in effect else 0, capacity of each fp32 basis in vectors (0
 * before the first such solve), stride between two stored vectors in entries (b * owned cells rounded up to a multiple of 64),
 * fp64 staging vectors allocated (b * ntot doubles each), restart cycles of the last fp32-basis FGMRES solve, true-residual
 * evaluations (one SpMV and one norm each) of that solve}.  tp_ksp_info's bytes count these buffers too. */
int tp_ksp_basis_info(tp_ctx *ctx, int64_t out[6]);
/* Gram-Schmidt refinement (tp_options.ksp_reorth): out = {ksp_reorth in effect, orthogonalisation steps since tp_create (every
 * mode, tp_vec_orth_step included), second passes executed, second passes enqueued but skipped by the device flag}.  The last
 * two are counters on the device, written by the kernel that takes the decision and copied out only by this call (one stream
 * synchronisation); on several slabs every rank counts the same decisions. */
int tp_ksp_reorth_info(tp_ctx *ctx, int64_t out[4]);
int tp_newton_solve(tp_ctx *ctx, tp_solve_info *info);
/* The line search: out = {ls_kind in effect, device bytes of line-search workspace allocated (the saved iterate u0
 * only: the reductions use the scratch they share with the Krylov loop; 0 until the first bt solve), residual evaluations of the
 * last Newton solve's searches (= trials; the re-assembly at an accepted shortened step repeats the accepted trial's state and is
 * not counted), non-finite trials among them} */
int tp_ls_info(tp_ctx *ctx, int64_t out[4]);
/* Per Newton iteration of the last solve, at most cap entries: the accepted lambda, ||F|| after it and the trials spent; *n =
 * the number of iterations recorded (a failed search is not an iteration).  n = 0 after a basic solve. */
int tp_ls_history(tp_ctx *ctx, int32_t cap, double *lambda, double *fnorm, int32_t *trials, int32_t *n);
/* The two kernels of the search on their own, on tp_vec ids:
 *   tp_ls_step_stats  out = {||dx||_2^2, max|dx_p|, max|dx_T|, max|dx_S|} over owned cells, summed / maxed over the slabs
 *                     (single-phase: out[3] = 0)
 *   tp_ls_trial       out_vec = u0_vec - lambda dx_vec on owned cells of all fields; halo planes of out_vec are not written */
int tp_ls_step_stats(tp_ctx *ctx, int32_t dx, double out[4]);
int tp_ls_trial(tp_ctx *ctx, int32_t u0, int32_t dx, double lambda, int32_t out);

/* Eisenstat-Walker (tp_options.ksp_ew).  tp_ew_next_rtol is the chooser on its own: the tolerance of linear solve k of a Newton
 * solve from fnorm = ||F_k||, fnorm_last = ||F_{k-1}||, lresid_last = rho_{k-1} and rtol_last = eta_{k-1} (the last three are not
 * read for k = 0), with the parameters and ksp_rtol of *opt (opt->ksp_ew must be 1 or 2; ranges are checked).  It needs no context
 * and no GPU.
 * tp_ew_info: out = {version in effect (0: off), Newton solves run under it since tp_create, linear solves among them, linear
 * solves whose eta the safeguard raised}.
 * tp_ew_history: per linear solve of the last Newton solve, at most cap entries: eta_k, ||F_k||, rho_k, the Krylov iterations and
 * the KSP reason of solve k; *n = the number of solves recorded.  n = 0 after a solve with ksp_ew 0. */
int tp_ew_next_rtol(const tp_options *opt, int32_t k, double fnorm, double fnorm_last, double lresid_last, double rtol_last,
                    double *rtol);
int tp_ew_info(tp_ctx *ctx, int64_t out[4]);
int tp_ew_history(tp_ctx *ctx, int32_t cap, double *rtol, double *fnorm, double *lresid, int32_t *kits, int32_t *kreason,
                  int32_t *n);

/* measurement hooks for bench.py: average device time (ms, HIP events on the context's stream)
 * of `reps` launches of one hot kernel.  which: 0 block SpMV, 1 ILU solve, 2 AMG V-cycle (pressure),
 * 3 assembly (residual+Jacobian), 4 full pc_apply, 5 pc_setup, 6 ILU factorisation, 7 one classical Gram-Schmidt
 * step against 16 basis vectors (VecMDot + VecMAXPY + VecNorm; needs a Krylov basis from an earlier solve), 8 the same step
 * against 16 vectors of the fp32 basis (needs one from an earlier ksp_basis_single solve), 9 the stage-1 right-hand side of a later
 * S stage in one launch (tp_stage_rhs), 10 the pair of launches it replaces (block residual over all b rows and columns + the
 * decoupled right-hand side per primary field), 11 that block residual alone, 12 the T stage's row right-hand side in one launch
 * (tp_ctr_rhs; needs pc_ctr), 13 the boundary-face kernel alone (needs a side from tp_set_boundary; it adds to R, J and S~, so
 * assemble again before using them; 3 includes it when a side is set), 14 the wells' rank-1 kernel alone (needs tp_set_wells; it
 * adds to a scratch vector), 15 the well kernel alone (needs tp_set_wells; it adds to R, J and S~ like 13), 16 the source kernel's
 * rates-only form (needs tp_set_sources).  4 times the pc_order and pc_ctr in force. */
int tp_time_kernel(tp_ctx *ctx, int32_t which, int32_t reps, double *ms_avg);
int tp_amg_info(tp_ctx *ctx, int32_t which, int32_t *nlevels, double *op_complexity);
/* level at which hierarchy `which` ends with relaxation only (amg_dom_tau), -1: full V-cycle; ratio0 = the
 * dominance ratio measured on level 0 at the last set-up */
int tp_amg_trunc(tp_ctx *ctx, int32_t which, int32_t *level, double *ratio0);
/* coarsening axis of every level (internal axis numbering, 2 = slab axis) and how many of the top levels are
 * distributed over the slabs (0 on one GPU and when the hierarchy is replicated, see amg_gather_cells);
 * which: 0 pressure, 1 S~, 2 the (p,T) system hierarchy of pc_cptramg */
int tp_amg_layout(tp_ctx *ctx, int32_t which, int32_t *dist_levels, int32_t *axes, int32_t cap, int32_t *naxes);
/* the tail of hierarchy `which` (0 pressure, 1 S~), i.e. its levels of <= 1024 cells: out = {1 if the cycles since the last
 * set-up apply the tail as one precomputed dense operator (TP_AMG_TAIL_DENSE) else 0, first tail level, cells
 * of that level, dense operators formed, dense applications launched or captured, multilevel tail kernels launched or
 * captured} -- the last three counted since the hierarchy was built.  Like tp_amg_trunc this is a query of the RESOLVED state:
 * it waits for the last set-up's dominance ratios and may enqueue the forming of the dense operator, so it belongs neither in
 * a timed region nor in a stream capture */
int tp_amg_tail_info(tp_ctx *ctx, int32_t which, int64_t out[6]);
/* line relaxation of hierarchy `which` (0 pressure, 1 S~) as planned from amg_line_levels: out = {line levels in effect, lines
 * per workgroup on level 0 (0 if level 0 is no line level), n0 of level 0, device bytes of the factor streams of all line levels} */
int tp_amg_line_info(tp_ctx *ctx, int32_t which, int64_t out[4]);
/* red-black Gauss-Seidel of hierarchy `which` (0 pressure, 1 S~) as planned from amg_gs_levels / amg_gs_sweeps: out = {GS levels
 * in effect, sweeps per leg g, red cells of level 0, black cells of level 0}; all zero when the hierarchy has no GS level */
int tp_amg_gs_info(tp_ctx *ctx, int32_t which, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
