// Host orchestration of the hot path: PC set-up/apply, FGMRES, Newton.
//
//   pc_setup / pc_apply  = PCSetUp / PCApply of PCCOMPOSITE multiplicative("python,bjacobi")
//                          (singlephase.py:341-351, twophase.py:531-550,582-597) with the python stage
//                          being CPRStage1PC (preconditioners.py:335-906) or CPTRStage1PC (:1243-1571)
//   fgmres               = KSP fgmres, right PC, restart/max_it 200, classical Gram-Schmidt without
//                          refinement (twophase.py:426-432)
//   newton               = SNES newtonls with Firedrake's default `basic` line search
//                          (thermalmodel.py:36-42,165), or the opt-in backtracking search `bt` (tp_options.ls_kind); opt-in
//                          Eisenstat-Walker tolerances per linear solve (tp_options.ksp_ew, tp_ew.hpp)
// The loops live here (C++) rather than in Python so that one Krylov iteration costs kernel time,
// not interpreter time; the Python PC classes call the same stage functions through the C ABI.
#include "tp_common.hpp"
#include <cmath>
#include <algorithm>
#include <cstdlib>

namespace tp {

// ------------------------------------------------------------------------------------------------
void ensure_work(tp_ctx *c) {
    const size_t nv = (size_t)c->b * c->g.ntot;
    // w3 holds the Schur stage's r0, r1 and t: three planes even for the 2-field single-phase system.
    // Every buffer is tested on its own size: nothing may assume that whoever allocated w1 also sized w3.
    const size_t n3 = std::max(nv, (size_t)3 * c->g.ntot);
    bool grew = false;
    if (c->w1.n < nv) { c->w1.alloc(nv); grew = true; }
    if (c->w2.n < nv) { c->w2.alloc(nv); grew = true; }
    if (c->w3.n < n3) { c->w3.alloc(n3); grew = true; }
    if (c->w4.n < nv) { c->w4.alloc(nv); grew = true; }
    if (c->dx.n < nv) { c->dx.alloc(nv); grew = true; }
    if (grew) c->graph_epoch++;          // captured pc_apply graphs hold the old addresses
    inner_ensure(c);                     // s1_ksp != preonly: basis and scalars of the inner solve
}

// multi-GPU scratch on the gathered global grid: grown on demand, never shrunk; captured graphs hold the old address
static void ensure_global(tp_ctx *c, DBuf<double> &b, size_t n) {
    if (b.n >= n) return;
    b.alloc(n);
    c->graph_epoch++;
}

// mean interior-face transmissibility per axis over the GLOBAL grid (sum/count all-reduced over slabs)
static void face_strengths(tp_ctx *c, double st[3]) {
    const long nt = c->g.ntot;
    std::vector<double> h(nt);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const int n[3] = {c->g.n0, c->g.n1, c->g.n2};
    for (int a = 0; a < 3; ++a) {
        copy_sync(c, h.data(), c->TK[a].p, nt * sizeof(double), hipMemcpyDeviceToHost);
        for (int i2 = 0; i2 < n[2]; ++i2)
            for (int i1 = 0; i1 < n[1]; ++i1)
                for (int i0 = 0; i0 < n[0]; ++i0) {
                    const int idx[3] = {i0, i1, c->g.off2 + i2};
                    const int ext[3] = {n[0], n[1], c->g.gn2};
                    if (idx[a] >= ext[a] - 1) continue;
                    acc[a] += h[c->g.np * (i2 + 1) + (long)c->g.n0 * i1 + i0];
                    acc[3 + a] += 1.0;
                }
    }
    if (c->dist) {
        if (c->red_out.n < 6) c->red_out.alloc(64);
        TP_HIP(hipMemcpyAsync(c->red_out.p, acc, sizeof(acc), hipMemcpyHostToDevice, c->stream));
        allreduce_sum(c, c->red_out.p, 6);
        TP_HIP(hipMemcpyAsync(acc, c->red_out.p, sizeof(acc), hipMemcpyDeviceToHost, c->stream));
        TP_HIP(hipStreamSynchronize(c->stream));
    }
    for (int a = 0; a < 3; ++a) st[a] = acc[3 + a] > 0 ? acc[a] / acc[3 + a] : 0.0;
}

// the captured pc_apply graphs bake in buffer addresses and options: invalidate them when any changes
static void refresh_pc_signature(tp_ctx *c) {
    uint64_t scale_bits = 0;                       // (the scale is a kernel argument of the recorded diag sequence)
    if (c->opt.schur_fact == 3) memcpy(&scale_bits, &c->opt.schur_scale, sizeof scale_bits);
    const uintptr_t sig[] = {(uintptr_t)c->opA00.base, (uintptr_t)c->opA01.base, (uintptr_t)c->opA10.base,
                             (uintptr_t)c->Sm.p, (uintptr_t)c->ilu.fwd.p, (uintptr_t)c->ilu.fwd32.p, (uintptr_t)c->ilu.fwdp.p, (uintptr_t)c->amg_p, (uintptr_t)c->amg_T, (uintptr_t)c->bamg,
                             (uintptr_t)c->w1.p, (uintptr_t)c->w3.p, (uintptr_t)c->w4.p, (uintptr_t)c->dcoef.p, (uintptr_t)c->spbuf.p,
                             (uintptr_t)c->opt.amg_nu, (uintptr_t)c->opt.pc_kind, (uintptr_t)c->opt.pc_order, (uintptr_t)c->opt.decoup,
                             (uintptr_t)c->opt.amg_single, (uintptr_t)c->opt.amg_gather_cells, (uintptr_t)c->opt.schur_a11, (uintptr_t)c->opt.fs_additive, (uintptr_t)c->opt.amg_full_levels, (uintptr_t)c->opt.amg_coarse_pre, (uintptr_t)c->opt.amg_coarse_post, (uintptr_t)c->opt.amg_tail_post, (uintptr_t)c->opt.amg_mid_skip, (uintptr_t)c->opt.amg_line_levels, (uintptr_t)c->opt.amg_gs_levels, (uintptr_t)c->opt.amg_gs_sweeps,
                             (uintptr_t)c->opt.s1_ksp, (uintptr_t)c->opt.s1_max_it, (uintptr_t)c->inner.V.p, (uintptr_t)c->inner.Z.p,
                             (uintptr_t)c->ilu.ntiles, (uintptr_t)c->ilu.nsteps, (uintptr_t)c->ilu.whole,
                             (uintptr_t)c->amg_ctr, (uintptr_t)c->opt.pc_ctr,
                             (uintptr_t)c->opt.schur_fact, (uintptr_t)scale_bits};
    uintptr_t h = 1469598103934665603ull;
    for (uintptr_t v : sig) h = (h ^ v) * 1099511628211ull;
    if (h != c->pc_sig) { c->pc_sig = h; c->graph_epoch++; }
}

// several GPUs, hierarchy replicated from the top: stage 1 works on the system gathered on the global grid of every rank
static bool replicated(const tp_ctx *c, const AmgPlan &plan) { return c->dist && plan.dist_levels == 0; }
static bool stage1_replicated(const tp_ctx *c) { return c->dist && replicated(c, sysamg_of(c->opt) ? c->bamg->plan : c->amg_p->plan); }
// the grid the stage-1 hierarchies are built on: the GLOBAL grid (one GPU: the slab is the whole grid)
static GridDev hierarchy_grid(const tp_ctx *c) { return c->dist ? c->gfull : make_grid(c->g.n0, c->g.n1, c->g.n2, c->g.n2, 0); }

// the inner solve's dot products are local: on several GPUs every rank must hold the whole stage-1 system
static void require_replicated_for_inner(tp_ctx *c, const AmgPlan &plan) {
    if (c->opt.s1_ksp == 0 || !c->dist) return;
    TP_REQUIRE(plan.dist_levels == 0, "s1_ksp richardson/fgmres on several GPUs needs the replicated stage-1 hierarchy: with "
               "slab-distributed top levels the inner dot products would need all-reduces between graph segments.  Set "
               "amg_gather_cells < 0 (replicate the whole hierarchy) or s1_ksp preonly");
}

// pc_cptramg[_QI|_TI] (twophase.py:552-566): CPTRStage1PC.update with ONE system-AMG V-cycle as stage-1 solver
static void pc_setup_sysamg(tp_ctx *c) {
    TP_REQUIRE(c->b == 3, "pc_cptramg is a two-phase preconditioner");
    TP_REQUIRE(c->opt.decoup >= 0 && c->opt.decoup <= 2, "pc_cptramg: decoupling No, QI or TI");
    decouple(c);
    const GridDev gam = hierarchy_grid(c);
    if (!c->bamg) {
        double st[3];
        face_strengths(c, st);             // the pressure's coarsening schedule
        bamg_build(c, c->bamg, gam, st);
    }
    require_replicated_for_inner(c, c->bamg->plan);
    const long nt = c->g.ntot;
    BStencil A0;
    if (c->opt.decoup == 0) { A0.base = c->J.p; A0.ss = (long)c->b * c->b * nt; A0.rs = (long)c->b * nt; A0.cs = nt; }
    else { A0.base = c->At.p; A0.ss = 4 * nt; A0.rs = 2 * nt; A0.cs = nt; }
    if (replicated(c, c->bamg->plan)) {
        // small grids: the hierarchy lives on the gathered global grid, replicated on every rank (as small scalar hierarchies
        // do); larger ones keep their top levels on the slabs (tp_amg_block.hip) and work on the slab operator directly
        const size_t ng = (size_t)c->gfull.ntot;
        ensure_global(c, c->gAt, 28 * ng);
        ensure_global(c, c->gvec, 6 * ng);      // (sized for every pc kind: switching kinds never shrinks it)
        for (int s = 0; s < 7; ++s)
            for (int q = 0; q < 2; ++q)       // the two column planes of a block row are nt apart on both sides
                gather_slabs(c, A0.at(s, q, 0), A0.cs, c->gAt.p + ((size_t)(s * 2 + q) * 2) * ng, (long)ng, 2);
        A0.base = c->gAt.p; A0.ss = 4 * (long)ng; A0.rs = 2 * (long)ng; A0.cs = (long)ng;
    }
    c->opPT = A0;
    bamg_setup(c, c->bamg, A0);
    ilu_factor(c);
    c->pc_ready = true;
    refresh_pc_signature(c);
}

void pc_setup(tp_ctx *c) {
    TP_REQUIRE(c->jac_ready, "pc_setup needs an assembled Jacobian");
    ensure_work(c);
    c->schur_k0 = c->schur_ks = 0;                 // tp_schur_info counts since the last set-up
    TP_REQUIRE(!(c->opt.pc_ctr && c->dist), "pc_ctr on a context with a communicator (slabs / ranks): the temperature stage is "
               "implemented for one GPU without one");
    if (c->opt.s1_ksp) inner_reset_stats(c);      // tp_inner_stats counts since the last set-up
    if (c->ilu.slots == 0) ilu_setup(c);          // (a stage-2 layout the options do not allow fails here, before the streams fork)
    if (c->opt.pc_kind == 4) {               // pc_bilu (twophase.py:758-762): bjacobi + ILU is the whole preconditioner
        ilu_factor(c);
        c->pc_ready = true;
        refresh_pc_signature(c);
        return;
    }
    if (sysamg_of(c->opt)) { pc_setup_sysamg(c); return; }
    const bool cptr = schur_of(c->opt);       // fieldsplit-Schur stage on (p,T): pc_cptr and pc_fieldsplit_cd
    if (c->opt.pc_kind == 1) TP_REQUIRE(c->b == 3, "pc_cptr is a two-phase preconditioner");
    if (c->opt.pc_kind == 2) {
        TP_REQUIRE(c->b == 2, "pc_fieldsplit_cd is a single-phase preconditioner (singlephase.py:309-319)");
        TP_REQUIRE(c->opt.decoup == 0, "pc_fieldsplit_cd has no decoupling stage");
    }
    // stage 1: decoupling + AMG hierarchies (CPRStage1PC.update / CPTRStage1PC.update)
    decouple(c);
    // single GPU: the AMG works on the slab (= whole grid).  Multi-GPU: the hierarchy is that of the GLOBAL grid,
    // so the preconditioner (and the iteration counts) are those of the single-GPU run and only stage 2 is
    // bjacobi.  Grids above amg_gather_cells keep their top levels distributed over the slabs (tp_amg.hip);
    // smaller ones are replicated from the top: every rank gathers the scalar stage-1 operators.
    const GridDev gam = hierarchy_grid(c);
    // selfp on several GPUs works on slab vectors (its exact-Sp sweep needs the slab's own Jacobian rows): the hierarchies
    // keep every level with >= 2 planes per rank distributed, whatever amg_gather_cells says
    const long gather_cells = (c->dist && cptr && c->opt.schur_a11 == 2) ? 0 : (long)c->opt.amg_gather_cells;
    if (!c->amg_p) {
        double st[3];
        face_strengths(c, st);         // coarsening schedule decided once; structure is static
        amg_build(c, c->amg_p, gam, st, gather_cells);
        if (cptr) {
            double sg[3];
            conduction_strengths(c, gam, sg);
            amg_build(c, c->amg_T, gam, sg, gather_cells);
            TP_REQUIRE((c->amg_p->plan.dist_levels > 0) == (c->amg_T->plan.dist_levels > 0), "stage-1 hierarchies disagree on distribution");
        }
    }
    // pc_ctr: the hierarchy of the T stage, coarsened by the conduction strengths of amg_T and set up on the T-T planes of the
    // UNDECOUPLED Jacobian: the stage takes its sub-matrix from the composite's operator, not from the decoupled copy
    const bool ctr = c->opt.pc_ctr != 0;
    Stencil Sc;
    if (ctr) {
        if (!c->amg_ctr) {
            double sg[3];
            conduction_strengths(c, gam, sg);
            amg_build(c, c->amg_ctr, gam, sg, gather_cells);
        }
        Sc.base = c->J.p + (long)(c->b + 1) * c->g.ntot;
        Sc.slot_stride = (long)c->b * c->b * c->g.ntot;
        ++c->ctr_setups;
    }
    require_replicated_for_inner(c, c->amg_p->plan);
    Stencil Sl;
    Sl.base = c->Sm.p;
    Sl.slot_stride = c->g.ntot;
    if (c->opt.fs_additive) TP_REQUIRE(c->opt.pc_kind == 2 && c->opt.schur_a11 != 2, "fs_additive is the single-phase pc_fieldsplit_diag preset");
    const bool selfp = cptr && c->opt.schur_a11 == 2;
    if (selfp) {
        // pc_fieldsplit_schur_precondition selfp (pc_fieldsplit_selfp, singlephase.py:322-330)
        TP_REQUIRE(c->opt.pc_kind == 2, "selfp is the single-phase pc_fieldsplit_selfp preset's Schur preconditioner");
        TP_REQUIRE(!c->dist || c->amg_p->plan.dist_levels > 0, "selfp on several GPUs needs slabs of at least two planes (its Schur "
                   "sweep works on slab vectors; the replicated global-grid stage 1 has no exact-Sp sweep)");
        if (c->spbuf.n < (size_t)10 * c->g.ntot) c->spbuf.alloc((size_t)10 * c->g.ntot);
        Sl.base = c->spbuf.p;                  // S7, filled by selfp_build on the stream of the S set-up below
        Sl.slot_stride = c->g.ntot;
    } else if (cptr && (c->opt.schur_a11 || c->opt.fs_additive)) {
        // pc_fieldsplit_schur_precondition a11 (singlephase.py:331-338, twophase.py:598-616): the T-T block of the
        // (decoupled) primary system stands in for the Schur complement
        Sl.base = c->opA00.base + 3 * (c->opA01.base - c->opA00.base);     // block (1,1) = 3 planes after (0,0)
        Sl.slot_stride = c->opA00.slot_stride;
        if (c->opt.decoup == 0) Sl.base = c->J.p + (long)(c->b + 1) * c->g.ntot;
    }
    if (cptr && !selfp) TP_REQUIRE(Sl.base, "pc_cptr needs the S~ operator (assemble with want_schur)");
    if (replicated(c, c->amg_p->plan)) {
        const size_t ng = (size_t)c->gfull.ntot;
        // every buffer is tested on its own size (an options switch cpr -> cptr, or cptr -> cptramg -> cptr, on a live
        // context must not find gvec shrunk or gA01/gA10/gSm missing because some OTHER buffer was already large enough)
        ensure_global(c, c->gA00, 7 * ng);
        if (cptr) { ensure_global(c, c->gA01, 7 * ng); ensure_global(c, c->gA10, 7 * ng); ensure_global(c, c->gSm, 7 * ng); }
        ensure_global(c, c->gvec, 6 * ng);
        gather_slabs(c, c->opA00.base, c->opA00.slot_stride, c->gA00.p, (long)ng, 7);
        Stencil G;
        G.slot_stride = (long)ng;
        G.base = c->gA00.p;
        amg_setup(c, c->amg_p, G);
        if (cptr) {
            gather_slabs(c, c->opA01.base, c->opA01.slot_stride, c->gA01.p, (long)ng, 7);
            gather_slabs(c, c->opA10.base, c->opA10.slot_stride, c->gA10.p, (long)ng, 7);
            gather_slabs(c, Sl.base, Sl.slot_stride, c->gSm.p, (long)ng, 7);
            G.base = c->gSm.p;
            amg_setup(c, c->amg_T, G);
        }
    } else if (c->dist) {
        amg_setup(c, c->amg_p, c->opA00);
        if (selfp) {
            // Sp of a boundary cell reads diag(A00) and the A01 row of its neighbour across the slab boundary: the Jacobian's
            // halo rows (singlephase.py:322-330 lets PETSc form Sp from the assembled parallel matrix)
            halo_exchange(c, c->g, c->J.p, 7 * c->b * c->b, c->g.ntot);
            selfp_build(c);
        }
        if (cptr) amg_setup(c, c->amg_T, Sl);
    } else {
        // one GPU: the AMG set-ups (2 x ~35 launch-latency-bound kernels) and the ILU factorisation are
        // independent -> three concurrent streams, joined before anything uses the preconditioner.
        // (not with RCCL in the set-up: one communicator must not be driven from two streams at once)
        hipStream_t main = c->stream;
        struct Restore { tp_ctx *c; hipStream_t s; ~Restore() { c->stream = s; } } restore{c, main};   // also on a throw
        TP_HIP(hipEventRecord(c->ev_fork, main));
        TP_HIP(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
        c->stream = c->aux[0];
        amg_setup(c, c->amg_p, c->opA00);
        TP_HIP(hipEventRecord(c->ev_join[0], c->aux[0]));
        if (cptr || ctr) {
            TP_HIP(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0));
            c->stream = c->aux[1];
            if (selfp) selfp_build(c);
            if (cptr) amg_setup(c, c->amg_T, Sl);
            if (ctr) amg_setup(c, c->amg_ctr, Sc);              // (behind amg_T on its stream: both are short chains)
            TP_HIP(hipEventRecord(c->ev_join[1], c->aux[1]));
        }
        c->stream = main;
        ilu_factor(c);
        TP_HIP(hipStreamWaitEvent(main, c->ev_join[0], 0));
        if (cptr || ctr) TP_HIP(hipStreamWaitEvent(main, c->ev_join[1], 0));
        c->pc_ready = true;
    }
    // stage 2: numeric block-ILU(0) of every tile of this rank's slab
    if (c->dist) ilu_factor(c);
    c->pc_ready = true;
    refresh_pc_signature(c);
}

// the relaxation-only truncation level of each hierarchy is known once its set-up kernels have run
void resolve_cycle_shapes(tp_ctx *c) {
    bool changed = amg_resolve_trunc(c, c->amg_p);
    changed = amg_resolve_trunc(c, c->amg_T) || changed;
    if (c->opt.pc_ctr) changed = amg_resolve_trunc(c, c->amg_ctr) || changed;
    if (changed) c->graph_epoch++;
}

// The system one stage-1 application runs on: this rank's slab, or (several GPUs, replicated hierarchy) the system gathered
// on the global grid of every rank.
struct Stage1Sys {
    GridDev g;
    Stencil A00, A01, A10;
    bool exchange;         // vectors need a halo exchange between the steps: slab vectors of a distributed context only
};
static Stage1Sys stage1_system(const tp_ctx *c, bool gathered) {
    if (!gathered) return {c->g, c->opA00, c->opA01, c->opA10, c->dist};
    const long ng = c->gfull.ntot;
    return {c->gfull, {c->gA00.p, ng}, {c->gA01.p, ng}, {c->gA10.p, ng}, false};
}

// ---- the factorisation of the Schur split (tp_options.schur_fact, schur_scale) ---------------------------
void pc_schur_fact_check_options(const tp_options &o) {
    TP_REQUIRE(o.schur_fact >= 0 && o.schur_fact <= 3, "schur_fact must be 0 (full), 1 (lower), 2 (upper) or 3 (diag)");
    TP_REQUIRE(std::isfinite(o.schur_scale), "schur_scale must be finite");
    if (o.schur_fact != 3)      // (0: a zeroed field of a C caller)
        TP_REQUIRE(o.schur_scale == -1.0 || o.schur_scale == 0.0, "schur_scale other than -1 with schur_fact other than 3 (diag): the "
                   "scale belongs to the diag factorisation");
    if (!o.schur_fact) return;
    TP_REQUIRE(o.pc_kind != 0, "schur_fact other than 0 (full) with pc_kind 0 (pc_cpr): one V-cycle on the pressure block, no Schur split");
    TP_REQUIRE(o.pc_kind != 3, "schur_fact other than 0 (full) with pc_kind 3 (pc_cptramg): one system V-cycle, no Schur split");
    TP_REQUIRE(o.pc_kind != 4, "schur_fact other than 0 (full) with pc_kind 4 (pc_bilu): bjacobi + ILU alone, no Schur split");
    TP_REQUIRE(!o.fs_additive, "schur_fact other than 0 (full) with fs_additive (pc_fieldsplit_diag): PETSc's additive split is no "
               "Schur factorisation");
}

// tp_schur_info: `stages` stage-1 sequences are about to be issued or replayed
void schur_count(tp_ctx *c, int stages) {
    const tp_options &o = c->opt;
    if (o.pc_kind == 3 || o.pc_kind == 4) return;
    const bool split = npri_of(o) == 2;
    c->schur_k0 += (long)stages * (split && !o.fs_additive && o.schur_fact == 0 ? 2 : 1);
    c->schur_ks += split ? stages : 0;
}

// y = K r on system `s`; t and w are two work vectors of the system's grid.  npri == 1: y0 = K(A00) r0.  Else
// PCFIELDSPLIT additive (pc_fieldsplit_diag, singlephase.py:371-375) or schur on (p,T) (twophase.py:536-545) in the
// factorisation of schur_fact: K(A00), K(S~) = one V-cycle each (slab-distributed AMG levels: the V-cycles return owned cells,
// the couplings read halos).  Nothing writes r0 or r1 (decoupling "No" on one GPU: they are the caller's x).
static void stage1_sequence(tp_ctx *c, const Stage1Sys &s, const double *r0, const double *r1, double *y0, double *y1,
                            double *t, double *w) {
    // K(A00): one V-cycle of the pressure hierarchy, or (s1_ksp) an inner solve preconditioned by it
    InnerOp op;
    op.g = s.g;
    op.A[0][0] = s.A00;
    const auto K00 = [&](const double *b, double *xx) { inner_solve(c, op, [&](const double *bb, double *xo) { amg_vcycle(c, c->amg_p, bb, xo); }, b, xx, 1); };
    if (npri_of(c->opt) == 1) { K00(r0, y0); return; }
    if (c->opt.fs_additive) {              // one V-cycle per field
        K00(r0, y0);
        amg_vcycle(c, c->amg_T, r1, y1);
        return;
    }
    const long n = s.g.ntot;
    // K(S): one V-cycle on S~ / A11, or (selfp; slab system only: pc_setup) V7 then one Jacobi sweep on the exact Sp
    const auto KS = [&](const double *b) {
        if (c->opt.schur_a11 == 2) {
            double *xv = c->spbuf.p + 9 * c->g.ntot;
            amg_vcycle(c, c->amg_T, b, xv);
            selfp_post(c, b, xv, y1);
        } else {
            amg_vcycle(c, c->amg_T, b, y1);                                 // y1 = K(S~) b
        }
    };
    const int fact = c->opt.schur_fact;
    if (fact == 3) {                       // diag: no coupling, no exchange; y1 scaled in place by an existing vector kernel
        K00(r0, y0);
        KS(r1);
        scale_plane(c, s.g, c->opt.schur_scale, y1);
        return;
    }
    if (fact == 1) {                       // lower: K(A00)'s result is y0 itself; the exchange in front of A10 is y0's
        K00(r0, y0);
        if (s.exchange) halo_exchange(c, s.g, y0, 1, n);
        spmv_scalar(c, s.g, s.A10, y0, t, -1.0, r1);                        // t = r1 - A10 y0
        KS(t);
        return;
    }
    if (fact == 2) {                       // upper
        KS(r1);
    } else {                               // full (the launch sequence of every build before schur_fact)
        K00(r0, w);                                                         // w = K(A00) r0
        if (s.exchange) halo_exchange(c, s.g, w, 1, n);
        spmv_scalar(c, s.g, s.A10, w, t, -1.0, r1);                         // t = r1 - A10 w
        KS(t);
    }
    if (s.exchange) halo_exchange(c, s.g, y1, 1, n);
    spmv_scalar(c, s.g, s.A01, y1, t, -1.0, r0);                            // t = r0 - A01 y1
    K00(t, y0);                                                             // y0 = K(A00) t
}

static void stage1_run(tp_ctx *c, const double *r0, const double *r1, double *y);

// y = B1 x :  CPRStage1PC.apply (preconditioners.py:881-903) / CPTRStage1PC.apply (:1550-1567)
void stage1_apply(tp_ctx *c, const double *x, double *y, bool zero_secondary) {
    const long nt = c->g.ntot;
    ensure_work(c);
    resolve_cycle_shapes(c);
    const double *r0 = c->w3.p, *r1 = c->w3.p + nt;                         // w3 has >= 3 planes
    // y_s = 0 for the non-primary fields (:902-903, :1566-1567)
    const int npri = npri_of(c->opt);
    if (zero_secondary)
        for (int f = npri; f < c->b; ++f) vec_zero(c, y + (long)f * nt, nt);
    if (c->opt.decoup == 0 && !c->dist) {
        // decoupling "No" (pc_cptr, pc_cpr, pc_fieldsplit_cd presets): the stage-1 right-hand sides ARE the
        // primary fields of x -- no copy (multi-GPU keeps the copy: the V-cycle's exchange writes b's halos)
        r0 = x;
        r1 = x + nt;
    } else {
        stage1_rhs(c, x, 0, c->w3.p);              // r_p = x_p - (D_ps D_ss^-1) x_s
        if (npri == 2) stage1_rhs(c, x, 1, c->w3.p + nt);
    }
    stage1_run(c, r0, r1, y);
}

// the stage-1 solver on prepared right-hand sides r0 (, r1): y_0 (, y_1) = K r; y holds npri planes of the slab.  Scratch: the third
// plane of w3, w4 and (replicated hierarchy on several GPUs) gvec -- r and y may be anything else, the first two planes of w3 included
static void stage1_run(tp_ctx *c, const double *r0, const double *r1, double *y) {
    const long nt = c->g.ntot;
    const int npri = npri_of(c->opt);
    // the system and its vectors: slab vectors, or the planes of gvec on the gathered global grid
    const bool gathered = stage1_replicated(c);
    const Stage1Sys s = stage1_system(c, gathered);
    double *y0 = y, *y1 = y + nt, *t = c->w3.p + 2 * nt, *w = c->w4.p;
    if (gathered) {
        const long ng = s.g.ntot;
        double *gv = c->gvec.p;
        gather_slabs(c, r0, nt, gv, ng, npri);     // r0 (and r1: consecutive planes on both sides)
        r0 = gv; r1 = gv + ng; y0 = gv + 2 * ng; y1 = gv + 3 * ng; t = gv + 4 * ng; w = gv + 5 * ng;
    }
    if (sysamg_of(c->opt)) {
        // pc_cptramg: y_pT = K(Atilde_00) r_pT, one V-cycle of the 2x2-block system AMG (r0, r1 and y0, y1 are adjacent
        // planes), or (s1_ksp) an inner solve preconditioned by it
        InnerOp op;
        op.g = s.g;
        for (int q = 0; q < 2; ++q)
            for (int r = 0; r < 2; ++r) { op.A[q][r].base = c->opPT.at(0, q, r); op.A[q][r].slot_stride = c->opPT.ss; }
        inner_solve(c, op, [&](const double *bb, double *xo) { bamg_vcycle(c, c->bamg, bb, xo); }, r0, y0, 2);
    } else {
        stage1_sequence(c, s, r0, r1, y0, y1, t, w);
    }
    if (gathered) {
        // my slab of the result INCLUDING its halo planes (global planes lo-1 .. hi), so y needs no exchange
        const long off = c->g.np * c->grid.off2;
        vec_copy(c, y0 + off, y, nt);
        if (npri == 2) vec_copy(c, y1 + off, y + nt, nt);
    }
}

// ---- the composite's stage orders (tp_options.pc_order) ------------------------------------------------
void pc_order_check_options(const tp_options &o) {
    TP_REQUIRE(o.pc_order >= 0 && o.pc_order <= 3, "pc_order must be 0 (SI), 1 (IS), 2 (ISI) or 3 (SIS)");
    if (!o.pc_order) return;
    TP_REQUIRE(o.pc_kind != 2, "pc_order other than 0 (SI) with pc_kind 2 (pc_fieldsplit_cd): that preconditioner has no second stage to order");
    TP_REQUIRE(o.pc_kind != 4, "pc_order other than 0 (SI) with pc_kind 4 (pc_bilu): that preconditioner has no first stage to order");
}

// A later S stage: y_q += [B_S (x - J y)]_q on the primary fields q; y's secondary fields stay as they are.
// Invariants (every supported order puts an I stage right before a later S stage):
//  - the residual behind the right-hand side reads ALL b columns of y.  That is correct only because the I stage before wrote
//    every field of y (ilu_solve writes all b fields, whatever nadd says about what it reads);
//  - that I stage wrote owned cells only: on several slabs all b fields of y need live halo planes first;
//  - scratch: the right-hand sides go to the first npri planes of w3 (where the decoupled first stage keeps them), stage1_run
//    works in w3's third plane, w4 and gvec, and the stage's result e lands in the first npri planes of w1 -- free here, the
//    residual the I stage solved for is dead once ilu_solve has returned.  None of them is x or y;
//  - the accumulation covers owned cells: y's primary halo planes are stale afterwards (pc_stage_I_full exchanges them).
static void pc_stage_S_later(tp_ctx *c, const double *x, double *y) {
    const long nt = c->g.ntot;
    const int npri = npri_of(c->opt);
    if (c->dist) halo_exchange(c, c->g, y, c->b, nt);
    stage_rhs(c, x, y, c->w3.p);                            // one launch: only the Jacobian rows stage 1 needs
    stage1_run(c, c->w3.p, c->w3.p + nt, c->w1.p);
    vec_axpy_owned(c, npri, 1.0, c->w1.p, y);               // y_q += e_q
}
// A later I stage behind a later S stage (ISI): y += B_I (x - J y) with all b columns of y -- every field is nonzero by now.
// Several slabs: the S stage before changed the owned cells of the primary fields; the secondary halo planes are still those of
// the exchange in front of that S stage.  w1 (the S stage's result, already added) is free again for the residual.
static void pc_stage_I_full(tp_ctx *c, const double *x, double *y) {
    if (c->dist) halo_exchange(c, c->g, y, npri_of(c->opt), c->g.ntot);
    resid_block_cols(c, c->J.p, x, y, c->b, c->w1.p);
    ilu_solve(c, c->w1.p, y, y, c->b);                      // y = y + M^-1 r, all fields of y read
}

// ---- the composite's temperature stage (tp_options.pc_ctr) ------------------------------------------------
void pc_ctr_check_options(const tp_options &o, int nranks) {
    TP_REQUIRE(o.pc_ctr == 0 || o.pc_ctr == 1, "pc_ctr must be 0 or 1");
    if (!o.pc_ctr) return;
    TP_REQUIRE(o.pc_kind != 2, "pc_ctr with pc_kind 2 (pc_fieldsplit_cd): that preconditioner is no composite to append a stage to");
    TP_REQUIRE(o.pc_kind != 3, "pc_ctr with pc_kind 3 (pc_cptramg): the temperature stage is implemented behind pc_cpr and pc_cptr");
    TP_REQUIRE(o.pc_kind != 4, "pc_ctr with pc_kind 4 (pc_bilu): that preconditioner is no composite to append a stage to");
    TP_REQUIRE(nranks <= 1, "pc_ctr with nranks > 1: the temperature stage is implemented for one slab");
}

// y_1 = V(A_TT) x_1, every other field of y zero: CTRStage1PC.apply
void ctr_apply(tp_ctx *c, const double *x, double *y) {
    const long nt = c->g.ntot;
    resolve_cycle_shapes(c);
    ++c->ctr_applies;
    vec_zero(c, y, (long)c->b * nt);
    amg_vcycle(c, c->amg_ctr, x + nt, y + nt);
}

// The T stage, last in every sequence (SIT, IST, ISIT, SIST): y_1 += V(A_TT) [x - J y]_1; every other field of y stays.
// Invariants:
//  - the row residual reads ALL b columns of y.  SI and ISI end with an I stage, which wrote every field of y; IS and SIS end
//    with a later S stage, which added into the primary fields and left the secondary ones as the I stage before it wrote them.
//    So all b columns are live in all four;
//  - one slab only (pc_ctr_check_options, pc_setup): no halo exchange, and the halo planes of y that the kernel reads through
//    its boundary cells meet zero Jacobian coefficients, as in every other residual of this file;
//  - scratch: the right-hand side goes to the first plane of w3, the cycle's result e to the first plane of w1.  Both are dead at
//    this point in all four sequences: w3 held the right-hand sides of an S stage whose stage1_run has returned (SI, SIS, IS) or
//    that lies two stages back (ISI); w1 held the residual of an I stage whose ilu_solve has returned (SI, ISI) or the result of a
//    later S stage that vec_axpy_owned has already added (IS, SIS).  w4 is not used.  None of them is x or y;
//  - the V-cycle works in the hierarchy's own level vectors; the accumulation covers owned cells.
static void pc_stage_T(tp_ctx *c, const double *x, double *y) {
    const long nt = c->g.ntot;
    row_rhs(c, x, y, c->w3.p);                              // one launch: only row 1 of the Jacobian
    amg_vcycle(c, c->amg_ctr, c->w3.p, c->w1.p);
    vec_axpy_owned(c, 1, 1.0, c->w1.p, y + nt);             // y_T += e
}

static void pc_apply_stages(tp_ctx *c, const double *x, double *y);

// composite multiplicative: the stages of pc_order, then (pc_ctr) the temperature stage
static void pc_apply_body(tp_ctx *c, const double *x, double *y) {
    pc_apply_stages(c, x, y);
    if (c->opt.pc_ctr) pc_stage_T(c, x, y);
}

// composite multiplicative: y = B1 x ; r = x - J y ; y += B2 r  (pc_order 0 = SI; 1..3: the same two stages as IS, ISI, SIS)
static void pc_apply_stages(tp_ctx *c, const double *x, double *y) {
    if (c->opt.pc_kind == 4) { ilu_solve(c, x, y, nullptr, 0); return; }
    const int npri = npri_of(c->opt);
    if (c->opt.pc_order == 1 || c->opt.pc_order == 2) {      // IS, ISI
        ilu_solve(c, x, y, nullptr, 0);                      // y = B_I x: every field of y written, nothing of it read
        pc_stage_S_later(c, x, y);
        if (c->opt.pc_order == 2) pc_stage_I_full(c, x, y);
        return;
    }
    // (y's secondary fields are left untouched: the second stage below never reads them and overwrites them)
    stage1_apply(c, x, y, false);                 // multi-GPU, replicated stage 1: y comes back with live halo planes
    if (c->dist && !stage1_replicated(c)) halo_exchange(c, c->g, y, npri, c->g.ntot);       // (slab-distributed hierarchies return owned cells only)
    if (c->opt.pc_kind == 2) return;                          // pc_fieldsplit_cd: the Schur stage IS the preconditioner
    resid_block_cols(c, c->J.p, x, y, npri, c->w1.p);        // secondary fields of y are zero
    ilu_solve(c, c->w1.p, y, y, npri);                       // y = y + M^-1 r  (y's secondary fields are zero: not read)
    // SIS: "y's secondary fields are never read" held while S was first only; the I stage above has now written every field
    if (c->opt.pc_order == 3) pc_stage_S_later(c, x, y);
}

// ---- recording of pc_apply programs: one capture segment between two exchanges ------------------------------------------
// TP_DEBUG=2: one line per HIP graph call (used to locate the profiler crash described in DESIGN.md 6)
static void pc_trace(const tp_ctx::PcProgram &pr, const char *what) {
    static const bool trace = tp_switch_int(TP_SW_DEBUG) >= 2;
    if (trace) { fprintf(stderr, "[tp] pc_apply(%p,%p): %s\n", (const void *)pr.x, (void *)pr.y, what); fflush(stderr); }
}
void seg_begin(tp_ctx *c) {
    pc_trace(*c->rec, "begin capture");
    TP_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->rec_capturing = true;
}
// closes the segment; a non-empty one is instantiated, appended to the program and LAUNCHED (a capture executes nothing: the
// recording pass must still produce the result, and the exchange that follows reads what these kernels wrote)
void seg_end(tp_ctx *c) {
    hipGraph_t graph = nullptr;
    pc_trace(*c->rec, "end capture");
    c->rec_capturing = false;
    TP_HIP(hipStreamEndCapture(c->stream, &graph));
    size_t nnodes = 0;
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphGetNodes(graph, nullptr, &nnodes);
    if (e == hipSuccess && nnodes > 0) {
        pc_trace(*c->rec, "instantiate");
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    }
    (void)hipGraphDestroy(graph);
    TP_HIP(e);
    if (!exec) return;
    c->rec->steps.push_back({GraphExec(exec), nullptr});
    pc_trace(*c->rec, "launch");
    TP_HIP(hipGraphLaunch(exec, c->stream));
    pc_trace(*c->rec, "launched");
}

// One preconditioner application is ~100 short kernels (the V-cycles' coarse levels); issued eagerly
// the host launch path (~3 us per kernel) is slower than the GPU executes them.  The whole sequence
// is therefore recorded once per (input, output) address pair -- FGMRES uses the fixed pairs (V_j, Z_j) --
// as a program (tp_common.hpp) and replayed per Krylov iteration: on one slab a single hipGraph, on several
// slabs graph segments between the exchanges with the exchanges themselves as host closures.
void pc_apply(tp_ctx *c, const double *x, double *y) {
    TP_REQUIRE(c->pc_ready, "pc_apply before pc_setup");
    static const bool use_graph = tp_switch_flag(TP_SW_GRAPH);
    c->vcycles += vcycles_per_apply(c);
    if (c->opt.pc_ctr) ++c->ctr_applies;
    schur_count(c, c->opt.pc_order == 3 ? 2 : 1);
    ensure_work(c);                      // never allocate inside a stream capture
    resolve_cycle_shapes(c);             // (waits for the last set-up's dominance ratios: not inside a capture either)
    if (!use_graph) {
        pc_apply_body(c, x, y);
        return;
    }
    if (c->pc_graph_epoch != c->graph_epoch || c->pc_programs.size() > 512) {      // stale (or runaway) cache
        c->pc_programs.clear();
        c->pc_graph_epoch = c->graph_epoch;
    }
    for (auto &pr : c->pc_programs)
        if (pr.x == x && pr.y == y) {
            for (auto &st : pr.steps) {
                if (!st.exec.h) { st.comm(); continue; }
                pc_trace(pr, "launch");
                TP_HIP(hipGraphLaunch(st.exec.h, c->stream));
                pc_trace(pr, "launched");
            }
            return;
        }
    c->pc_programs.push_back({x, y, {}});
    c->rec = &c->pc_programs.back();
    try {
        seg_begin(c);
        pc_apply_body(c, x, y);
        seg_end(c);
    } catch (...) {
        if (c->rec_capturing) {              // a dangling capture: end it, so that the stream is usable again
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(c->stream, &g);
            if (g) (void)hipGraphDestroy(g);
        }
        c->rec_capturing = c->rec_in_comm = false;
        c->rec = nullptr;
        c->pc_programs.pop_back();           // (destroys the segments recorded so far)
        throw;
    }
    c->rec = nullptr;
}

// ------------------------------------------------------------------------------------------------
// FGMRES's options.  The bases stored in fp32 (tp_options.ksp_basis_single; compressed-basis GMRES)
void basis_single_check_options(const tp_options &o) {
    if (!o.ksp_basis_single) return;
    TP_REQUIRE(o.ksp_kind == 0, "ksp_basis_single with ksp_kind 1 (bcgs): BiCGStab has no basis to store in fp32");
    TP_REQUIRE(o.ksp_single_floor > 0x1p-24 && o.ksp_single_floor < 1.0, "ksp_single_floor must lie in (2^-24, 1)");
}
// Gram-Schmidt refinement of the fp64-basis FGMRES (tp_options.ksp_reorth)
void reorth_check_options(const tp_options &o) {
    TP_REQUIRE(o.ksp_reorth >= 0 && o.ksp_reorth <= 2, "ksp_reorth must be 0 (never), 1 (if needed) or 2 (always)");
    if (!o.ksp_reorth) return;
    TP_REQUIRE(o.ksp_kind == 0, "ksp_reorth with ksp_kind 1 (bcgs): BiCGStab has no basis to orthogonalise against");
    TP_REQUIRE(!o.ksp_basis_single, "ksp_reorth with ksp_basis_single: a basis rounded to fp32 cannot be orthonormal below 2^-24, "
               "a second Gram-Schmidt pass buys nothing");
    TP_REQUIRE(o.ksp_reorth_eta > 0.0 && o.ksp_reorth_eta < 1.0, "ksp_reorth_eta must lie in (0, 1)");
}
void basis_single_release(tp_ctx *c) {
    c->V.free(); c->Z.free(); c->gs_cap = 0;
    c->Vs.free(); c->Zs.free(); c->kstage.free(); c->gs_cap_s = 0;
}

// column j of the Hessenberg matrix from the Gram-Schmidt coefficients hcol[0..j] and hn = ||w||: the previous Givens rotations,
// the new one, the rotated right-hand side.  Returns the recurrence residual norm |g_{j+1}|
static double givens_column(std::vector<double> &H, std::vector<double> &cs, std::vector<double> &sn, std::vector<double> &gvec,
                            const double *hcol, double hn, int m, int j) {
    for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = hcol[i];
    H[(size_t)(j + 1) * m + j] = hn;
    for (int i = 0; i < j; ++i) {
        const double t = cs[i] * H[(size_t)i * m + j] + sn[i] * H[(size_t)(i + 1) * m + j];
        H[(size_t)(i + 1) * m + j] = -sn[i] * H[(size_t)i * m + j] + cs[i] * H[(size_t)(i + 1) * m + j];
        H[(size_t)i * m + j] = t;
    }
    const double d = std::hypot(H[(size_t)j * m + j], H[(size_t)(j + 1) * m + j]);
    cs[j] = H[(size_t)j * m + j] / d;
    sn[j] = H[(size_t)(j + 1) * m + j] / d;
    H[(size_t)j * m + j] = d;
    H[(size_t)(j + 1) * m + j] = 0.0;
    gvec[j + 1] = -sn[j] * gvec[j];
    gvec[j] = cs[j] * gvec[j];
    return std::fabs(gvec[j + 1]);
}
// y = H(0:k,0:k)^-1 g(0:k)
static void hessenberg_solve(const std::vector<double> &H, const std::vector<double> &gvec, int m, int k, std::vector<double> &y) {
    y.assign(k, 0.0);
    for (int i = k - 1; i >= 0; --i) {
        double s = gvec[i];
        for (int q = i + 1; q < k; ++q) s -= H[(size_t)i * m + q] * y[q];
        y[i] = s / H[(size_t)i * m + i];
    }
}

// basis storage grows on demand (restart 200 x 2 vectors would be 10.8 GB on SPE10 3-D), to max(need, min(restart + 1,
// max(32, 2 cap))) vectors; in the fp32 form the padding between two vectors arrives zeroed and is never written
template <typename T>
static void grow_basis(tp_ctx *c, DBuf<T> &V, DBuf<T> &Z, int &have, long stride, int need, int restart) {
    if (have >= need) return;
    const int cap = std::max(need, std::min(restart + 1, std::max(32, 2 * have)));
    DBuf<T> nV, nZ;
    nV.alloc((size_t)cap * stride);
    nZ.alloc((size_t)cap * stride);
    if (have > 0) {
        TP_HIP(hipMemcpyAsync(nV.p, V.p, sizeof(T) * have * stride, hipMemcpyDeviceToDevice, c->stream));
        TP_HIP(hipMemcpyAsync(nZ.p, Z.p, sizeof(T) * have * stride, hipMemcpyDeviceToDevice, c->stream));
        TP_HIP(hipStreamSynchronize(c->stream));
    }
    std::swap(V.p, nV.p); std::swap(V.n, nV.n);
    std::swap(Z.p, nZ.p); std::swap(Z.n, nZ.n);
    have = cap;
}

// ------------------------------------------------------------------------------------------------
// FGMRES(m) from x0 = 0 to the relative tolerance rtol (ksp_rtol, or the solve's eta under ksp_ew: tp_common.hpp).  Returns KSP reason (2 = CONVERGED_RTOL, 3 = CONVERGED_ATOL, -3 = DIVERGED_ITS).
// (the other outer method, tp_options.ksp_kind = 1, is bcgs in tp_bcgs.hip)
//
// One restart loop serves both representations of the bases, chosen by tp_options.ksp_basis_single.  What
// they differ in stands in the helpers at the head of the function and in the verdict at a cycle's end:
//                   fp64 basis                               fp32 basis
//   storage         V_j, Z_j doubles, nv apart (gs_cap)      Vs_j, Zs_j floats, basis_stride() apart (gs_cap_s); the fp64 vectors
//                                                            the kernels work on are the staging vectors W and Zt (kstage)
//   z_j, w          Z_j = M^-1 V_j ; V_{j+1} = J Z_j         Zt = M^-1 W ; Zs_j = (float) Zt, Zt widened back BEFORE W = J Zt, so
//                                                            FGMRES stays exactly consistent with the stored Z
//   v_{j+1}         V_{j+1} scaled in place                  Vs_{j+1} = (float)(W/||W||), W <- widen(Vs_{j+1}) in place
//   orthogonalise   against V, with ksp_reorth               W against the widened Vs, one pass
//   cycle ends at   tol                                      max(tol, theta beta_cycle), theta = ksp_single_floor: below that the
//                                                            rounded basis has lost its orthogonality and the recurrence no
//                                                            longer tracks the residual
//   verdict         the recurrence residual; r = b - J x     always r = b - J x, recomputed at every cycle's end (counted in
//                   is formed only to restart                ksp_cycles, ksp_true_res)
int fgmres(tp_ctx *c, const double *bvec, double *x, int *its_out, double *rnorm_out, double rtol) {
    const GridDev &g = c->g;
    const int B = c->b;
    const bool single = c->opt.ksp_basis_single;
    const long nv = (long)B * g.ntot, vs = single ? basis_stride(c) : nv;
    const int maxit = c->opt.ksp_max_it;
    const int restart = std::max(1, std::min(c->opt.ksp_restart, maxit));
    ensure_work(c);
    double *W = nullptr, *Zt = nullptr;
    if (single) {
        c->ksp_cycles = c->ksp_true_res = 0;
        if (c->kstage.n < (size_t)tp_ctx::KS_STAGE * nv) c->kstage.alloc((size_t)tp_ctx::KS_STAGE * nv);
        W = c->kstage.p;
        Zt = c->kstage.p + nv;
    }
    // ---- the basis: everything the two representations differ in, up to the verdict at a cycle's end (the pointers are formed
    // at the call: ensure_basis moves the storage) ----
    auto ensure_basis = [&](int need) {
        if (single) grow_basis(c, c->Vs, c->Zs, c->gs_cap_s, vs, need, restart);
        else grow_basis(c, c->V, c->Z, c->gs_cap, nv, need, restart);
    };
    auto w_of = [&](int j) { return single ? W : c->V.p + (long)(j + 1) * nv; };                 // where w = J z_j lives
    auto apply_and_multiply = [&](int j) {                                                         // z_j = M^-1 v_j ; w = J z_j
        double *v = single ? W : c->V.p + (long)j * nv, *z = single ? Zt : c->Z.p + (long)j * nv;
        pc_apply(c, v, z);
        if (single) basis_round_store(c, B, Zt, c->Zs.p + (long)j * vs);
        krylov_apply(c, z, w_of(j));                             // J z_j plus the wells' rank-1 terms (multi-GPU: exchange of z_j's halos overlapped)
    };
    auto orth = [&](int j, double *host_out) {                   // h = V^T w ; w -= V h ; ||w||^2 (host_out null: no host wait yet)
        if (single) orthogonalize_s(c, B, c->Vs.p, vs, j + 1, W, host_out);
        else orthogonalize(c, B, c->V.p, nv, j + 1, w_of(j), host_out);
    };
    auto set_v = [&](int j, double a, const double *src) {       // v_j = a src
        if (single) basis_scale_store(c, B, a, src, W, c->Vs.p + (long)j * vs);
        else vec_scale_to(c, B, a, src, c->V.p + (long)j * nv);
    };
    auto set_v_dev_norm = [&](int j) {                           // v_{j+1} = w/||w||, the norm still on the device
        if (single) basis_scale_store_dev(c, B, orthogonalize_norm_dev(c, j + 1), W, c->Vs.p + (long)(j + 1) * vs);
        else vec_scale_dev_norm(c, B, orthogonalize_norm_dev(c, j + 1), w_of(j));
    };
    auto add_Zy = [&](int k, const double *y, double *dst) {     // dst += Z y
        if (single) multi_axpy_s(c, B, c->Zs.p, vs, k, y, 1.0, dst);
        else multi_axpy(c, B, c->Z.p, nv, k, y, 1.0, dst);
    };
    int its = 0;
    auto done = [&](int reason, double rnorm) { *its_out = its; *rnorm_out = rnorm; return reason; };

    vec_zero(c, x, nv);
    const double bnorm = norm2(c, B, bvec);
    if (bnorm == 0.0) return done(2, 0.0);
    if (!std::isfinite(bnorm)) return done(-9, bnorm);
    const double tol = std::max(rtol * bnorm, c->opt.ksp_atol);
    double beta = bnorm;
    const double *rsrc = bvec;
    std::vector<double> H, cs, sn, gvec, hcol, yk;
    // The loop is PIPELINED.  The host needs h (Givens rotations, convergence test) once per iteration; waiting for
    // it with the stream empty leaves the GPU idle for a host wake-up plus a launch latency (~40 us of a 1.1 ms iteration).
    // Instead v_{j+1} = w / ||w|| is formed from the norm on the device and z_{j+1} = M^-1 v_{j+1}, J z_{j+1} are enqueued
    // BEFORE the host waits -- on an event behind the reductions, not on the stream.  Speculative: if iteration j turns out
    // to be the last, that work is discarded (~0.9 ms), so it is only issued while the residual, extrapolated with the last
    // reduction factor, stays 4x above the cycle's threshold.  Same arithmetic either way (bit-identical iterates).
    static const bool pipe_on = tp_switch_flag(TP_SW_FGMRES_PIPE);
    static const double spec_margin = tp_switch_real(TP_SW_SPEC_MARGIN);
    while (true) {
        const int m = std::min(restart, maxit - its);
        H.assign((size_t)(m + 1) * m, 0.0);
        cs.assign(m, 0.0); sn.assign(m, 0.0); gvec.assign(m + 1, 0.0);
        hcol.resize(m + 2);
        gvec[0] = beta;
        // this cycle's stopping threshold (not folded into max(tol, 0 * beta): the fp64 form compares with tol whatever beta is)
        const double stop = single ? std::max(tol, c->opt.ksp_single_floor * beta) : tol;
        if (single) ++c->ksp_cycles;
        ensure_basis(2);
        set_v(0, 1.0 / beta, rsrc);                                         // v0 = r/beta
        int k = 0, reason = 0;
        double res = beta, res_prev = beta, rate = 1.0;
        bool have_w = false;               // z_j, w = J z_j already enqueued by the previous iteration
        for (int j = 0; j < m; ++j) {
            const bool pipe = pipe_on && !c->monitor && orthogonalize_can_split(c, j + 2);
            ensure_basis(j + (pipe ? 3 : 2));
            if (!have_w) apply_and_multiply(j);
            have_w = false;
            bool spec = false;
            if (pipe) {
                orth(j, nullptr);
                spec = j + 1 < m && its + 1 < maxit && res_prev * std::min(rate, 1.0) > spec_margin * stop;     // (predicted res_j)
                if (spec) ++c->spec_issued; else ++c->spec_skipped;
                if (spec) {
                    set_v_dev_norm(j);
                    apply_and_multiply(j + 1);
                    have_w = true;
                }
                orthogonalize_wait(c, j + 1, hcol.data());
            } else {
                orth(j, hcol.data());
            }
            const double hn = std::sqrt(hcol[j + 1]);
            res = givens_column(H, cs, sn, gvec, hcol.data(), hn, m, j);
            ++its;
            k = j + 1;
            if (c->monitor) {
                // ksp.buildResidual() per field (thermalmodel.py:44-74): x_j = x + Z y_j, r = b - J x_j, ||r_f||
                std::vector<double> ym, fn(B, 0.0);
                hessenberg_solve(H, gvec, m, k, ym);
                double *xm = c->w4.p, *rm = c->w2.p;                        // free between pc_apply calls (this cycle's r is already in v0)
                vec_copy(c, x, xm, nv);
                add_Zy(k, ym.data(), xm);
                if (c->dist) halo_exchange(c, g, xm, B, g.ntot);
                krylov_resid(c, bvec, xm, rm);
                // (each field plane as a 1-field vector)
                for (int f = 0; f < B; ++f) { const double *one[1] = {rm + (long)f * g.ntot}; multi_norm2sq(c, 1, 1, one, &fn[f]); fn[f] = std::sqrt(fn[f]); }
                c->monitor(its, res, fn.data(), B, c->monitor_user);
            }
            rate = res_prev > 0.0 ? res / res_prev : 1.0;
            res_prev = res;
            if (!std::isfinite(res) || res <= stop || hn == 0.0) {
                if (have_w) ++c->spec_wasted;
                if (have_w) c->vcycles -= vcycles_per_apply(c);   // (discarded application)
                reason = !std::isfinite(res) ? -9 : 2;                     // KSP_DIVERGED_NANORINF | the recurrence's end of the cycle (or happy breakdown)
                break;
            }
            if (!spec) set_v(j + 1, 1.0 / hn, w_of(j));                     // v_{j+1} = w/||w||
        }
        hessenberg_solve(H, gvec, m, k, yk);
        add_Zy(k, yk.data(), x);                                            // x += Z y
        if (reason == -9) return done(-9, res);
        if (!single) {                     // the recurrence decides; its >= maxit is tested BEFORE a restart residual is formed
            if (reason) return done(reason, res);
            if (its >= maxit) return done(-3, res);
        }
        // r = b - J x: to restart from and, in the fp32 form, the only verdict
        if (c->dist) halo_exchange(c, g, x, B, g.ntot);
        krylov_resid(c, bvec, x, c->w2.p);
        beta = norm2(c, B, c->w2.p);
        rsrc = c->w2.p;
        // (fp64: no finiteness test here -- a non-finite beta surfaces as -9 one iteration later, with that iteration counted)
        if (single) {
            ++c->ksp_true_res;
            if (!std::isfinite(beta)) return done(-9, beta);
        }
        if (beta <= tol) return done(2, beta);
        if (single && its >= maxit) return done(-3, beta);
    }
}

// ------------------------------------------------------------------------------------------------
// Backtracking line search (tp_options.ls_kind = 1, snes_linesearch_type bt).
void ls_check_options(const tp_options &o) {
    TP_REQUIRE(o.ls_kind == 0 || o.ls_kind == 1, "ls_kind must be 0 (basic) or 1 (bt)");
    if (o.ls_kind == 0) {
        // the bt fields at their defaults (or zeroed, as a C caller that never heard of them leaves them): refused, never ignored
        TP_REQUIRE(o.ls_order == 0 || o.ls_order == 3, "ls_order is set but ls_kind is 0 (basic): the field belongs to the bt search");
        TP_REQUIRE(o.ls_max_it == 0 || o.ls_max_it == 40, "ls_max_it is set but ls_kind is 0 (basic): the field belongs to the bt search");
        TP_REQUIRE(o.ls_alpha == 0.0 || o.ls_alpha == 1e-4, "ls_alpha is set but ls_kind is 0 (basic): the field belongs to the bt search");
        TP_REQUIRE(o.ls_maxstep == 0.0 || o.ls_maxstep == 1e8, "ls_maxstep is set but ls_kind is 0 (basic): the field belongs to the bt search");
        TP_REQUIRE(o.ls_minlambda == 0.0 || o.ls_minlambda == 1e-12, "ls_minlambda is set but ls_kind is 0 (basic): the field belongs to the bt search");
        for (int f = 0; f < 3; ++f)
            TP_REQUIRE(!(o.ls_max_change[f] > 0.0), "ls_max_change is set but ls_kind is 0 (basic): the field belongs to the bt search");
        return;
    }
    TP_REQUIRE(o.ls_order == 2 || o.ls_order == 3, "ls_order must be 2 (quadratic) or 3 (cubic)");
    TP_REQUIRE(o.ls_alpha > 0.0 && o.ls_alpha < 0.5, "ls_alpha must lie in (0, 0.5)");
    TP_REQUIRE(o.ls_max_it >= 1, "ls_max_it must be >= 1");
    TP_REQUIRE(o.ls_maxstep > 0.0, "ls_maxstep must be > 0");
    TP_REQUIRE(o.ls_minlambda >= 0.0 && o.ls_minlambda < 1.0, "ls_minlambda must lie in [0, 1)");
    for (int f = 0; f < 3; ++f) TP_REQUIRE(o.ls_max_change[f] == o.ls_max_change[f], "ls_max_change must not be NaN");
}

// The next trial length after the finite rejected trial (lam, phi = ||F||^2); (lam_p, phi_p): the finite rejected trial before
// it, if any since the start or the last non-finite trial.  f = phi / 2, f0 = ||F0||^2 / 2, slope g0 = -||F0||^2.  Written
// operation by operation as tests/newton_ls_ref.py:next_lambda is: same inputs, same bits.
double ls_next_lambda(int order, double g0, double f0, double lam, double phi, bool have_prev, double lam_p, double phi_p) {
    double nl;
    const double f = 0.5 * phi;
    if (order == 2 || !have_prev) {
        nl = -g0 * lam * lam / (2.0 * (f - f0 - g0 * lam));                 // minimiser of the quadratic through f0, g0, f
    } else {
        // Dennis & Schnabel, A6.3.1: minimiser of the cubic through f0, g0 and the last two trials
        const double fp = 0.5 * phi_p;
        const double t1 = f - f0 - lam * g0, t2 = fp - f0 - lam_p * g0;
        const double a = (t1 / (lam * lam) - t2 / (lam_p * lam_p)) / (lam - lam_p);
        const double b = (-lam_p * t1 / (lam * lam) + lam * t2 / (lam_p * lam_p)) / (lam - lam_p);
        const double d = b * b - 3.0 * a * g0;
        if (d < 0.0) nl = 0.5 * lam;
        else if (a == 0.0) nl = -g0 / (2.0 * b);
        else nl = (-b + std::sqrt(d)) / (3.0 * a);
    }
    if (!(nl >= 0.1 * lam)) nl = 0.1 * lam;                                 // (also catches a NaN)
    if (nl > 0.5 * lam) nl = 0.5 * lam;
    return nl;
}

// One search from u0 = c->u (residual norm fnorm_in, correction dx).  On success c->u is the accepted iterate, R and J are
// assembled there, and lam, ynorm, phi = ||F||^2, xsq = ||u||^2 describe the step.  On failure c->u is u0 again.
static bool ls_backtrack(tp_ctx *c, bool schur, const double *dx, double fnorm_in, double *lam_out, double *ynorm_out,
                         double *phi_out, double *xsq_out, int *trials_out) {
    const GridDev &g = c->g;
    const int B = c->b;
    const long nv = (long)B * g.ntot;
    const tp_options &o = c->opt;
    if (c->ls_u0.n < (size_t)nv) c->ls_u0.alloc(nv);
    double st[4];
    ls_step_stats(c, dx, st);                                               // (all-reduced: every slab decides alike)
    vec_copy(c, c->u.p, c->ls_u0.p, nv);
    const double ynorm = std::sqrt(st[0]);
    double lam = 1.0;
    if (o.ls_maxstep / ynorm < lam) lam = o.ls_maxstep / ynorm;
    for (int f = 0; f < B; ++f)
        if (o.ls_max_change[f] > 0.0 && o.ls_max_change[f] / st[1 + f] < lam) lam = o.ls_max_change[f] / st[1 + f];
    const double ff = fnorm_in * fnorm_in, f0 = 0.5 * ff, g0 = -ff;
    bool have = false, have_prev = false;                                   // finite rejected trials since the last non-finite one
    double lam_1 = 0.0, phi_1 = 0.0, lam_2 = 0.0, phi_2 = 0.0;
    *ynorm_out = ynorm;
    bool ok = std::isfinite(ynorm);
    for (int t = 1; ok; ++t) {
        ls_trial(c, c->ls_u0.p, dx, lam, c->u.p);
        if (c->dist) halo_exchange(c, g, c->u.p, B, g.ntot);
        if (t == 1) assemble(c, true, schur);                               // an accepted first trial costs what the basic step costs
        else assemble(c, false, false);
        double nrm[2];
        const double *v2[2] = {c->R.p, c->u.p};
        multi_norm2sq(c, B, 2, v2, nrm);                                    // the one host wait of a trial
        const double phi = nrm[0];
        ++c->ls_evals;
        *trials_out = t;
        const bool finite = std::isfinite(phi);
        if (!finite) ++c->ls_nonfinite;
        if (finite && phi <= (1.0 - 2.0 * o.ls_alpha * lam) * ff) {
            // INVARIANT: a rejected first trial left J (and S~) of a state that was thrown away, possibly non-finite, and later
            // trials wrote R only.  The fused assembly below rewrites EVERY owned entry of R, J and S~ from the accepted
            // state -- the assembly kernels store, they never accumulate into what they find -- so nothing of a rejected
            // trial reaches pc_setup.  (Halo planes of J are written by nobody and exchanged where they are read.)
            if (t > 1) assemble(c, true, schur);
            *lam_out = lam; *phi_out = phi; *xsq_out = nrm[1];
            return true;
        }
        if (t >= o.ls_max_it) break;
        if (!finite) {
            lam = 0.5 * lam;
            have = have_prev = false;
        } else {
            if (have) { lam_2 = lam_1; phi_2 = phi_1; have_prev = true; }
            lam_1 = lam; phi_1 = phi; have = true;
            lam = ls_next_lambda(o.ls_order, g0, f0, lam_1, phi_1, have_prev, lam_2, phi_2);
        }
        if (lam < o.ls_minlambda) break;
    }
    vec_copy(c, c->ls_u0.p, c->u.p, nv);                                    // u <- u0, bitwise (halo planes included)
    c->jac_ready = c->pc_ready = false;                                     // R, J: whatever the last trial left
    return false;
}

// ------------------------------------------------------------------------------------------------
void newton(tp_ctx *c, tp_solve_info *info) {
    const GridDev &g = c->g;
    const int B = c->b;
    const long nv = (long)B * g.ntot;
    ensure_work(c);
    const bool schur = schur_of(c->opt);
    if (schur && c->Sm.n < (size_t)7 * g.ntot) c->Sm.alloc((size_t)7 * g.ntot);
    TP_REQUIRE(c->u.n > 0, "state not set");
    tp::DBuf<double> *dx = &c->dx;
    if (dx->n < (size_t)nv) dx->alloc(nv);

    if (c->dist) halo_exchange(c, g, c->u.p, B, g.ntot);
    assemble(c, true, schur);
    double fnorm = norm2(c, B, c->R.p);
    const double fnorm0 = fnorm;
    int nits = 0, lits = 0, reason = 0, kreason = 0;
    c->ls_lambda.clear(); c->ls_fnorm.clear(); c->ls_trials.clear();
    c->ls_evals = c->ls_nonfinite = 0;
    // Eisenstat-Walker (tp_options.ksp_ew, tp_ew.hpp): eta_k of linear solve k from ||F_k||, ||F_{k-1}||, rho_{k-1}, eta_{k-1}.  The
    // norms are the all-reduced ones, so every slab computes the same eta bit for bit.  Off: rtol below is ksp_rtol, as ever.
    const bool ew = c->opt.ksp_ew != 0;
    double ew_f_last = 0.0, ew_rho_last = 0.0, ew_eta_last = 0.0;
    c->ew_rtol.clear(); c->ew_fnorm.clear(); c->ew_lresid.clear(); c->ew_kits.clear(); c->ew_kreason.clear();
    if (ew) ++c->ew_solves;
    if (!std::isfinite(fnorm)) reason = -4;                      // SNES_DIVERGED_FNORM_NAN
    else if (fnorm < c->opt.snes_atol) reason = 2;               // SNES_CONVERGED_FNORM_ABS
    while (reason == 0) {
        if (nits >= c->opt.snes_max_it) { reason = -5; break; }  // SNES_DIVERGED_MAX_IT
        pc_setup(c);
        int kits = 0;
        double rn = 0.0;
        // (lits counts Krylov iterations: a BiCGStab iteration applies the preconditioner twice, vcycles counts per application)
        double rtol = c->opt.ksp_rtol;
        if (ew) {
            int fl = 0;
            rtol = ew_next_rtol(c->opt, (int)c->ew_rtol.size(), fnorm, ew_f_last, ew_rho_last, ew_eta_last, &fl);
            ++c->ew_lsolves;
            if (fl & EW_SAFE_RAISED) ++c->ew_safeguard;
        }
        kreason = c->opt.ksp_kind == 1 ? bcgs(c, c->R.p, dx->p, &kits, &rn, rtol) : fgmres(c, c->R.p, dx->p, &kits, &rn, rtol);
        lits += kits;
        if (ew) {
            // (after an accepted bt step fnorm is the accepted trial's norm: the next eta sees it as ||F_{k+1}||)
            c->ew_rtol.push_back(rtol); c->ew_fnorm.push_back(fnorm); c->ew_lresid.push_back(rn);
            c->ew_kits.push_back(kits); c->ew_kreason.push_back(kreason);
            ew_f_last = fnorm; ew_rho_last = rn; ew_eta_last = rtol;
        }
        if (kreason < 0) { reason = -3; break; }                 // SNES_DIVERGED_LINEAR_SOLVE
        if (c->opt.ls_kind == 1) {                               // bt: backtracking from the full step (ls_backtrack above)
            double lam = 0.0, ynorm = 0.0, phi = 0.0, xsq = 0.0;
            int trials = 0;
            if (!ls_backtrack(c, schur, dx->p, fnorm, &lam, &ynorm, &phi, &xsq, &trials)) { reason = -6; break; }   // SNES_DIVERGED_LINE_SEARCH
            ++nits;
            fnorm = std::sqrt(phi);
            c->ls_lambda.push_back(lam); c->ls_fnorm.push_back(fnorm); c->ls_trials.push_back(trials);
            const double snorm = lam * ynorm, xnorm = std::sqrt(xsq);
            if (fnorm < c->opt.snes_atol) reason = 2;            // (an accepted phi is finite)
            else if (fnorm <= c->opt.snes_rtol * fnorm0) reason = 3;
            else if (snorm < c->opt.snes_stol * xnorm) reason = 4;
            continue;
        }
        vec_axpy_owned(c, B, -1.0, dx->p, c->u.p);               // basic line search, lambda = 1
        if (c->dist) halo_exchange(c, g, c->u.p, B, g.ntot);
        assemble(c, true, schur);
        ++nits;
        double nrm[3];
        const double *nv3[3] = {c->R.p, dx->p, c->u.p};
        multi_norm2sq(c, B, 3, nv3, nrm);                       // one reduction, one all-reduce, one host sync
        fnorm = std::sqrt(nrm[0]);
        const double snorm = std::sqrt(nrm[1]), xnorm = std::sqrt(nrm[2]);
        if (!std::isfinite(fnorm)) reason = -4;
        else if (fnorm < c->opt.snes_atol) reason = 2;
        else if (fnorm <= c->opt.snes_rtol * fnorm0) reason = 3;  // SNES_CONVERGED_FNORM_RELATIVE
        else if (snorm < c->opt.snes_stol * xnorm) reason = 4;    // SNES_CONVERGED_SNORM_RELATIVE
    }
    info->nits = nits;
    info->lits = lits;
    info->reason = reason;
    info->last_ksp_reason = kreason;
    info->fnorm0 = fnorm0;
    info->fnorm = fnorm;
    info->vcycles = (int)c->vcycles;
}

}  // namespace tp
