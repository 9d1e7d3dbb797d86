// Shared host-side declarations of libthermalporous_hip (context, buffers, launch helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include <stdexcept>
#include <functional>
#include "../../include/thermalporous_hip.h"
#include "tp_ew.hpp"
#include "tp_switches.hpp"

struct ncclComm;

namespace tp {
struct LocalGroup;

void set_error(const std::string &msg);

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define TP_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            throw tp::Error(std::string(#call) + " failed: " + hipGetErrorString(e_) + " at " +  \
                            __FILE__ + ":" + std::to_string(__LINE__));                          \
    } while (0)

#define TP_REQUIRE(cond, msg)                                                                    \
    do {                                                                                         \
        if (!(cond)) throw tp::Error(std::string(msg) + " [" #cond "]");                         \
    } while (0)

// Device view of the slab grid, passed by value to kernels.
struct GridDev {
    int n0, n1, n2;        // owned
    int gn2, off2;         // global extent/offset along axis 2
    long np;               // n0*n1 (plane)
    long nown;             // np*n2
    long ntot;             // np*(n2+2)
    int nb_lo, nb_hi;      // 1 if a neighbouring slab exists below/above (halo is live)
};

inline GridDev make_grid(int n0, int n1, int n2, int gn2, int off2) {
    GridDev g;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.gn2 = gn2; g.off2 = off2;
    g.np = (long)n0 * n1; g.nown = g.np * n2; g.ntot = g.np * (n2 + 2);
    g.nb_lo = off2 > 0; g.nb_hi = off2 + n2 < gn2;
    return g;
}

// XCD-aware block -> cell-range mapping (cdna_hip_programming.md T1): workgroups are dealt round-robin over
// the 8 XCDs, each with its own L2.  Remapping block b to chunk (b % 8)*(nblocks/8) + b/8 gives every XCD
// one contiguous eighth of the cell range, so the stencil's neighbour reads (x at c +- 1, +- n0, +- n0*n1)
// hit in that XCD's L2 instead of being fetched once per XCD.  Pure performance: any placement is correct.
// Grids launched with xcd_grid() have a multiple of 8 blocks; the kernel bounds-checks the cell index.
#if defined(__HIPCC__)
// Every kernel that calls this is launched with TP_BLOCK (= 256) threads (xcd_grid's default): the block size is a compile-time
// constant here on purpose.  `blockDim.x` is a 16-bit field of the hidden kernel arguments that the compiler fetches with a
// VECTOR load (global_load_ushort) followed by s_waitcnt vmcnt(0) before the first useful instruction: one dependent memory round
// trip at the start of every kernel, ~0.5-1 us of the 4-6 us the small AMG levels' kernels take.
constexpr int TP_BLOCK = 256;
__device__ __forceinline__ long xcd_tid() {
    const unsigned nb = gridDim.x, b = blockIdx.x;
    const unsigned rb = (b & 7u) * (nb >> 3) + (b >> 3);
    return (long)rb * TP_BLOCK + threadIdx.x;
}
// Multi-GPU AMG (tp_amg.hip, tp_amg_block.hip): along the slab axis (2) the C points are the even GLOBAL planes, so a slab that
// starts on an odd plane is shifted by one; its F neighbours / C parents across the slab boundary live in the halo planes.
__device__ __forceinline__ int par_of(const GridDev &gf, int a) { return a == 2 ? (gf.off2 & 1) : 0; }
__device__ __forceinline__ bool open_lo(const GridDev &g, int a) { return a == 2 && g.nb_lo; }
__device__ __forceinline__ bool open_hi(const GridDev &g, int a) { return a == 2 && g.nb_hi; }
#endif
inline dim3 xcd_grid(long n, int bs = 256) {
    const long nb = (n + bs - 1) / bs;
    return dim3((unsigned)(((nb + 7) / 8) * 8));
}
inline dim3 grid_for(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

// pc_kind: 0 pc_cpr, 1 pc_cptr, 2 pc_fieldsplit_cd, 3 pc_cptramg.  1 and 2 run the fieldsplit-Schur-FULL stage on
// (p,T) and need the S~ operator from the assembly; 3 runs ONE system-AMG V-cycle on the 2x2-block (p,T) operator.
inline int npri_of(const tp_options &o) { return o.pc_kind >= 1 ? 2 : 1; }
inline bool schur_of(const tp_options &o) { return o.pc_kind == 1 || o.pc_kind == 2; }
inline bool sysamg_of(const tp_options &o) { return o.pc_kind == 3; }

// Scalar 7-point stencil operator: slot s lives at base + s*slot_stride (doubles).
struct Stencil {
    double *base = nullptr;
    long slot_stride = 0;
    __host__ __device__ const double *slot(int s) const { return base + (long)s * slot_stride; }
    __host__ __device__ double *slot(int s) { return base + (long)s * slot_stride; }
};

// Block 7-point stencil operator (system AMG): block (q,r) of slot s lives at base + s*ss + q*rs + r*cs.
struct BStencil {
    double *base = nullptr;
    long ss = 0, rs = 0, cs = 0;
    __host__ __device__ const double *at(int s, int q, int r) const { return base + s * ss + q * rs + r * cs; }
    __host__ __device__ double *at(int s, int q, int r) { return base + s * ss + q * rs + r * cs; }
};

// Derived closure constants (device copy of tp_params + precomputed factors).
struct DevPrm {
    double ko, kw, kr, c_v_w, c_v_o, c_r, rho_r, T_inj, g, U;
    double rho_ref, mu_o_coef, mu_o_exp;   // oil_rho / oil_mu (physicalparameters.py:37-57)
    double w0, w2;                          // equation weights (twophase.py:142-147)
};

// Saturation functions (tp_set_saturation_functions) as the kernels read them: Corey's curves on
// Se_o = (S - Sr_o)/D and Se_w = (So_max - S)/D, So_max = 1 - Sr_w (this order, so that S = 1 - Sr_w is the end exactly, as
// S = Sr_o is), and the capillary pressure.  Only the SATFN instantiations take one; DevPrm does not change.
struct DevSat {
    double Sr_o, So_max, D, invD;           // residual oil, 1 - Sr_w, D = 1 - Sr_o - Sr_w and 1/D
    double n_o, n_w, kro_max, krw_max;      // Corey exponents and end points (Brooks-Corey: translated by the caller)
    double p_ct, inv_lmbda, pc_se_min, pc_max;   // entry pressure, 1/lmbda, floor of Se_w, and p_c at that floor
    int kr_kind, pc_kind;                   // tp_satfn.relperm, tp_satfn.capillary
};

template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    bool owned = true;
    void alloc(size_t n_) {
        free();
        n = n_;
        if (n) {
            // (zeroed on the per-thread stream, complete on return.  Nothing in the library uses the LEGACY default stream: a
            // legacy-stream operation synchronises with every blocking stream of the device and is an error -- "would make the
            // legacy stream depend on a capturing blocking stream" -- while any other slab thread is capturing its pc_apply)
            TP_HIP(hipMalloc((void **)&p, n * sizeof(T)));
            TP_HIP(hipMemsetAsync(p, 0, n * sizeof(T), hipStreamPerThread));
            TP_HIP(hipStreamSynchronize(hipStreamPerThread));
        }
    }
    // a slice of somebody else's allocation (zeroed by its owner)
    void view(T *q, size_t n_) {
        free();
        p = q; n = n_; owned = false;
    }
    void free() {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        n = 0;
        owned = true;
    }
    ~DBuf() { free(); }
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
};

// move-only owner of one instantiated hipGraph (a capture segment of a recorded pc_apply program)
struct GraphExec {
    hipGraphExec_t h = nullptr;
    GraphExec() = default;
    explicit GraphExec(hipGraphExec_t h_) : h(h_) {}
    GraphExec(GraphExec &&o) noexcept : h(o.h) { o.h = nullptr; }
    GraphExec &operator=(GraphExec &&o) noexcept { std::swap(h, o.h); return *this; }
    GraphExec(const GraphExec &) = delete;
    GraphExec &operator=(const GraphExec &) = delete;
    ~GraphExec() { if (h) (void)hipGraphExecDestroy(h); }
};

// Layout of one semicoarsening hierarchy, shared by the scalar (tp_amg.hip) and the system (tp_amg_block.hip) AMG: pure host-side
// integer logic, built once by amg_plan (tp_amg.hip), mirrored by oracle/linalg.py and reported by tp_amg_layout.  Every option it
// is derived from is in tp_set_options' amg_changed list, which deletes the hierarchies: a plan never outlives its options.
struct AmgPlan {
    struct Level {
        GridDev g;             // levels [0, dist_levels): this rank's slab of the level; below: the whole box, dead halo planes
        int axis = -1;         // coarsening axis towards the next level (-1: coarsest)
        int pre = 0, post = 0; // smoothing sweeps V(pre, post); post == 0: pure transfer level
        // line relaxation (tp_options.amg_line_levels): the level's sweeps are line-Jacobi along axis 0, one workgroup per
        // line_g consecutive lines (flattened line index i1 + n1 i2); line_g == 0: point Jacobi
        int line_g = 0;
        // red-black Gauss-Seidel (tp_options.amg_gs_levels): gs > 0: the level's sweeps are GS sweeps, pre == post == gs
        int gs = 0;
    };
    std::vector<int> sched;    // axis of every coarsening step
    std::vector<Level> lv;     // sched.size() + 1 levels
    // multi-GPU: levels [0, dist_levels) live on this rank's slab (halo exchanges between sweeps), the levels
    // below on the gathered global grid, replicated on every rank.  0 = the whole hierarchy is replicated.
    int dist_levels = 0;
    int tail_level = 0;        // first level handled by the single-workgroup tail kernel
    std::vector<std::vector<std::pair<int, int>>> ranges;   // [level][rank] -> owned global planes along axis 2
    // level l+1 as its parent level l sees it.  Below the last distributed level that is `rank`'s planes of the global
    // (replicated) arrays -- pointer arithmetic, no copy: plane 0 of the view is the lower halo.
    struct View {
        GridDev g;
        long off;              // element offset of the view inside the level's arrays
    };
    View coarse_view(int l, int rank) const {
        const GridDev &gc = lv[l + 1].g;
        if (l + 1 < dist_levels || l >= dist_levels) return {gc, 0};
        const auto &q = ranges[l + 1][rank];
        return {make_grid(gc.n0, gc.n1, q.second - q.first, gc.n2, q.first), gc.np * q.first};
    }
};

struct AmgLevel {
    GridDev g;                 // (copies of the plan's, filled by amg_build)
    DBuf<double> A;        // 7 planes (levels >= 1); level 0 uses an external stencil view
    Stencil op;
    DBuf<double> invd;     // omega / diag
    DBuf<double> wm, wp;   // interpolation weights of F points along `axis`
    DBuf<double> b, x, x2, r, e;
    // line levels: Thomas factors m, 1/d~ and the super-diagonal a+ of every line, three streams of ngroups * n0 * line_g
    // doubles in the order [group of line_g lines][i0][line of the group] (allocated once by amg_build)
    DBuf<double> linef;
    int axis = -1;
};

struct Amg {
    AmgPlan plan;
    // one allocation for every buffer of every level: the coarse levels are tiny, and with one hipMalloc each
    // (~150 of them) every small kernel of the cycle starts with TLB misses on half a dozen scattered pages
    DBuf<double> arena;
    std::vector<AmgLevel *> lv;
    DBuf<double> coarse_inv;   // dense inverse on the coarsest grid
    int ncoarse = 0;
    bool single = false;       // operators / weights / inverse diagonals stored in fp32
    double omega = 0.0;        // amg_omega of the last set-up: invd = omega / diag (LevelDevT::omega)
    int tail_lds = 0;          // doubles per LDS-resident vector set of the tail (0: tail vectors stay in global memory)
    long fuse_below = 200000;  // levels with fewer cells use the fused (launch-saving) kernels
    // relaxation-only truncation (tp_options.amg_dom_tau): dominance ratios of the V(nu,nu) levels, measured by the set-up
    // kernels into 64 slots per level (spread atomics), copied to pinned host memory behind `ev_ratio`
    DBuf<double> ratio_dev;
    double *ratio_host = nullptr;
    hipEvent_t ev_ratio = nullptr;
    bool ratio_pending = false;
    int trunc = -1;            // level that ends the cycle with two Jacobi sweeps (-1: none)
    double ratio0 = 0.0;
    // dense tail: between two set-ups the tail (levels >= plan.tail_level) is a fixed linear map e = T b on the n cells of
    // its first level.  T (row-major, n x n, allocated once: its address is part of the captured pc_apply graphs) is formed
    // by a batched launch of the tail kernel on the unit vectors after a set-up and applied by k_amg_tail_dense.
    DBuf<double> tdense;
    DBuf<double> tdense_scratch;   // per-workgroup level vectors of the batched build when they do not fit the LDS
    long tail_vec = 0;             // doubles of one vector set (b, e, x or x2) over all tail levels
    int tdense_groups = 0;         // workgroups of the build (each walks columns j, j + groups, ...)
    bool tdense_eligible = false;  // the tail has >= 2 levels and <= 1024 cells on its first (amg_build)
    bool tdense_on = false;        // the cycles after the last set-up apply T (TP_AMG_TAIL_DENSE, truncation cannot land in the tail)
    uint64_t setup_id = 0;         // counts set-ups; T is valid iff tdense_stamp == setup_id
    uint64_t tdense_stamp = ~(uint64_t)0;
    long tdense_builds = 0, tdense_applies = 0, tail_launches = 0;   // launches enqueued or captured (tp_amg_tail_info)
    DBuf<char> lvdev;          // device array of level descriptors (LevelDev) for the tail kernel
    std::vector<char> lvhost;
    ~Amg() {
        for (auto *l : lv) delete l;
        if (ratio_host) (void)hipHostFree(ratio_host);
        if (ev_ratio) (void)hipEventDestroy(ev_ratio);
    }
};

// system AMG on the (p,T) blocks (tp_amg_block.hip)
struct BAmgLevel {
    GridDev g;                 // (copies of the plan's, filled by bamg_build)
    DBuf<double> A;            // 7*NB*NB planes (levels >= 1; level 0 views the Jacobian / decoupled operator)
    BStencil op;
    DBuf<double> invD;         // NB*NB planes: omega * inverse of the diagonal block
    DBuf<double> wm, wp;       // NB planes each
    DBuf<double> b, x, x2, r, e;
    int axis = -1;
    int pre = 0, post = 0;
};

struct BAmg {
    AmgPlan plan;
    int nb = 2;
    std::vector<BAmgLevel *> lv;
    DBuf<double> dense;        // [M | Minv] of the coarsest grid, (nb*ncoarse)^2 each
    int ncoarse = 0;
    long fuse_below = 0;       // replicated levels with fewer cells fuse prolongation + first post-sweep
    DBuf<char> lvdev;          // device array of BTailLevel descriptors
    std::vector<char> lvhost;
    ~BAmg() { for (auto *l : lv) delete l; }
};

// Inner Krylov solve of the stage-1 pressure / (p,T) block (tp_inner.hip, tp_options.s1_ksp).  The operator the V-cycle
// preconditions: nplanes == 1: A[0][0] (opA00, or the gathered gA00); nplanes == 2: the 2x2 block of pc_cptramg.
struct InnerOp {
    GridDev g;                 // grid of the vectors: nplanes planes of g.ntot doubles
    Stencil A[2][2];
};
// workspace of the inner solve (sized by inner_ensure from ensure_work: never inside a capture).  Every scalar of the
// iteration -- Hessenberg column, rotations, residual estimate, the convergence latch -- lives in `state` on the device.
struct InnerWork {
    DBuf<double> V, Z;         // fgmres: s1_max_it + 1 basis vectors, s1_max_it preconditioned vectors; richardson: V = (r, e)
    DBuf<double> partial;      // per-wave partial sums of the fused reductions
    DBuf<double> state;
    DBuf<long long> stats;     // applies, iterations used, unconverged (tp_inner_stats)
};

// workspace of the outer BiCGStab (tp_bcgs.hip, tp_options.ksp_kind = 1): a fixed set of vectors allocated once per context --
// their addresses are the (input, output) pairs of the two pc_apply programs a set-up records -- and the device block that
// holds every scalar of the iteration
struct BcgsWork {
    DBuf<double> vec;          // r^, r, p, v, s, p^, s^: 7 vectors of b*ntot (t lives in tp_ctx::w2)
    DBuf<double> partial;      // per-wave partial sums, two outputs
    DBuf<double> state;        // sums, rho, alpha, omega, beta, tol, latches
};

// a batch of n compact fp32 vectors at the basis stride (tp_fvec_create_batch: the kernels of ksp_basis_single, testable alone)
struct FBatch {
    DBuf<float> buf;
    int n = 0;
};

// Dirichlet sides of the box (tp_set_boundary; k_assemble_bc in tp_assembly.hip).  side = 2*axis + d in internal axes, d = 0 the
// low-index side; a face of a side is numbered over the other two internal axes, the lower axis fastest.  Every array is
// surface-sized.  With no side set (ncells == 0) nothing of this is allocated, launched or read.
struct BcSide {
    int kind = 0;              // 0 none, 1 open (flow and conduction), 2 thermal (conduction only)
    long nf = 0;               // faces of the side
    DBuf<double> val;          // ghost state, b fields of nf
    DBuf<double> tk;           // T^K of the half cell: 2 K_a(c) |E| / h_a^2 (open), 0 (thermal)
    DBuf<double> flux;         // what each face added to R at the last assembly, b fields of nf (tp_boundary_flux)
};
struct Bc {
    BcSide side[6];
    DBuf<int> cells;           // owned indices (c - np) of the cells that touch a set side, ascending: one thread each
    int ncells = 0;
};

// Completed wells (tp_set_wells; tp_wells.hip).  With no well set (nw == 0) nothing of this is allocated, launched
// or read.  Per-perforation planes are np entries long, entry k of the caller's perforation array.
struct WellDev {
    int kind, shut, first, count, datum;   // datum: the perforation whose old pressure an injector's head density is taken at
    double rate, limit;
};
struct Wells {
    int nw = 0, np = 0;
    std::vector<tp_well> wells;            // host copies: tp_set_well_control edits them and uploads the controls again
    std::vector<tp_perf> perfs;
    DBuf<WellDev> wd;
    DBuf<long> cell;
    DBuf<double> WI, dz;                   // dz = z_ref - z_k (0 without a gravity axis)
    DBuf<double> rho;                      // per well: the head density, frozen over a time step (k_well_rho)
    DBuf<double> pa, pth;                  // scratch of k_wells: a_k, theta_k
    DBuf<double> fc, fb;                   // the rank-1 factors c and b of the last Jacobian assembly, b planes of np each
    DBuf<double> pq;                       // per-perforation rates of the last assembly: total, water, oil
    DBuf<double> info;                     // per well, 8 doubles (tp_well_info)
    DBuf<int> r1;                          // per well: 1 if the last Jacobian assembly left it a rank-1 term
};

struct IluData {
    int t0 = 0, t1 = 8, t2 = 8, nt0 = 0, nt1 = 0, nt2 = 0, ntiles = 0, nsteps = 0;
    DBuf<double> fwd, bwd, ytmp;   // streaming factor data in consumption order
    DBuf<float> fwd32, bwd32;      // tp_options.ilu_single: the same streams stored as floats (fwd / bwd are then empty)
    bool single = false;
    DBuf<double> jt;               // the Jacobian blocks re-ordered the same way (input of the factorisation)
    long slots = 0;                // ntiles*nsteps*64
    bool mw = false;               // ILU(0): factor stored in the row-major layout of the multi-wave sweep (tp_ilu.hip)
    int levels = 0;                // 0: ILU(0), 1: ILU(1) (tp_options.ilu_levels; other chunk layout, see tp_ilu.hip)
    // ILU(1): PACKED copy of the factor for the sweeps -- a (tile, step) chunk holds rows only for the lanes that have a cell
    // at that step (the s = l0 + 2j + 4k skew leaves a third of the padded stream zero, 54-lane tiles another 16 %);
    // pref[s] = slots before step s of a tile, ptot = slots per tile
    DBuf<double> fwdp, bwdp;
    DBuf<int> pref;
    int ptot = 0;
    // tp_options.ilu_whole (one block per rank) / ilu_block (boxes of bb cells): blocks of SEVERAL tiles.  The tiles of a
    // block keep their couplings; block-local tile-diagonal d = T0'+T1'+T2' of every block is one launch:
    // tiles diag_tiles[diag_off[d] .. diag_off[d+1]) (device array); xtmp: the raw backward-sweep result of every
    // (tile, step, lane) for the tiles of later launches (x itself may already hold addto + result)
    bool whole = false;            // block-bounded sweeps (false: every block is one tile)
    int bb[3] = {0, 0, 0};         // block extents (clipped to the slab), pb: tiles per full block along each axis
    int pb[3] = {1, 1, 1};
    int ndiag = 0;
    std::vector<int> diag_off;
    DBuf<int> diag_tiles;
    DBuf<double> xtmp;
};

}  // namespace tp

struct tp_ctx {
    tp_grid grid;
    tp_params prm;
    tp_options opt;
    tp::GridDev g;
    tp::DevPrm dprm;
    int nph = 1, b = 2, device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // pc_setup forks: the two AMG set-ups and the ILU factorisation are independent chains of small kernels
    hipStream_t aux[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    double dt = 0.0, vol = 0.0;
    bool fields_ready = false, have_old = false, jac_ready = false, pc_ready = false;
    // fields
    tp::DBuf<double> phi, K[3], kTs, TK[3];
    // state
    tp::DBuf<double> u, u_old, acc_old, R, J, Sm;
    // sources
    tp::DBuf<tp_source> src;
    tp::DBuf<int> src_start;      // groups of entries sharing a cell
    int nsrc = 0, nsrc_groups = 0;
    tp::DBuf<double> rates;       // 3*nsrc
    tp::Bc bc;                    // Dirichlet sides (tp_set_boundary)
    tp::Wells wells;              // completed wells (tp_set_wells)
    // graded tensor-product grid (tp_set_spacing): widths of the cells along each internal axis, on the host and
    // on the device.  graded == false: nothing of this is allocated or read and grid.h / vol describe every cell.
    bool graded = false;
    std::vector<double> hs_host[3];
    tp::DBuf<double> hs[3];
    // saturation functions (tp_set_saturation_functions).  satfn == false: the kernels launched are the
    // instantiations without them, with the arguments they have always had
    bool satfn = false;
    tp_satfn sat_host;
    tp::DevSat dsat;
    // linear algebra
    std::vector<tp::DBuf<double> *> vecs;
    tp::DBuf<double> At;          // decoupled primary block (QI/TI); planes as in J with b' = nprimary
    tp::DBuf<double> dcoef;       // decoupling coefficients d_q per cell (nprimary planes)
    tp::Stencil opA00, opA01, opA10;   // views used by stage 1
    tp::Amg *amg_p = nullptr, *amg_T = nullptr;
    // tp_options.pc_ctr: the hierarchy of the composite's temperature stage, on the T-T planes of the undecoupled J (a view, as
    // level 0 of the others); its set-ups and the T-stage applications launched since tp_create (tp_ctr_info)
    tp::Amg *amg_ctr = nullptr;
    long ctr_setups = 0, ctr_applies = 0;
    // tp_schur_info: applications of K(A00) and of K(S) issued or replayed since the last pc_setup (host counters)
    long schur_k0 = 0, schur_ks = 0;
    tp::BAmg *bamg = nullptr;          // pc_cptramg: system AMG on the (p,T) blocks (tp_amg_block.hip)
    tp::BStencil opPT;                 // pc_cptramg: the operator handed to bamg_setup (the slab's, or the gathered one)
    tp::InnerWork inner;               // s1_ksp != preonly: workspace of the inner Krylov solve (tp_inner.hip)
    tp::DBuf<double> spbuf;            // selfp (schur_a11 == 2): S7 (7 planes), w/diag(Sp), two work planes
    tp::DBuf<double> gAt;              // multi-GPU pc_cptramg: the 28 operator planes gathered on the global grid
    tp::IluData ilu;
    // FGMRES workspace
    tp::DBuf<double> V, Z, gs_partial, gs_h, red_out;
    int gs_cap = 0;
    // tp_options.ksp_basis_single: the two bases as COMPACT fp32 vectors (owned entries only, field-major, stride
    // basis_stride()) plus a ring of KS_STAGE fp64 staging vectors in the ordinary halo layout at fixed addresses: slot 0 holds
    // w = J z_j, orthogonalised and normalised in place into the widened stored v_{j+1}; slot 1 the widened stored z_j.  Every
    // preconditioner application of a solve is the one (slot 0, slot 1) program.  Exactly one representation is allocated:
    // tp_set_options frees both when the option changes.
    static constexpr int KS_STAGE = 2;
    tp::DBuf<float> Vs, Zs;
    tp::DBuf<double> kstage;
    int gs_cap_s = 0;
    // tp_options.ksp_reorth: the second Gram-Schmidt pass's sums c (k) and its ||w||^2, and the device-resident latch
    // {flag of the step in flight, second passes executed, second passes skipped} (tp_linalg.hip; tp_ksp_reorth_info)
    tp::DBuf<double> ro_c;
    tp::DBuf<long long> ro_stat;
    long ro_steps = 0;                       // orthogonalisation steps since create
    long ksp_cycles = 0, ksp_true_res = 0;   // restart cycles / true-residual evaluations of the last fp32-basis solve (tp_ksp_basis_info)
    std::vector<tp::FBatch *> fbatches;      // fp32 vector batches of the C ABI (tp_fvec_*)
    tp::BcgsWork bcgs;                 // ksp_kind 1: the BiCGStab work vectors and its device-resident scalars (tp_bcgs.hip)
    std::vector<double> hostbuf;
    // scratch vectors for PC apply
    tp::DBuf<double> w1, w2, w3, w4, dx;
    // A preconditioner application is recorded as a PROGRAM, one per (input, output) vector pair: FGMRES applies the
    // preconditioner to basis vector j into Z_j, a handful of fixed address pairs that recur in every solve.  A program is
    // hipGraph segments (the kernel sequences between two exchanges) alternating with the exchanges themselves (RCCL calls /
    // in-process copies, replayed as host closures on the same stream).  RCCL calls are never captured; only what lies between
    // them is.  A single slab has no exchange: its program is one segment, one hipGraphLaunch per replay.
    struct PcStep { tp::GraphExec exec; std::function<void()> comm; };     // a segment (exec.h set) or an exchange
    struct PcProgram { const double *x; double *y; std::vector<PcStep> steps; };
    std::vector<PcProgram> pc_programs;
    PcProgram *rec = nullptr;          // program being recorded (comm calls split the capture), else null
    bool rec_capturing = false, rec_in_comm = false;
    uint64_t graph_epoch = 1, pc_graph_epoch = 0;
    uintptr_t pc_sig = 0;
    // comm: RCCL communicator (one process per GPU) or an in-process slab group (several contexts on one GPU,
    // used to validate the slab algorithm where only one GPU is available)
    ncclComm *comm = nullptr;
    tp::LocalGroup *lgroup = nullptr;
    bool dist = false;
    // multi-GPU stage 1: the pressure (and temperature) systems gathered on the global grid of every rank
    tp::GridDev gfull;
    tp::DBuf<double> gA00, gA01, gA10, gSm, gvec;   // operators: 7 planes each; gvec: work vectors
    long vcycles = 0;
    long spec_issued = 0, spec_wasted = 0, spec_skipped = 0;   // pipelined FGMRES loop: speculative applications issued / discarded / iterations run without one (TP_DEBUG)
    static constexpr int H_PIN = 1024;   // doubles of pinned, device-mapped host memory the reductions write their results to
    double *h_pin = nullptr;
    hipEvent_t ev_h = nullptr;           // recorded behind the reductions of an orthogonalisation (pipelined FGMRES loop)
    // line search of newton() (tp_options.ls_kind = 1): the saved iterate u0 (b*ntot doubles, allocated by the first bt solve) and
    // what tp_ls_info / tp_ls_history report about the last solve
    tp::DBuf<double> ls_u0;
    std::vector<double> ls_lambda, ls_fnorm;
    std::vector<int32_t> ls_trials;
    long ls_evals = 0, ls_nonfinite = 0;
    // Eisenstat-Walker (tp_options.ksp_ew; tp_ew.hpp): per linear solve of the last Newton solve eta_k, ||F_k||, rho_k, the Krylov
    // iterations and reason (tp_ew_history), and the counters of tp_ew_info since tp_create.  Host data only.
    std::vector<double> ew_rtol, ew_fnorm, ew_lresid;
    std::vector<int32_t> ew_kits, ew_kreason;
    long ew_solves = 0, ew_lsolves = 0, ew_safeguard = 0;
    tp_ksp_monitor_fn monitor = nullptr;      // per-field true-residual monitor (ksp_monitor_residuals)
    void *monitor_user = nullptr;
    ~tp_ctx();
};

namespace tp {
// Host <-> device copy ordered on the context's stream (after everything queued there) and complete on return.  The context's
// streams are non-blocking and no call goes to the legacy default stream (see DBuf::alloc).
inline void copy_sync(tp_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    TP_HIP(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    TP_HIP(hipStreamSynchronize(c->stream));
}
// ---- launch wrappers implemented in the .hip files ------------------------------------------------
// assembly
void compute_trans(tp_ctx *c);
void accum_old(tp_ctx *c);
void assemble(tp_ctx *c, bool want_jac, bool want_schur);
void well_rates(tp_ctx *c);
// Dirichlet sides: bc_set checks and stores one side (kind 0 removes it), bc_trans refills the half-cell transmissibilities of
// the set sides from K (tp_finalize_fields), assemble_bc adds the boundary faces to R, slot 0 of J and the diagonal of S~
// (assemble calls it behind the cell kernel when a side is set), bc_flux sums each side's last contributions on the host
void bc_set(tp_ctx *c, int side, int kind, const double *values, long nfaces);
void bc_trans(tp_ctx *c);
void assemble_bc(tp_ctx *c, bool want_jac, bool want_schur);
void bc_flux(tp_ctx *c, double *out);
// completed wells (tp_wells.hip): wells_set checks and stores them (0 wells removes them), wells_control changes one well's targets,
// wells_rho refreshes the head densities from the old state (accum_old calls it), wells_assemble adds the perforations to R, the
// diagonal block of J and the diagonal of S~ and stores the rank-1 factors (assemble calls it behind the source kernel)
void wells_set(tp_ctx *c, int nw, const tp_well *wells, int np, const tp_perf *perfs);
void wells_control(tp_ctx *c, int w, double rate, double limit, int shut);
void wells_rho(tp_ctx *c);
void wells_assemble(tp_ctx *c, bool want_jac, bool want_schur);
void wells_info(tp_ctx *c, tp_well_state *out);
void wells_perf_rates(tp_ctx *c, double *rate, double *water, double *oil);
void wells_factors(tp_ctx *c, double *fc, double *fb);
// The Krylov operator A = J + sum_w c_w b_w^T on the assembled Jacobian: y = A x (halo: through spmv_block_halo) and r = b - A x over
// all b columns.  The outer Krylov methods and tp_spmv use these two; the preconditioner's own products keep the 7-point J.
void krylov_apply(tp_ctx *c, double *x, double *y, bool halo = true);
void krylov_resid(tp_ctx *c, const double *b, const double *x, double *r);
void wells_apply_only(tp_ctx *c, const double *x, double *y);     // y += sum_w c_w (b_w . x): the kernel alone (tp_time_kernel)
// graded grid (tp_set_spacing): spacing_set checks and stores the widths (all null: back to uniform) and marks the fields as not
// finalised; conduction_strengths gives the per-axis coarsening strengths of amg_T and the pc_ctr hierarchy on grid `gam`: |E|/h_a^2,
// or with spacing the mean of |e|/(d_P + d_M) over the axis's interior faces
// saturation functions (tp_set_saturation_functions): checks every range, stores the setting (null, or linear without p_c: the
// default) and recomputes the old state's accumulation; satfn_defaults: the values tp_saturation_info reports when none is set
void satfn_set(tp_ctx *c, const tp_satfn *sat);
tp_satfn satfn_defaults();
void spacing_set(tp_ctx *c, const double *h0, long n0, const double *h1, long n1, const double *h2, long n2);
void conduction_strengths(const tp_ctx *c, const GridDev &gam, double sg[3]);
// vectors / reductions (vectors are b field planes of ntot; reductions run over owned cells only)
void vec_zero(tp_ctx *c, double *x, long n);
void vec_copy(tp_ctx *c, const double *x, double *y, long n);
void vec_axpy_owned(tp_ctx *c, int nf, double a, const double *x, double *y);            // y += a x
void vec_scale_to(tp_ctx *c, int nf, double a, const double *x, double *y);             // y = a x (owned)
void scale_plane(tp_ctx *c, const tp::GridDev &g, double a, double *x);                 // x *= a (owned cells of one plane of g)
void multi_dot(tp_ctx *c, int nf, const double *V, long vstride, int k, const double *w, const double *w2,
               double *host_out);   // host_out[i] = <V_i, w>, i<k ; host_out[k] = <w2,w2> if w2
void multi_axpy(tp_ctx *c, int nf, const double *V, long vstride, int k, const double *hcoef_host, double sign,
                double *w);          // w += sign * sum_i h_i V_i
double norm2(tp_ctx *c, int nf, const double *x);
void multi_norm2sq(tp_ctx *c, int nf, int nvec, const double *const *x, double *host_out);   // host_out[i] = <x_i, x_i>
// TP_PIN (default 1; read once per process): the reductions' sums reach the host through the pinned, device-mapped buffer h_pin
bool tp_use_pin();
// h = V^T w ; w -= V h ; host_out[0..k-1] = h, host_out[k] = ||w||^2  (one host sync).  host_out = nullptr (only where
// orthogonalize_can_split): enqueue only; orthogonalize_wait then hands the sums over, ||w||^2 stays at orthogonalize_norm_dev
void orthogonalize(tp_ctx *c, int nf, const double *V, long vstride, int k, double *w, double *host_out);
bool orthogonalize_can_split(const tp_ctx *c, int k);
const double *orthogonalize_norm_dev(const tp_ctx *c, int k);
void orthogonalize_wait(tp_ctx *c, int k, double *host_out);
// the same step with the refinement mode and eta given by the caller instead of tp_options (tp_vec_orth_step); *refined = the
// device flag of this step
void orthogonalize_mode(tp_ctx *c, int nf, const double *V, long vstride, int k, double *w, int mode, double eta, double *host_out,
                        int *refined);
void reorth_check_options(const tp_options &o);
void pc_order_check_options(const tp_options &o);
void vec_scale_dev_norm(tp_ctx *c, int nf, const double *n2_dev, double *x);   // x *= 1/sqrt(*n2_dev) (owned)
// fp32 Krylov bases (tp_options.ksp_basis_single; tp_linalg.hip): Vs points at compact float vectors `vstride` entries apart
long basis_stride(const tp_ctx *c);                                              // b*nown rounded up to 64 entries
void basis_round_store(tp_ctx *c, int nf, double *z, float *slot);             // slot = (float) z ; z = (double) slot
void basis_scale_store(tp_ctx *c, int nf, double a, const double *x, double *y, float *slot);   // slot = (float)(a x) ; y = (double) slot
void basis_scale_store_dev(tp_ctx *c, int nf, const double *n2_dev, double *x, float *slot);    // the same in place, a = 1/sqrt(*n2_dev)
void multi_dot_s(tp_ctx *c, int nf, const float *Vs, long vstride, int k, const double *w, double *host_out);
void multi_axpy_s(tp_ctx *c, int nf, const float *Vs, long vstride, int k, const double *hcoef_host, double sign, double *w);
void orthogonalize_s(tp_ctx *c, int nf, const float *Vs, long vstride, int k, double *w, double *host_out);
// line search (tp_options.ls_kind = 1): host_out = {||dx||^2, max|dx_f| f < 3} over owned cells, all slabs (one host sync);
// u = u0 - lambda dx on owned cells of all fields
void ls_step_stats(tp_ctx *c, const double *dx, double *host_out);
void ls_trial(tp_ctx *c, const double *u0, const double *dx, double lambda, double *u);
void field_minmax(tp_ctx *c, const double *x, double *lo, double *hi);
void field_clamp01(tp_ctx *c, double *x);
// stencil operators
void spmv_block(tp_ctx *c, const double *J, const double *x, double *y);
void spmv_block_halo(tp_ctx *c, const double *J, double *x, double *y);          // exchange x's halos, y = J x; interior overlaps the exchange                 // y = J x
void resid_block_cols(tp_ctx *c, const double *J, const double *x, const double *y, int ncols, double *r);  // r = x - J[:, :ncols] y
void spmv_scalar(tp_ctx *c, const GridDev &g, const Stencil &A, const double *x, double *y, double alpha, const double *z);  // y = z + alpha*A x (z may be null)
void decouple(tp_ctx *c);
void selfp_build(tp_ctx *c);                                                           // S7, w/diag(Sp) into spbuf
void selfp_post(tp_ctx *c, const double *b, const double *x, double *y);                  // y = x + w D^-1 (b - Sp x)
void stage1_rhs(tp_ctx *c, const double *x, int q, double *out);                        // out = x_q - d_q x_s
void stage_rhs(tp_ctx *c, const double *x, const double *y, double *out);                // out_q = [x - J y]_q - d_q [x - J y]_s, q < npri
void row_rhs(tp_ctx *c, const double *x, const double *y, double *o1);                   // the plane o1 = [x - J y]_1, all b columns of y
// ILU
void ilu_setup(tp_ctx *c);
void ilu_factor(tp_ctx *c);
void ilu_layout(tp_ctx *c, int32_t out[8]);
long ilu_factor_bytes(tp_ctx *c);
// x = addto + M^-1 r ; only the first nadd fields of addto are read, the others count as zero (< 0: all fields)
void ilu_solve(tp_ctx *c, const double *r, double *x, const double *addto, int nadd = -1);
// AMG.  slabs: each rank's owned global planes along axis 2 (rank_slabs; empty: not distributed); a level stays on the slabs
// while it has more than gather_cells cells (< 0: never), the tail kernel starts at the first replicated level of <= tail_cells
AmgPlan amg_plan(const GridDev &g0, const double strength[3], const tp_options &o, int me,
                 const std::vector<std::pair<int, int>> &slabs, long gather_cells, long tail_cells);
std::vector<std::pair<int, int>> rank_slabs(const tp_ctx *c);
void amg_build(tp_ctx *c, Amg *&amg, const GridDev &g0, const double strength[3], long gather_cells);
void amg_setup(tp_ctx *c, Amg *amg, const Stencil &A0);
void amg_vcycle(tp_ctx *c, Amg *amg, const double *b, double *x);
void amg_line_check_options(const tp_options &o, int nranks);      // what amg_line_levels excludes (throws, naming both options)
void amg_line_info(const Amg *amg, int64_t out[4]);
void amg_gs_check_options(const tp_options &o, int nranks);        // what amg_gs_levels excludes (throws, naming both options)
void amg_gs_info(const Amg *amg, int64_t out[4]);
bool amg_resolve_trunc(tp_ctx *c, Amg *amg);      // waits for the set-up's dominance ratios; true if the cycle shape changed
// system AMG (2x2 blocks on (p,T))
void bamg_build(tp_ctx *c, BAmg *&amg, const GridDev &g0, const double strength[3]);
void bamg_setup(tp_ctx *c, BAmg *amg, const BStencil &A0);
void bamg_vcycle(tp_ctx *c, BAmg *amg, const double *b, double *x);     // b, x: 2 planes, stride = ntot of the grid
// comm
void halo_exchange(tp_ctx *c, const GridDev &g, double *x, int nf, long fstride);
void halo_exchange_raw(tp_ctx *c, const GridDev &g, void *x, int nf, size_t fstride_bytes, size_t elem_bytes);
void gather_ranges(tp_ctx *c, void *global, long np, const std::vector<std::pair<int, int>> &ranges, int nslots,
                   size_t slot_stride_bytes, size_t elem_bytes);
void allreduce_sum(tp_ctx *c, double *dev, int n);
void allreduce_max(tp_ctx *c, double *dev, int n);
void slab_of(const tp_ctx *c, int rank, int &lo, int &hi);
// recording of pc_apply programs (tp_solver.hip): close / reopen the current stream-capture segment around an exchange
void seg_begin(tp_ctx *c);
void seg_end(tp_ctx *c);
// gather `nplanes` slab-distributed cell planes into arrays on the global grid (every rank gets all slabs)
void gather_slabs(tp_ctx *c, const double *local, long lstride, double *global, long gstride, int nplanes);
// inner Krylov solve of a stage-1 block (tp_inner.hip): out = K(op) rhs with the V-cycle `prec` as (right) preconditioner.
// s1_ksp preonly: prec(rhs, out) and nothing else.  No host synchronisation: capturable.
void inner_ensure(tp_ctx *c);         // workspace for the current options (called by ensure_work)
void inner_check_options(const tp_options &o);
void inner_reset_stats(tp_ctx *c);
void inner_solve(tp_ctx *c, const InnerOp &op, const std::function<void(const double *, double *)> &prec, const double *rhs,
                 double *out, int nplanes);
int vcycles_per_apply(const tp_ctx *c);   // V-cycles one pc_apply launches
// solver
void resolve_cycle_shapes(tp_ctx *c);     // fix the AMG truncation levels after a set-up (host wait; never in a capture)
void ensure_work(tp_ctx *c);          // scratch vectors w1..w4, dx of the preconditioner / Krylov loops
void pc_setup(tp_ctx *c);
void stage1_apply(tp_ctx *c, const double *x, double *y, bool zero_secondary = true);
void pc_apply(tp_ctx *c, const double *x, double *y);
// the composite's temperature stage (tp_options.pc_ctr): what the option excludes (throws, naming both options), and the stage on
// its own, y_1 = V(A_TT) x_1 with every other field of y zero
// the factorisation of the Schur split on (p,T) (tp_options.schur_fact, schur_scale): what it excludes (throws, naming both
// options), and the host counters of tp_schur_info for `stages` stage-1 sequences issued or replayed
void pc_schur_fact_check_options(const tp_options &o);
void schur_count(tp_ctx *c, int stages);
void pc_ctr_check_options(const tp_options &o, int nranks);
void ctr_apply(tp_ctx *c, const double *x, double *y);
// rtol: the relative tolerance of THIS solve (tp_fgmres / tp_bcgs pass tp_options.ksp_rtol, newton() the same or, under ksp_ew, eta_k):
// every reader of the tolerance -- the FGMRES loop in both basis representations, the speculation margin, the fp32 basis' true-residual test, the
// BiCGStab latch on the device -- follows it; tp_options is never written
int fgmres(tp_ctx *c, const double *b, double *x, int *its, double *rnorm, double rtol);
// outer BiCGStab (tp_bcgs.hip): same contract as fgmres; reasons 2, -3, -5 (breakdown), -9
int bcgs(tp_ctx *c, const double *b, double *x, int *its, double *rnorm, double rtol);
void bcgs_check_options(const tp_options &o);
void ksp_info(tp_ctx *c, int64_t out[4]);
void basis_single_check_options(const tp_options &o);
void basis_single_release(tp_ctx *c);     // frees the FGMRES bases of both representations (the option changed)
void ls_check_options(const tp_options &o);
double ls_next_lambda(int order, double g0, double f0, double lam, double phi, bool have_prev, double lam_p, double phi_p);
void newton(tp_ctx *c, tp_solve_info *info);
}  // namespace tp
