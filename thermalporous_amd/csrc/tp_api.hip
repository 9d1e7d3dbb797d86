// extern "C" surface of libthermalporous_hip.so (declared in include/thermalporous_hip.h) and the RCCL
// slab communication (halo exchange over xGMI point-to-point links, batched dot-product all-reduce).
#include "tp_common.hpp"
#include <rccl/rccl.h>
#include <cmath>
#include <algorithm>
#include <map>
#include <utility>
#include <mutex>
#include <condition_variable>

namespace tp {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

#define TP_NCCL(call)                                                                          \
    do {                                                                                       \
        ncclResult_t r_ = (call);                                                              \
        if (r_ != ncclSuccess)                                                                 \
            throw tp::Error(std::string(#call) + " failed: " + ncclGetErrorString(r_));        \
    } while (0)

// ---- in-process slab group: N contexts (threads) on one GPU exchange through device-to-device copies ------
// Same call sequence and same buffer arithmetic as the RCCL path below; exists so that the slab
// algorithm can be validated end to end on a single GPU (tests/test_gpu_slabs.py).
struct LocalGroup {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long generation = 0;
    std::vector<const void *> ptr;       // published buffer of every rank
    std::vector<std::vector<double>> red;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long gen = generation;
        if (++arrived == n) { arrived = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen; });
    }
};

static void lg_publish(tp_ctx *c, const void *p) {
    TP_HIP(hipStreamSynchronize(c->stream));          // my data is complete before anybody reads it
    c->lgroup->ptr[c->grid.rank] = p;
    c->lgroup->barrier();
}
static void lg_done(tp_ctx *c) {
    TP_HIP(hipStreamSynchronize(c->stream));          // my copies are complete before sources may change
    c->lgroup->barrier();
}

// One 1-cell halo plane per side along axis 2; each plane of each field is contiguous, so the
// exchange is 2*nf send/recv pairs in one RCCL group on the compute stream (<= 2 neighbours, one
// xGMI link each).  Element size 8 (vectors, fp64 operators) or 4 (fp32 AMG operators); `g` is the
// grid of the array being exchanged (the slab itself, or one of its distributed AMG levels).
struct HaloPub { const char *p; size_t fstride; int n2; };

// While a pc_apply program is being recorded (tp_solver.hip) an exchange closes the current capture segment (which is
// instantiated and launched, so the recording pass computes the real result), runs eagerly, is remembered as a host
// closure, and a new segment is opened behind it.  `call` re-enters the same function with recording suspended.
#define TP_COMM_RECORD(c, call)                                                     \
    do {                                                                            \
        if ((c)->rec && !(c)->rec_in_comm) {                                        \
            seg_end(c);                                                             \
            (c)->rec->steps.push_back({GraphExec(), [=]() { call; }});              \
            (c)->rec_in_comm = true;                                                \
            try { call; } catch (...) { (c)->rec_in_comm = false; throw; }          \
            (c)->rec_in_comm = false;                                               \
            seg_begin(c);                                                           \
            return;                                                                 \
        }                                                                           \
    } while (0)


void halo_exchange_raw(tp_ctx *c, const GridDev &g, void *x_, int nf, size_t fstride, size_t elem) {
    if (!c->dist) return;
    TP_REQUIRE(g.n2 >= 1, "halo exchange of an empty slab");
    TP_COMM_RECORD(c, halo_exchange_raw(c, g, x_, nf, fstride, elem));
    char *x = (char *)x_;
    const int lo = c->grid.rank - 1, hi = c->grid.rank + 1;
    const size_t pb = (size_t)g.np * elem;       // bytes per plane
    if (c->lgroup) {
        HaloPub mine{x, fstride, g.n2};
        lg_publish(c, &mine);
        for (int f = 0; f < nf; ++f) {
            char *p = x + (size_t)f * fstride;
            if (g.nb_lo) {       // neighbour's last owned plane -> my lower halo
                const HaloPub *q = (const HaloPub *)c->lgroup->ptr[lo];
                TP_HIP(hipMemcpyAsync(p, q->p + (size_t)f * q->fstride + pb * q->n2, pb, hipMemcpyDeviceToDevice, c->stream));
            }
            if (g.nb_hi) {       // neighbour's first owned plane -> my upper halo
                const HaloPub *q = (const HaloPub *)c->lgroup->ptr[hi];
                TP_HIP(hipMemcpyAsync(p + pb * (g.n2 + 1), q->p + (size_t)f * q->fstride + pb, pb, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        lg_done(c);
        return;
    }
    ncclComm_t comm = (ncclComm_t)c->comm;
    const ncclDataType_t dt = elem == 8 ? ncclDouble : ncclFloat;
    TP_REQUIRE(elem == 8 || elem == 4, "halo element size");
    TP_NCCL(ncclGroupStart());
    for (int f = 0; f < nf; ++f) {
        char *p = x + (size_t)f * fstride;
        if (g.nb_lo) {
            TP_NCCL(ncclSend(p + pb, g.np, dt, lo, comm, c->stream));                      // first owned plane
            TP_NCCL(ncclRecv(p, g.np, dt, lo, comm, c->stream));                           // lower halo
        }
        if (g.nb_hi) {
            TP_NCCL(ncclSend(p + pb * g.n2, g.np, dt, hi, comm, c->stream));               // last owned plane
            TP_NCCL(ncclRecv(p + pb * (g.n2 + 1), g.np, dt, hi, comm, c->stream));         // upper halo
        }
    }
    TP_NCCL(ncclGroupEnd());
}

void halo_exchange(tp_ctx *c, const GridDev &g, double *x, int nf, long fstride) {
    halo_exchange_raw(c, g, x, nf, (size_t)fstride * sizeof(double), sizeof(double));
}

// In-place all-gather on a global-grid array every rank holds: rank r owns global planes
// [ranges[r].first, ranges[r].second) of each of the nslots planes-sets and broadcasts them to everybody.
void gather_ranges(tp_ctx *c, void *global_, long np, const std::vector<std::pair<int, int>> &ranges, int nslots,
                   size_t slot_stride, size_t elem) {
    TP_REQUIRE(c->dist, "gather_ranges without a communicator");
    TP_COMM_RECORD(c, gather_ranges(c, global_, np, ranges, nslots, slot_stride, elem));
    char *global = (char *)global_;
    const size_t pb = (size_t)np * elem;
    if (c->lgroup) {
        lg_publish(c, global);
        for (int r = 0; r < c->grid.nranks; ++r) {
            if (r == c->grid.rank) continue;
            const char *src = (const char *)c->lgroup->ptr[r];
            const size_t off = pb * (ranges[r].first + 1), len = pb * (ranges[r].second - ranges[r].first);
            for (int s = 0; s < nslots; ++s)
                TP_HIP(hipMemcpyAsync(global + s * slot_stride + off, src + s * slot_stride + off, len,
                                      hipMemcpyDeviceToDevice, c->stream));
        }
        lg_done(c);
        return;
    }
    ncclComm_t comm = (ncclComm_t)c->comm;
    const ncclDataType_t dt = elem == 8 ? ncclDouble : ncclFloat;
    TP_NCCL(ncclGroupStart());
    for (int s = 0; s < nslots; ++s)
        for (int r = 0; r < c->grid.nranks; ++r) {
            char *buf = global + s * slot_stride + pb * (ranges[r].first + 1);
            TP_NCCL(ncclBroadcast(buf, buf, (size_t)np * (ranges[r].second - ranges[r].first), dt, r, comm, c->stream));
        }
    TP_NCCL(ncclGroupEnd());
}

void slab_of(const tp_ctx *c, int rank, int &lo, int &hi) {
    const int base = c->grid.gn2 / c->grid.nranks, rem = c->grid.gn2 % c->grid.nranks;
    lo = rank * base + std::min(rank, rem);
    hi = lo + base + (rank < rem ? 1 : 0);
}

// Every rank broadcasts the owned part of each of its planes into the same place of everybody's global
// array (uneven slabs: one ncclBroadcast per (plane, root) inside one group).
void gather_slabs(tp_ctx *c, const double *local, long lstride, double *global, long gstride, int nplanes) {
    TP_REQUIRE(c->dist, "gather_slabs without a communicator");
    TP_COMM_RECORD(c, gather_slabs(c, local, lstride, global, gstride, nplanes));
    const long np = c->g.np;
    if (c->lgroup) {
        // NOTE: lstride is the same on every rank only when it is expressed in this rank's ntot; ranks
        // publish (pointer, stride) pairs
        struct Pub { const double *p; long stride; };
        Pub mine{local, lstride};
        lg_publish(c, &mine);
        for (int r = 0; r < c->grid.nranks; ++r) {
            int lo, hi;
            slab_of(c, r, lo, hi);
            const Pub *pr = (const Pub *)c->lgroup->ptr[r];
            for (int p = 0; p < nplanes; ++p)
                TP_HIP(hipMemcpyAsync(global + (long)p * gstride + np * (lo + 1), pr->p + (long)p * pr->stride + np,
                                      sizeof(double) * np * (hi - lo), hipMemcpyDeviceToDevice, c->stream));
        }
        lg_done(c);
        return;
    }
    ncclComm_t comm = (ncclComm_t)c->comm;
    TP_NCCL(ncclGroupStart());
    for (int p = 0; p < nplanes; ++p)
        for (int r = 0; r < c->grid.nranks; ++r) {
            int lo, hi;
            slab_of(c, r, lo, hi);
            double *dst = global + (long)p * gstride + np * (lo + 1);
            // sendbuff is only read on the root; elsewhere pass the (valid, large enough) receive buffer
            const double *src = (r == c->grid.rank) ? local + (long)p * lstride + np : dst;
            TP_NCCL(ncclBroadcast(src, dst, (size_t)np * (hi - lo), ncclDouble, r, comm, c->stream));
        }
    TP_NCCL(ncclGroupEnd());
}

// in-process group: copy out, barrier, combine in rank order (identical result on every rank), barrier, copy in
template <class Op>
static void lg_allreduce(tp_ctx *c, double *dev, int n, Op combine) {
    LocalGroup *G = c->lgroup;
    std::vector<double> &mine = G->red[c->grid.rank];
    mine.resize(n);
    TP_HIP(hipMemcpyAsync(mine.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    TP_HIP(hipStreamSynchronize(c->stream));
    G->barrier();
    std::vector<double> acc(n, 0.0);
    for (int r = 0; r < G->n; ++r)
        for (int i = 0; i < n; ++i) acc[i] = combine(acc[i], G->red[r][i]);
    G->barrier();                                  // everybody has read before anybody overwrites
    TP_HIP(hipMemcpyAsync(dev, acc.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    TP_HIP(hipStreamSynchronize(c->stream));
}

void allreduce_sum(tp_ctx *c, double *dev, int n) {
    if (!c->dist || n <= 0) return;
    TP_COMM_RECORD(c, allreduce_sum(c, dev, n));
    if (c->lgroup) { lg_allreduce(c, dev, n, [](double a, double b) { return a + b; }); return; }
    TP_NCCL(ncclAllReduce(dev, dev, n, ncclDouble, ncclSum, (ncclComm_t)c->comm, c->stream));
}

// element-wise maximum over the ranks (non-negative doubles: the AMG dominance ratios)
void allreduce_max(tp_ctx *c, double *dev, int n) {
    if (!c->dist || n <= 0) return;
    TP_COMM_RECORD(c, allreduce_max(c, dev, n));
    if (c->lgroup) { lg_allreduce(c, dev, n, [](double a, double b) { return std::max(a, b); }); return; }
    TP_NCCL(ncclAllReduce(dev, dev, n, ncclDouble, ncclMax, (ncclComm_t)c->comm, c->stream));
}

// the AMG hierarchies follow the options and the fields they were built from: dropped, pc_setup rebuilds them
static void drop_hierarchies(tp_ctx *c) {
    delete c->amg_p; c->amg_p = nullptr;
    delete c->amg_T; c->amg_T = nullptr;
    delete c->bamg; c->bamg = nullptr;
    delete c->amg_ctr; c->amg_ctr = nullptr;
}

}  // namespace tp

tp_ctx::~tp_ctx() {
    if (tp_switch_int(TP_SW_DEBUG) >= 1 && spec_issued + spec_skipped > 0)
        fprintf(stderr, "[tp] pipelined FGMRES: %ld speculative applications issued, %ld discarded, %ld iterations without one\n",
                spec_issued, spec_wasted, spec_skipped);
    for (auto *v : vecs) delete v;
    for (auto *f : fbatches) delete f;
    tp::drop_hierarchies(this);
    pc_programs.clear();                 // (the graph segments go before the stream they were captured on)
    if (comm) ncclCommDestroy((ncclComm_t)comm);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (int i = 0; i < 2; ++i) {
        if (aux[i]) (void)hipStreamDestroy(aux[i]);
        if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (stream) (void)hipStreamDestroy(stream);
    if (h_pin) (void)hipHostFree(h_pin);
    if (ev_h) (void)hipEventDestroy(ev_h);
}

using namespace tp;

#define TP_API_BEGIN try {
#define TP_API_END                                   \
    return 0;                                        \
    }                                                \
    catch (const std::exception &e) {                \
        tp::set_error(e.what());                     \
        return -1;                                   \
    }                                                \
    catch (...) {                                    \
        tp::set_error("unknown C++ exception");      \
        return -1;                                   \
    }

static void derive_params(tp_ctx *c) {
    const tp_params &p = c->prm;
    DevPrm &d = c->dprm;
    d.ko = p.ko; d.kw = p.kw; d.kr = p.kr; d.c_v_w = p.c_v_w; d.c_v_o = p.c_v_o; d.c_r = p.c_r;
    d.rho_r = p.rho_r; d.T_inj = p.T_inj; d.g = p.g; d.U = p.U;
    const double SG = 141.5 / (p.API + 131.5);               // physicalparameters.py:39-40
    d.rho_ref = SG * 999.0;
    d.mu_o_coef = 1e-3 * std::pow(10.0, -0.8021 * p.API + 23.8765);   // :52-57
    d.mu_o_exp = 0.31458 * p.API + (-9.21592);
    if (c->nph == 2) {                                        // twophase.py:142-147
        d.w0 = p.T_prod;
        d.w2 = p.T_prod * (p.c_v_w * (1.0 - p.S_o) + p.c_v_o * p.S_o);
    } else {                                                  // m_w = 1 (singlephase.py:26,112-115)
        d.w0 = 1.0;
        d.w2 = 0.0;
    }
}

static DBuf<double> &vec_of(tp_ctx *c, int id) {
    TP_REQUIRE(id >= 0 && id < (int)c->vecs.size(), "bad vector id");
    return *c->vecs[id];
}

// every option against its range and against the options it excludes (each check stands beside its feature); tp_create and
// tp_set_options are the only places that store a tp_options, so whatever a context holds has passed this
static void check_options(const tp_options &o, int nranks) {
    inner_check_options(o);
    bcgs_check_options(o);
    basis_single_check_options(o);
    reorth_check_options(o);
    pc_order_check_options(o);
    pc_schur_fact_check_options(o);
    pc_ctr_check_options(o, nranks);
    ls_check_options(o);
    ew_check_options(o);
    amg_line_check_options(o, nranks);
    amg_gs_check_options(o, nranks);
}

extern "C" {

const char *tp_last_error(void) { return tp::g_err.c_str(); }
int tp_version(void) { return 101; }
int tp_switch_count(void) { return TP_SW_COUNT; }
int tp_switch_entry(int i, const char **name, const char **kind, const char **dflt, const char **when, const char **effect) {
    TP_API_BEGIN
    TP_REQUIRE(i >= 0 && i < TP_SW_COUNT && name && kind && dflt && when && effect, "tp_switch_entry: bad index or null argument");
    const tp_switch_info &s = tp_switch_infos[i];
    *name = s.name, *kind = s.kind, *dflt = s.dflt, *when = s.when, *effect = s.effect;
    TP_API_END
}

int tp_create(const tp_grid *grid, const tp_params *prm, const tp_options *opt, int device, tp_ctx **out) {
    TP_API_BEGIN
    TP_REQUIRE(grid && prm && opt && out, "null argument");
    TP_REQUIRE(grid->n0 >= 1 && grid->n1 >= 1 && grid->n2 >= 1, "empty grid");
    TP_REQUIRE(grid->nphase == 1 || grid->nphase == 2, "nphase must be 1 or 2");
    TP_REQUIRE(grid->off2 >= 0 && grid->off2 + grid->n2 <= grid->gn2, "slab outside the global grid");
    TP_REQUIRE((long)grid->n0 * grid->n1 * (grid->n2 + 2) < (1L << 31), "slab too large for int32 block indices");
    int ndev = 0;
    TP_HIP(hipGetDeviceCount(&ndev));
    TP_REQUIRE(ndev > 0, "no HIP device: the thermalporous hot path has no CPU fallback");
    TP_REQUIRE(device >= 0 && device < ndev, "bad device ordinal");
    check_options(*opt, grid->nranks);
    TP_HIP(hipSetDevice(device));
    tp_ctx *c = new tp_ctx();
    c->grid = *grid; c->prm = *prm; c->opt = *opt; c->device = device;
    c->nph = grid->nphase; c->b = grid->nphase + 1;
    c->g = make_grid(grid->n0, grid->n1, grid->n2, grid->gn2, grid->off2);
    c->gfull = make_grid(grid->n0, grid->n1, grid->gn2, grid->gn2, 0);
    c->vol = grid->h[0] * grid->h[1] * grid->h[2];
    derive_params(c);
    TP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));      // (never tied to the legacy stream: tp_common.hpp)
    // coherent (fine-grained) host memory and a system-scope release at the event: the host reads what the reduction kernel
    // wrote after waiting for ev_h only, not for the stream
    TP_HIP(hipHostMalloc((void **)&c->h_pin, sizeof(double) * tp_ctx::H_PIN, hipHostMallocMapped | hipHostMallocCoherent));
    TP_HIP(hipEventCreateWithFlags(&c->ev_h, hipEventDisableTiming | hipEventReleaseToSystem));
    for (int i = 0; i < 2; ++i) {
        TP_HIP(hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking));
        TP_HIP(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    TP_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    TP_HIP(hipEventCreate(&c->ev0));
    TP_HIP(hipEventCreate(&c->ev1));
    const size_t nt = (size_t)c->g.ntot, B = (size_t)c->b;
    c->phi.alloc(nt); c->kTs.alloc(nt);
    for (int a = 0; a < 3; ++a) { c->K[a].alloc(nt); c->TK[a].alloc(nt); }
    c->u.alloc(B * nt); c->u_old.alloc(B * nt); c->acc_old.alloc(B * nt); c->R.alloc(B * nt);
    c->J.alloc(7 * B * B * nt);
    if (schur_of(*opt)) c->Sm.alloc(7 * nt);
    *out = c;
    TP_API_END
}

int tp_destroy(tp_ctx *ctx) {
    TP_API_BEGIN
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        // (this context's streams only: a device-wide synchronisation would wait for -- and, while one of them captures, fail on --
        // the other slab contexts of an in-process group)
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (int i = 0; i < 2; ++i)
            if (ctx->aux[i]) (void)hipStreamSynchronize(ctx->aux[i]);
        delete ctx;
    }
    TP_API_END
}

int tp_set_options(tp_ctx *c, const tp_options *opt) {
    TP_API_BEGIN
    TP_REQUIRE(c && opt, "null argument");
    TP_REQUIRE(opt->ilu_levels == 0 || opt->ilu_levels == 1, "ilu_levels must be 0 or 1");
    TP_REQUIRE(!(opt->ilu_single && opt->ilu_levels), "ilu_single (fp32 factor) is implemented for block-ILU(0): not with ilu_levels 1");
    TP_REQUIRE(!(opt->ilu_single && opt->ilu_whole), "ilu_single (fp32 factor) is implemented for one tile per block: not with ilu_whole");
    check_options(*opt, c->grid.nranks);
    const bool tile_changed = opt->ilu_t1 != c->opt.ilu_t1 || opt->ilu_t2 != c->opt.ilu_t2 || opt->ilu_t0 != c->opt.ilu_t0 ||
                              opt->ilu_levels != c->opt.ilu_levels || opt->ilu_whole != c->opt.ilu_whole ||
                              (opt->ilu_single != 0) != (c->opt.ilu_single != 0) ||
                              std::memcmp(opt->ilu_block, c->opt.ilu_block, sizeof(opt->ilu_block)) != 0;
    const bool amg_changed = opt->amg_min_cells != c->opt.amg_min_cells || opt->pc_kind != c->opt.pc_kind ||
                             opt->amg_nu != c->opt.amg_nu || opt->amg_full_levels != c->opt.amg_full_levels ||
                             opt->amg_coarse_pre != c->opt.amg_coarse_pre || opt->amg_coarse_post != c->opt.amg_coarse_post ||
                             opt->amg_tail_post != c->opt.amg_tail_post || opt->amg_mid_skip != c->opt.amg_mid_skip ||
                             opt->amg_dom_tau != c->opt.amg_dom_tau || opt->amg_line_levels != c->opt.amg_line_levels ||
                             opt->amg_gs_levels != c->opt.amg_gs_levels || opt->amg_gs_sweeps != c->opt.amg_gs_sweeps ||
                             opt->amg_single != c->opt.amg_single || opt->amg_gather_cells != c->opt.amg_gather_cells ||
                             opt->schur_a11 != c->opt.schur_a11 || opt->fs_additive != c->opt.fs_additive;
    // the FGMRES bases exist in one representation at a time: the next solve allocates the one the option asks for
    if ((opt->ksp_basis_single != 0) != (c->opt.ksp_basis_single != 0)) basis_single_release(c);
    if (opt->ls_kind == 0) c->ls_u0.free();          // the saved iterate belongs to the bt search: the next bt solve allocates it
    c->opt = *opt;
    if (tile_changed) c->ilu.slots = 0;
    if (amg_changed) drop_hierarchies(c);
    if (!opt->pc_ctr) { delete c->amg_ctr; c->amg_ctr = nullptr; }      // the T stage's hierarchy lives while its option is on
    if (schur_of(*opt) && c->Sm.n == 0) c->Sm.alloc((size_t)7 * c->g.ntot);
    c->pc_ready = false;
    c->graph_epoch++;            // any option may change the captured kernel sequence: drop the pc_apply graphs
    TP_API_END
}

int tp_comm_unique_id(void *id128) {
    TP_API_BEGIN
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    TP_NCCL(ncclGetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    TP_API_END
}

int tp_comm_init(tp_ctx *c, const void *id128) {
    TP_API_BEGIN
    TP_REQUIRE(c && id128, "null argument");
    TP_REQUIRE(c->grid.nranks >= 1, "bad nranks");     // a 1-rank communicator is legal (exercises the RCCL calls on one GPU)
    TP_REQUIRE(!c->graded, "tp_comm_init: this context has spacing (tp_set_spacing): graded grids exist on one slab without a communicator");
    TP_REQUIRE(c->wells.nw == 0, "tp_comm_init: this context has wells (tp_set_wells): completed wells exist on one slab without a communicator");
    TP_HIP(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclComm_t comm;
    TP_NCCL(ncclCommInitRank(&comm, c->grid.nranks, id, c->grid.rank));
    c->comm = (ncclComm *)comm;
    c->dist = true;
    int lo, hi;
    slab_of(c, c->grid.rank, lo, hi);
    TP_REQUIRE(lo == c->grid.off2 && hi - lo == c->grid.n2, "slab of this rank does not follow the library's partition rule");
    TP_API_END
}

int tp_local_group_create(int32_t nranks, void **group) {
    TP_API_BEGIN
    TP_REQUIRE(nranks >= 2 && group, "bad arguments");
    LocalGroup *G = new LocalGroup();
    G->n = nranks;
    G->ptr.assign(nranks, nullptr);
    G->red.resize(nranks);
    *group = G;
    TP_API_END
}

int tp_local_group_destroy(void *group) {
    TP_API_BEGIN
    delete (LocalGroup *)group;
    TP_API_END
}

int tp_comm_init_local(tp_ctx *c, void *group) {
    TP_API_BEGIN
    TP_REQUIRE(c && group, "null argument");
    LocalGroup *G = (LocalGroup *)group;
    TP_REQUIRE(!c->graded, "tp_comm_init_local: this context has spacing (tp_set_spacing): graded grids exist on one slab without a slab group");
    TP_REQUIRE(c->wells.nw == 0, "tp_comm_init_local: this context has wells (tp_set_wells): completed wells exist on one slab without a slab group");
    TP_REQUIRE(c->grid.nranks == G->n, "group size differs from the context's nranks");
    int lo, hi;
    slab_of(c, c->grid.rank, lo, hi);
    TP_REQUIRE(lo == c->grid.off2 && hi - lo == c->grid.n2, "slab of this rank does not follow the library's partition rule");
    c->lgroup = G;
    c->dist = true;
    TP_API_END
}

int tp_set_field(tp_ctx *c, const char *name, const double *host, int64_t n) {
    TP_API_BEGIN
    TP_REQUIRE(c && name && host, "null argument");
    TP_REQUIRE(n == c->g.ntot, "field must have n0*n1*(n2+2) entries (slab with halo planes)");
    DBuf<double> *dst = nullptr;
    const std::string s(name);
    if (s == "phi") dst = &c->phi;
    else if (s == "kT") dst = &c->kTs;
    else if (s == "K0") dst = &c->K[0];
    else if (s == "K1") dst = &c->K[1];
    else if (s == "K2") dst = &c->K[2];
    TP_REQUIRE(dst, "unknown field name (phi, kT, K0, K1, K2)");
    copy_sync(c, dst->p, host, sizeof(double) * n, hipMemcpyHostToDevice);
    c->fields_ready = false;
    TP_API_END
}

int tp_finalize_fields(tp_ctx *c) {
    TP_API_BEGIN
    compute_trans(c);
    bc_trans(c);                 // (the half-cell transmissibilities of the Dirichlet sides follow K; nothing when no side is set)
    TP_HIP(hipStreamSynchronize(c->stream));
    c->fields_ready = true;
    drop_hierarchies(c);
    c->pc_ready = false;
    c->graph_epoch++;
    TP_API_END
}

int tp_set_sources(tp_ctx *c, int32_t n, const tp_source *entries) {
    TP_API_BEGIN
    TP_REQUIRE(c && (n == 0 || entries), "null argument");
    std::vector<tp_source> v(entries, entries + n);
    const GridDev &g = c->g;
    for (auto &e : v) {
        TP_REQUIRE(e.cell >= g.np && e.cell < g.np + g.nown, "source cell is not an owned cell of this slab");
        TP_REQUIRE(e.kind >= 0 && e.kind <= 2, "source kind must be 0 (prod), 1 (inj) or 2 (heater)");
    }
    std::stable_sort(v.begin(), v.end(), [](const tp_source &a, const tp_source &b) { return a.cell < b.cell; });
    std::vector<int> start;
    for (int i = 0; i < n; ++i)
        if (i == 0 || v[i].cell != v[i - 1].cell) start.push_back(i);
    c->nsrc = n;
    c->nsrc_groups = (int)start.size();
    start.push_back(n);
    c->src.alloc(std::max(1, n));
    c->src_start.alloc(start.size());
    c->rates.alloc((size_t)3 * std::max(1, n));
    if (n) copy_sync(c, c->src.p, v.data(), sizeof(tp_source) * n, hipMemcpyHostToDevice);
    copy_sync(c, c->src_start.p, start.data(), sizeof(int) * start.size(), hipMemcpyHostToDevice);
    TP_API_END
}

int tp_set_wells(tp_ctx *c, int32_t nwells, const tp_well *wells, int32_t nperfs, const tp_perf *perfs) {
    TP_API_BEGIN
    wells_set(c, nwells, wells, nperfs, perfs);
    TP_API_END
}

int tp_set_well_control(tp_ctx *c, int32_t well, double rate, double bhp_limit, int32_t shut) {
    TP_API_BEGIN
    wells_control(c, well, rate, bhp_limit, shut);
    TP_API_END
}

int tp_well_info(tp_ctx *c, tp_well_state *out) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    wells_info(c, out);
    TP_API_END
}

int tp_well_perf_rates(tp_ctx *c, double *rate, double *water_rate, double *oil_rate) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    wells_perf_rates(c, rate, water_rate, oil_rate);
    TP_API_END
}

int tp_well_factors(tp_ctx *c, double *cfac, double *bfac) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    wells_factors(c, cfac, bfac);
    TP_API_END
}

int tp_set_boundary(tp_ctx *c, int32_t side, int32_t kind, const double *values, int64_t nfaces) {
    TP_API_BEGIN
    bc_set(c, side, kind, values, (long)nfaces);
    TP_API_END
}

int tp_boundary_flux(tp_ctx *c, double *out) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "null argument");
    bc_flux(c, out);
    TP_API_END
}

int tp_set_spacing(tp_ctx *c, const double *h0, int64_t n0, const double *h1, int64_t n1, const double *h2, int64_t n2) {
    TP_API_BEGIN
    spacing_set(c, h0, (long)n0, h1, (long)n1, h2, (long)n2);
    TP_API_END
}

int tp_spacing_info(tp_ctx *c, int32_t *graded, double *hmin, double *hmax) {
    TP_API_BEGIN
    TP_REQUIRE(c && graded && hmin && hmax, "null argument");
    *graded = c->graded ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        hmin[a] = hmax[a] = c->grid.h[a];
        if (!c->graded) continue;
        hmin[a] = *std::min_element(c->hs_host[a].begin(), c->hs_host[a].end());
        hmax[a] = *std::max_element(c->hs_host[a].begin(), c->hs_host[a].end());
    }
    TP_API_END
}

int tp_set_saturation_functions(tp_ctx *c, const tp_satfn *sat) {
    TP_API_BEGIN
    satfn_set(c, sat);
    TP_API_END
}

int tp_saturation_info(tp_ctx *c, tp_satfn *out, int32_t *active) {
    TP_API_BEGIN
    TP_REQUIRE(c && out && active, "null argument");
    *out = c->satfn ? c->sat_host : satfn_defaults();
    *active = c->satfn ? 1 : 0;
    TP_API_END
}

int tp_set_state(tp_ctx *c, const double *u_host) {
    TP_API_BEGIN
    TP_REQUIRE(c && u_host, "null argument");
    copy_sync(c, c->u.p, u_host, sizeof(double) * c->u.n, hipMemcpyHostToDevice);
    TP_API_END
}

int tp_get_state(tp_ctx *c, double *u_host) {
    TP_API_BEGIN
    TP_REQUIRE(c && u_host, "null argument");
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, u_host, c->u.p, sizeof(double) * c->u.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_set_old_state(tp_ctx *c, const double *u_host) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    TP_REQUIRE(c->fields_ready, "fields not finalised");
    if (u_host) copy_sync(c, c->u_old.p, u_host, sizeof(double) * c->u.n, hipMemcpyHostToDevice);
    else vec_copy(c, c->u.p, c->u_old.p, (long)c->u.n);
    accum_old(c);
    c->have_old = true;
    TP_API_END
}

int tp_set_dt(tp_ctx *c, double dt) {
    TP_API_BEGIN
    TP_REQUIRE(c && dt > 0.0, "dt must be positive");
    c->dt = dt;
    TP_API_END
}

int tp_get_old_state(tp_ctx *c, double *u_host) {
    TP_API_BEGIN
    TP_REQUIRE(c && u_host, "null argument");
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, u_host, c->u_old.p, sizeof(double) * c->u_old.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_restore_state(tp_ctx *c) {
    TP_API_BEGIN
    TP_REQUIRE(c && c->have_old, "no old state to restore");
    vec_copy(c, c->u_old.p, c->u.p, (long)c->u.n);
    TP_API_END
}

int tp_saturation_range(tp_ctx *c, double *smin, double *smax) {
    TP_API_BEGIN
    TP_REQUIRE(c && smin && smax, "null argument");
    TP_REQUIRE(c->nph == 2, "saturation exists only in the two-phase model");
    field_minmax(c, c->u.p + 2 * c->g.ntot, smin, smax);
    TP_API_END
}

int tp_clamp_saturation(tp_ctx *c) {
    TP_API_BEGIN
    TP_REQUIRE(c && c->nph == 2, "saturation exists only in the two-phase model");
    field_clamp01(c, c->u.p + 2 * c->g.ntot);
    TP_API_END
}

int tp_residual(tp_ctx *c, double *norm2_out) {
    TP_API_BEGIN
    if (c->dist) halo_exchange(c, c->g, c->u.p, c->b, c->g.ntot);
    assemble(c, false, false);
    const double n = norm2(c, c->b, c->R.p);
    if (norm2_out) *norm2_out = n;
    TP_API_END
}

int tp_jacobian(tp_ctx *c) {
    TP_API_BEGIN
    if (c->dist) halo_exchange(c, c->g, c->u.p, c->b, c->g.ntot);
    assemble(c, true, schur_of(c->opt));
    c->pc_ready = false;
    TP_HIP(hipStreamSynchronize(c->stream));
    TP_API_END
}

int tp_get_residual(tp_ctx *c, double *host) {
    TP_API_BEGIN
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, host, c->R.p, sizeof(double) * c->R.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_export_jacobian(tp_ctx *c, double *host) {
    TP_API_BEGIN
    TP_REQUIRE(c->jac_ready, "Jacobian not assembled");
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, host, c->J.p, sizeof(double) * c->J.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_export_schur(tp_ctx *c, double *host) {
    TP_API_BEGIN
    TP_REQUIRE(c->Sm.n > 0 && c->jac_ready, "S~ not assembled (pc_cptr only)");
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, host, c->Sm.p, sizeof(double) * c->Sm.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_well_rates(tp_ctx *c, double *rate, double *water_rate, double *oil_rate) {
    TP_API_BEGIN
    if (c->nsrc == 0) return 0;
    well_rates(c);
    TP_HIP(hipStreamSynchronize(c->stream));
    const size_t n = c->nsrc;
    if (rate) copy_sync(c, rate, c->rates.p, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (water_rate) copy_sync(c, water_rate, c->rates.p + n, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (oil_rate) copy_sync(c, oil_rate, c->rates.p + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_vec_create(tp_ctx *c, int32_t *id) {
    TP_API_BEGIN
    auto *v = new DBuf<double>();
    v->alloc((size_t)c->b * c->g.ntot);
    c->vecs.push_back(v);
    *id = (int32_t)c->vecs.size() - 1;
    TP_API_END
}

int tp_set_ksp_monitor(tp_ctx *c, tp_ksp_monitor_fn cb, void *user) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    c->monitor = cb;
    c->monitor_user = user;
    TP_API_END
}

int tp_vec_create_batch(tp_ctx *c, int32_t n, int32_t *first_id) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && first_id, "bad arguments");
    const size_t nv = (size_t)c->b * c->g.ntot;
    auto *owner = new DBuf<double>();
    owner->alloc(nv * (size_t)n);                   // vector 0 of the batch owns the allocation
    DBuf<double> *first = new DBuf<double>();
    first->p = owner->p; first->n = nv; first->owned = true;
    owner->p = nullptr; owner->n = 0;
    delete owner;
    c->vecs.push_back(first);
    *first_id = (int32_t)c->vecs.size() - 1;
    for (int i = 1; i < n; ++i) {
        auto *v = new DBuf<double>();
        v->view(first->p + (size_t)i * nv, nv);
        c->vecs.push_back(v);
    }
    TP_API_END
}

// ids first..first+n-1 must be consecutive vectors of one batch (one allocation, stride b*ntot)
static const double *batch_base(tp_ctx *c, int32_t first, int32_t n) {
    const size_t nv = (size_t)c->b * c->g.ntot;
    const double *base = vec_of(c, first).p;
    for (int i = 1; i < n; ++i)
        TP_REQUIRE(vec_of(c, first + i).p == base + (size_t)i * nv, "vectors are not consecutive members of one batch "
                   "(tp_vec_create_batch)");
    return base;
}

int tp_vec_dot_batch(tp_ctx *c, int32_t first, int32_t n, int32_t w, double *out) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && out, "bad arguments");
    const double *V = batch_base(c, first, n);
    multi_dot(c, c->b, V, (long)c->b * c->g.ntot, n, vec_of(c, w).p, nullptr, out);
    TP_API_END
}

int tp_vec_axpy_batch(tp_ctx *c, int32_t first, int32_t n, const double *coef, int32_t w) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && coef, "bad arguments");
    const double *V = batch_base(c, first, n);
    TP_REQUIRE(w < first || w >= first + n, "w must not be a member of the batch");
    multi_axpy(c, c->b, V, (long)c->b * c->g.ntot, n, coef, 1.0, vec_of(c, w).p);
    TP_API_END
}

int tp_vec_orth_step(tp_ctx *c, int32_t first, int32_t k, int32_t w, int32_t mode, double eta, double *h, double *norm2,
                     int32_t *refined) {
    TP_API_BEGIN
    TP_REQUIRE(c && k >= 1 && h && norm2 && refined, "bad arguments");
    TP_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (never), 1 (if needed) or 2 (always)");
    TP_REQUIRE(mode != 1 || (eta > 0.0 && eta < 1.0), "eta must lie in (0, 1)");
    const double *V = batch_base(c, first, k);
    TP_REQUIRE(w < first || w >= first + k, "w must not be one of the k basis vectors");
    std::vector<double> out((size_t)k + 1);
    int ran = 0;
    orthogonalize_mode(c, c->b, V, (long)c->b * c->g.ntot, k, vec_of(c, w).p, mode, eta, out.data(), &ran);
    std::memcpy(h, out.data(), sizeof(double) * k);
    *norm2 = out[k];
    *refined = ran;
    TP_API_END
}

static FBatch &fbatch_of(tp_ctx *c, int32_t id, int32_t n) {
    TP_REQUIRE(id >= 0 && id < (int)c->fbatches.size(), "bad float batch id");
    TP_REQUIRE(n >= 0 && n <= c->fbatches[id]->n, "float batch has fewer vectors");
    return *c->fbatches[id];
}

int tp_fvec_create_batch(tp_ctx *c, int32_t n, int32_t *batch) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && batch, "bad arguments");
    auto *f = new FBatch();
    c->fbatches.push_back(f);
    f->buf.alloc((size_t)n * basis_stride(c));
    f->n = n;
    *batch = (int32_t)c->fbatches.size() - 1;
    TP_API_END
}

int tp_fvec_store(tp_ctx *c, int32_t batch, int32_t i, int32_t x) {
    TP_API_BEGIN
    TP_REQUIRE(c && i >= 0, "bad arguments");
    FBatch &f = fbatch_of(c, batch, i + 1);
    basis_round_store(c, c->b, vec_of(c, x).p, f.buf.p + (size_t)i * basis_stride(c));
    TP_HIP(hipGetLastError());
    TP_API_END
}

int tp_fvec_get(tp_ctx *c, int32_t batch, int32_t i, float *host) {
    TP_API_BEGIN
    TP_REQUIRE(c && i >= 0 && host, "bad arguments");
    FBatch &f = fbatch_of(c, batch, i + 1);
    copy_sync(c, host, f.buf.p + (size_t)i * basis_stride(c), sizeof(float) * (size_t)c->b * c->g.nown, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_fvec_dot_batch(tp_ctx *c, int32_t batch, int32_t n, int32_t w, double *out) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && out, "bad arguments");
    FBatch &f = fbatch_of(c, batch, n);
    multi_dot_s(c, c->b, f.buf.p, basis_stride(c), n, vec_of(c, w).p, out);
    TP_API_END
}

int tp_fvec_axpy_batch(tp_ctx *c, int32_t batch, int32_t n, const double *coef, int32_t w) {
    TP_API_BEGIN
    TP_REQUIRE(c && n >= 1 && coef, "bad arguments");
    FBatch &f = fbatch_of(c, batch, n);
    multi_axpy_s(c, c->b, f.buf.p, basis_stride(c), n, coef, 1.0, vec_of(c, w).p);
    TP_API_END
}

int tp_vec_norm2(tp_ctx *c, int32_t x, double *out) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "bad arguments");
    *out = norm2(c, c->b, vec_of(c, x).p);
    TP_API_END
}

int tp_vec_set(tp_ctx *c, int32_t id, const double *host) {
    TP_API_BEGIN
    DBuf<double> &v = vec_of(c, id);
    copy_sync(c, v.p, host, sizeof(double) * v.n, hipMemcpyHostToDevice);
    TP_API_END
}

int tp_vec_get(tp_ctx *c, int32_t id, double *host) {
    TP_API_BEGIN
    DBuf<double> &v = vec_of(c, id);
    TP_HIP(hipStreamSynchronize(c->stream));
    copy_sync(c, host, v.p, sizeof(double) * v.n, hipMemcpyDeviceToHost);
    TP_API_END
}

int tp_vec_copy_residual(tp_ctx *c, int32_t id) {
    TP_API_BEGIN
    vec_copy(c, c->R.p, vec_of(c, id).p, (long)c->R.n);
    TP_API_END
}

int tp_spmv(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    TP_REQUIRE(c->jac_ready, "Jacobian not assembled");
    TP_REQUIRE(x != y, "tp_spmv: x and y must differ");
    if (c->dist) halo_exchange(c, c->g, vec_of(c, x).p, c->b, c->g.ntot);
    krylov_apply(c, vec_of(c, x).p, vec_of(c, y).p, false);     // (J x plus the wells' rank-1 terms: the operator the Krylov methods see)
    TP_API_END
}

int tp_pc_setup(tp_ctx *c) {
    TP_API_BEGIN
    pc_setup(c);
    TP_API_END
}

int tp_pc_apply(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    TP_REQUIRE(x != y, "tp_pc_apply: x and y must differ");
    pc_apply(c, vec_of(c, x).p, vec_of(c, y).p);
    TP_API_END
}

int tp_stage1_update(tp_ctx *c) {
    TP_API_BEGIN
    // CPRStage1PC.update: assemble_blocks + create_decoup + pc_schur.setOperators (AMG set-up).
    // Here PCSetUp of both stages is one call; kept separate in the API for the PCBase mirror.
    pc_setup(c);
    TP_API_END
}

int tp_stage1_apply(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    TP_REQUIRE(c->pc_ready, "stage 1 not set up");
    TP_REQUIRE(x != y, "x and y must differ");
    schur_count(c, 1);
    stage1_apply(c, vec_of(c, x).p, vec_of(c, y).p);
    TP_API_END
}

int tp_ilu0_factor(tp_ctx *c) {
    TP_API_BEGIN
    ilu_factor(c);
    TP_API_END
}

int tp_ilu0_solve(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    TP_REQUIRE(x != y, "x and y must differ");
    ilu_solve(c, vec_of(c, x).p, vec_of(c, y).p, nullptr);
    TP_API_END
}

int tp_stage_rhs(tp_ctx *c, int32_t x, int32_t y, int32_t out) {
    TP_API_BEGIN
    TP_REQUIRE(c && c->pc_ready, "tp_stage_rhs: preconditioner not set up (the decoupling coefficients are those of tp_pc_setup)");
    TP_REQUIRE(c->opt.pc_kind == 0 || c->opt.pc_kind == 1 || c->opt.pc_kind == 3, "tp_stage_rhs: pc_kind 0, 1 or 3 (a first stage with a second one behind it)");
    TP_REQUIRE(x != y && x != out && y != out, "tp_stage_rhs: x, y and out must differ");
    if (c->dist) halo_exchange(c, c->g, vec_of(c, y).p, c->b, c->g.ntot);
    stage_rhs(c, vec_of(c, x).p, vec_of(c, y).p, vec_of(c, out).p);
    TP_API_END
}

// the composite's temperature stage (tp_options.pc_ctr)
static void require_ctr(tp_ctx *c, const char *who) {
    TP_REQUIRE(c, "null argument");
    if (!c->opt.pc_ctr) throw Error(std::string(who) + ": pc_ctr is off (the temperature stage and its hierarchy exist with tp_options.pc_ctr = 1)");
    if (!c->pc_ready || !c->amg_ctr) throw Error(std::string(who) + ": preconditioner not set up (the A_TT hierarchy of pc_ctr is that of tp_pc_setup)");
}

int tp_ctr_rhs(tp_ctx *c, int32_t x, int32_t y, int32_t out) {
    TP_API_BEGIN
    require_ctr(c, "tp_ctr_rhs");
    TP_REQUIRE(x != y && x != out && y != out, "tp_ctr_rhs: x, y and out must differ");
    row_rhs(c, vec_of(c, x).p, vec_of(c, y).p, vec_of(c, out).p + c->g.ntot);
    TP_API_END
}

int tp_ctr_apply(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    require_ctr(c, "tp_ctr_apply");
    TP_REQUIRE(x != y, "tp_ctr_apply: x and y must differ");
    ctr_apply(c, vec_of(c, x).p, vec_of(c, y).p);
    TP_API_END
}

int tp_ctr_info(tp_ctx *c, int32_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "bad arguments");
    TP_REQUIRE(c->opt.pc_ctr, "tp_ctr_info: pc_ctr is off (the temperature stage exists with tp_options.pc_ctr = 1)");
    TP_REQUIRE(c->pc_ready && c->amg_ctr, "tp_ctr_info: preconditioner not set up");
    out[0] = c->opt.pc_ctr;
    out[1] = (int32_t)c->amg_ctr->plan.lv.size();
    out[2] = (int32_t)c->ctr_setups;
    out[3] = (int32_t)c->ctr_applies;
    TP_API_END
}

int tp_schur_info(tp_ctx *c, int *fact, double *scale, long *k0_applies, long *ks_applies) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    if (fact) *fact = c->opt.schur_fact;
    if (scale) *scale = c->opt.schur_fact == 3 ? c->opt.schur_scale : -1.0;
    if (k0_applies) *k0_applies = c->schur_k0;
    if (ks_applies) *ks_applies = c->schur_ks;
    TP_API_END
}

int tp_amg_setup(tp_ctx *c, int32_t which) {
    TP_API_BEGIN
    (void)which;
    pc_setup(c);
    TP_API_END
}

int tp_amg_vcycle(tp_ctx *c, int32_t which, int32_t field_b, int32_t b, int32_t field_x, int32_t x) {
    TP_API_BEGIN
    TP_REQUIRE(c->pc_ready, "AMG not set up");
    if (which == 2) {       // pc_cptramg: the system V-cycle on fields (0,1) of b -> fields (0,1) of x
        TP_REQUIRE(c->bamg && !c->dist, "system AMG not set up (pc_cptramg, single slab)");
        TP_REQUIRE(b != x && field_b == 0 && field_x == 0, "system V-cycle: fields (0,1) of two different vectors");
        bamg_vcycle(c, c->bamg, vec_of(c, b).p, vec_of(c, x).p);
        return 0;
    }
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg, "this AMG hierarchy does not exist for the selected preconditioner");
    resolve_cycle_shapes(c);
    TP_REQUIRE(!c->dist || amg->plan.dist_levels > 0, "tp_amg_vcycle works on slab vectors: not available when the hierarchy is replicated on the gathered global grid");
    TP_REQUIRE(field_b >= 0 && field_b < c->b && field_x >= 0 && field_x < c->b, "bad field index");
    TP_REQUIRE(!(b == x && field_b == field_x), "b and x must differ");
    amg_vcycle(c, amg, vec_of(c, b).p + (long)field_b * c->g.ntot, vec_of(c, x).p + (long)field_x * c->g.ntot);
    TP_API_END
}

int tp_schur_apply(tp_ctx *c, int32_t x, int32_t y) {
    TP_API_BEGIN
    TP_REQUIRE(c->pc_ready && c->amg_T, "S~ AMG not set up (pc_cptr only)");
    resolve_cycle_shapes(c);
    TP_REQUIRE(!c->dist || c->amg_T->plan.dist_levels > 0, "tp_schur_apply works on slab vectors: not available when the hierarchy is replicated on the gathered global grid");
    TP_REQUIRE(x != y, "x and y must differ");
    amg_vcycle(c, c->amg_T, vec_of(c, x).p + c->g.ntot, vec_of(c, y).p + c->g.ntot);
    TP_API_END
}

int tp_fgmres(tp_ctx *c, int32_t b, int32_t x, int32_t *its, int32_t *reason, double *rnorm) {
    TP_API_BEGIN
    TP_REQUIRE(b != x, "b and x must differ");
    if (!c->pc_ready) pc_setup(c);
    int it = 0;
    double rn = 0.0;
    const int r = fgmres(c, vec_of(c, b).p, vec_of(c, x).p, &it, &rn, c->opt.ksp_rtol);
    if (its) *its = it;
    if (reason) *reason = r;
    if (rnorm) *rnorm = rn;
    TP_API_END
}

int tp_bcgs(tp_ctx *c, int32_t b, int32_t x, int32_t *its, int32_t *reason, double *rnorm) {
    TP_API_BEGIN
    TP_REQUIRE(b != x, "b and x must differ");
    if (!c->pc_ready) pc_setup(c);
    int it = 0;
    double rn = 0.0;
    const int r = bcgs(c, vec_of(c, b).p, vec_of(c, x).p, &it, &rn, c->opt.ksp_rtol);
    if (its) *its = it;
    if (reason) *reason = r;
    if (rnorm) *rnorm = rn;
    TP_API_END
}

int tp_ksp_info(tp_ctx *c, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "null argument");
    ksp_info(c, out);
    TP_API_END
}

int tp_ksp_basis_info(tp_ctx *c, int64_t out[6]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "null argument");
    out[0] = c->opt.ksp_basis_single ? 1 : 0;
    out[1] = c->gs_cap_s;
    out[2] = basis_stride(c);
    out[3] = (int64_t)(c->kstage.n / ((size_t)c->b * c->g.ntot));
    out[4] = c->ksp_cycles;
    out[5] = c->ksp_true_res;
    TP_API_END
}

int tp_ksp_reorth_info(tp_ctx *c, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "null argument");
    long long h[4] = {0, 0, 0, 0};
    if (c->ro_stat.n >= 4) copy_sync(c, h, c->ro_stat.p, sizeof(h), hipMemcpyDeviceToHost);
    out[0] = c->opt.ksp_reorth;
    out[1] = c->ro_steps;
    out[2] = h[1];
    out[3] = h[2];
    TP_API_END
}

int tp_inner_stats(tp_ctx *c, int64_t *applies, int64_t *its, int64_t *unconverged) {
    TP_API_BEGIN
    TP_REQUIRE(c, "null argument");
    long long h[3] = {0, 0, 0};
    if (c->inner.stats.n >= 3) copy_sync(c, h, c->inner.stats.p, sizeof(h), hipMemcpyDeviceToHost);
    if (applies) *applies = h[0];
    if (its) *its = h[1];
    if (unconverged) *unconverged = h[2];
    TP_API_END
}

int tp_newton_solve(tp_ctx *c, tp_solve_info *info) {
    TP_API_BEGIN
    TP_REQUIRE(c && info, "null argument");
    newton(c, info);
    TP_HIP(hipStreamSynchronize(c->stream));
    TP_API_END
}

int tp_ls_info(tp_ctx *c, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "bad arguments");
    out[0] = c->opt.ls_kind;
    out[1] = (int64_t)(c->ls_u0.n * sizeof(double));
    out[2] = c->ls_evals;
    out[3] = c->ls_nonfinite;
    TP_API_END
}

int tp_ls_history(tp_ctx *c, int32_t cap, double *lambda, double *fnorm, int32_t *trials, int32_t *n) {
    TP_API_BEGIN
    TP_REQUIRE(c && n && cap >= 0 && (cap == 0 || (lambda && fnorm && trials)), "bad arguments");
    *n = (int32_t)c->ls_lambda.size();
    for (int i = 0; i < std::min<int>(cap, *n); ++i) { lambda[i] = c->ls_lambda[i]; fnorm[i] = c->ls_fnorm[i]; trials[i] = c->ls_trials[i]; }
    TP_API_END
}

int tp_ew_next_rtol(const tp_options *opt, int32_t k, double fnorm, double fnorm_last, double lresid_last, double rtol_last,
                    double *rtol) {
    TP_API_BEGIN
    TP_REQUIRE(opt && rtol && k >= 0, "bad arguments");
    TP_REQUIRE(opt->ksp_ew != 0, "tp_ew_next_rtol needs ksp_ew 1 or 2");
    ew_check_options(*opt);
    *rtol = ew_next_rtol(*opt, k, fnorm, fnorm_last, lresid_last, rtol_last);
    TP_API_END
}

int tp_ew_info(tp_ctx *c, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "bad arguments");
    out[0] = c->opt.ksp_ew;
    out[1] = c->ew_solves;
    out[2] = c->ew_lsolves;
    out[3] = c->ew_safeguard;
    TP_API_END
}

int tp_ew_history(tp_ctx *c, int32_t cap, double *rtol, double *fnorm, double *lresid, int32_t *kits, int32_t *kreason,
                  int32_t *n) {
    TP_API_BEGIN
    TP_REQUIRE(c && n && cap >= 0 && (cap == 0 || (rtol && fnorm && lresid && kits && kreason)), "bad arguments");
    *n = (int32_t)c->ew_rtol.size();
    for (int i = 0; i < std::min<int>(cap, *n); ++i) {
        rtol[i] = c->ew_rtol[i]; fnorm[i] = c->ew_fnorm[i]; lresid[i] = c->ew_lresid[i];
        kits[i] = c->ew_kits[i]; kreason[i] = c->ew_kreason[i];
    }
    TP_API_END
}

int tp_ls_step_stats(tp_ctx *c, int32_t dx, double out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "bad arguments");
    ls_step_stats(c, vec_of(c, dx).p, out);
    TP_API_END
}

int tp_ls_trial(tp_ctx *c, int32_t u0, int32_t dx, double lambda, int32_t out) {
    TP_API_BEGIN
    TP_REQUIRE(c, "bad arguments");
    ls_trial(c, vec_of(c, u0).p, vec_of(c, dx).p, lambda, vec_of(c, out).p);
    TP_HIP(hipStreamSynchronize(c->stream));
    TP_API_END
}

int tp_time_kernel(tp_ctx *c, int32_t which, int32_t reps, double *ms_avg) {
    TP_API_BEGIN
    TP_REQUIRE(reps > 0 && ms_avg, "bad arguments");
    ensure_work(c);          // (w3 needs three planes even when b == 2: tp_solver.hip)
    if (which != 3) TP_REQUIRE(c->jac_ready, "Jacobian not assembled");
    if (which == 1 || which == 2 || which == 4 || which == 9 || which == 10) TP_REQUIRE(c->pc_ready, "preconditioner not set up");
    if (which == 12) require_ctr(c, "tp_time_kernel 12");
    if (which == 9 || which == 10) TP_REQUIRE(c->opt.pc_kind == 0 || c->opt.pc_kind == 1 || c->opt.pc_kind == 3, "pc_kind 0, 1 or 3");
    auto run = [&]() {
        switch (which) {
            case 0: spmv_block(c, c->J.p, c->R.p, c->w2.p); break;
            case 1: ilu_solve(c, c->R.p, c->w2.p, nullptr); break;
            case 2:
                resolve_cycle_shapes(c);
                if (sysamg_of(c->opt)) { TP_REQUIRE(!c->dist, "single slab only"); bamg_vcycle(c, c->bamg, c->R.p, c->w2.p); break; }
                if (c->dist && c->amg_p->plan.dist_levels == 0) amg_vcycle(c, c->amg_p, c->gvec.p, c->gvec.p + 2 * c->gfull.ntot);   // global-grid buffers
                else amg_vcycle(c, c->amg_p, c->R.p, c->w2.p);
                break;
            case 3: assemble(c, true, schur_of(c->opt)); break;
            case 4: pc_apply(c, c->R.p, c->dx.p); break;
            case 5: pc_setup(c); break;
            case 6: ilu_factor(c); break;
            case 7: {       // one classical Gram-Schmidt step against 16 basis vectors (VecMDot + VecMAXPY + norm)
                TP_REQUIRE(c->gs_cap >= 17, "Krylov basis smaller than 17 vectors: run a solve first");
                std::vector<double> hh(18);
                orthogonalize(c, c->b, c->V.p, (long)c->b * c->g.ntot, 16, c->w2.p, hh.data());
                break;
            }
            case 8: {       // the same step against 16 vectors of the fp32 basis
                TP_REQUIRE(c->gs_cap_s >= 17, "fp32 Krylov basis smaller than 17 vectors: run a ksp_basis_single solve first");
                std::vector<double> hh(18);
                orthogonalize_s(c, c->b, c->Vs.p, basis_stride(c), 16, c->w2.p, hh.data());
                break;
            }
            case 9: stage_rhs(c, c->R.p, c->dx.p, c->w3.p); break;      // (dx: whatever the last application left; the time does not depend on it)
            case 10:
                resid_block_cols(c, c->J.p, c->R.p, c->dx.p, c->b, c->w1.p);
                for (int q = 0; q < npri_of(c->opt); ++q) stage1_rhs(c, c->w1.p, q, c->w3.p + (long)q * c->g.ntot);
                break;
            case 11: resid_block_cols(c, c->J.p, c->R.p, c->dx.p, c->b, c->w1.p); break;
            case 12: row_rhs(c, c->R.p, c->dx.p, c->w3.p); break;       // (dx as in 9)
            case 13:        // k_assemble_bc alone: it ADDS to R, J and S~, which are no assembly afterwards (re-assemble)
                TP_REQUIRE(c->bc.ncells > 0, "no boundary set (tp_set_boundary)");
                assemble_bc(c, true, schur_of(c->opt));
                break;
            case 14:        // k_well_apply alone: it ADDS the rank-1 terms of R to w2
                TP_REQUIRE(c->wells.nw > 0, "no well set (tp_set_wells)");
                wells_apply_only(c, c->R.p, c->w2.p);
                break;
            case 15:        // k_wells alone: it ADDS to R, J and S~, which are no assembly afterwards (re-assemble)
                TP_REQUIRE(c->wells.nw > 0, "no well set (tp_set_wells)");
                wells_assemble(c, true, schur_of(c->opt));
                break;
            case 16:        // k_sources alone (the rates-only form, which writes nothing but the rates)
                TP_REQUIRE(c->nsrc_groups > 0, "no source set (tp_set_sources)");
                well_rates(c);
                break;
            default: throw Error("unknown kernel id");
        }
    };
    run();                                                      // warm-up
    TP_HIP(hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) run();
    TP_HIP(hipEventRecord(c->ev1, c->stream));
    TP_HIP(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    TP_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *ms_avg = (double)ms / reps;
    TP_API_END
}

// layout of hierarchy `which`: 0 pressure, 1 temperature / Schur, 2 the (p,T) system hierarchy of pc_cptramg
static const AmgPlan &plan_of(tp_ctx *c, int which) {
    if (which == 2) {
        TP_REQUIRE(c->bamg, "system AMG hierarchy not built");
        return c->bamg->plan;
    }
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg, "AMG hierarchy not built");
    return amg->plan;
}

int tp_amg_info(tp_ctx *c, int32_t which, int32_t *nlevels, double *op_complexity) {
    TP_API_BEGIN
    const AmgPlan &P = plan_of(c, which);
    if (nlevels) *nlevels = (int)P.lv.size();
    double s = 0.0, s0 = 0.0;       // global cells per level (a distributed level holds this rank's slab only)
    for (size_t l = 0; l < P.lv.size(); ++l) {
        const GridDev &g = P.lv[l].g;
        const double cells = (double)g.np * g.gn2;
        s += cells;
        if (l == 0) s0 = cells;
    }
    if (op_complexity) *op_complexity = which == 2 ? 0.0 : s / s0;
    TP_API_END
}

int tp_amg_trunc(tp_ctx *c, int32_t which, int32_t *level, double *ratio0) {
    TP_API_BEGIN
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg, "AMG hierarchy not built");
    resolve_cycle_shapes(c);
    if (level) *level = amg->trunc;
    if (ratio0) *ratio0 = amg->ratio0;
    TP_API_END
}

int tp_amg_layout(tp_ctx *c, int32_t which, int32_t *dist_levels, int32_t *axes, int32_t cap, int32_t *naxes) {
    TP_API_BEGIN
    const AmgPlan &P = plan_of(c, which);
    if (dist_levels) *dist_levels = P.dist_levels;
    if (naxes) *naxes = (int)P.sched.size();
    for (int i = 0; axes && i < cap && i < (int)P.sched.size(); ++i) axes[i] = P.sched[i];
    TP_API_END
}

int tp_amg_tail_info(tp_ctx *c, int32_t which, int64_t out[6]) {
    TP_API_BEGIN
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg && out, "AMG hierarchy not built");
    resolve_cycle_shapes(c);
    out[0] = amg->tdense_on ? 1 : 0;
    out[1] = amg->plan.tail_level;
    out[2] = amg->lv[amg->plan.tail_level]->g.nown;
    out[3] = amg->tdense_builds;
    out[4] = amg->tdense_applies;
    out[5] = amg->tail_launches;
    TP_API_END
}

int tp_amg_line_info(tp_ctx *c, int32_t which, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out && (which == 0 || which == 1), "bad arguments");
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg, "AMG hierarchy not built");
    amg_line_info(amg, out);
    TP_API_END
}

int tp_amg_gs_info(tp_ctx *c, int32_t which, int64_t out[4]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out && (which == 0 || which == 1), "bad arguments");
    Amg *amg = which == 0 ? c->amg_p : c->amg_T;
    TP_REQUIRE(amg, "AMG hierarchy not built");
    amg_gs_info(amg, out);
    TP_API_END
}

int tp_ilu_factor_bytes(tp_ctx *c, int64_t *bytes) {
    TP_API_BEGIN
    TP_REQUIRE(c && bytes, "null argument");
    *bytes = ilu_factor_bytes(c);
    TP_API_END
}

int tp_ilu_layout(tp_ctx *c, int32_t out[8]) {
    TP_API_BEGIN
    TP_REQUIRE(c && out, "null argument");
    ilu_layout(c, out);
    TP_API_END
}

}  // extern "C"
