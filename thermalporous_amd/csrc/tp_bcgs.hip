// Right-preconditioned (flexible) BiCGStab as the outer Krylov method (tp_options.ksp_kind = 1; PETSc: ksp_type fbcgs, or
// bcgs with ksp_pc_side right).  A short recurrence: seven vectors plus the shared scratch w2 whatever the iteration count, no basis, no
// Gram-Schmidt.
//
//   r = b; r^ = b; rho = (b,b); tol = max(rtol ||b||, ksp_atol)      (rtol: ksp_rtol, or the solve's eta under ksp_ew)
//   repeat:  p = r + beta (p - omega v)            (first iteration: beta = 0, p = r)
//            p^ = M p;  v = J p^;  alpha = rho / (r^,v)
//            s = r - alpha v;  ||s|| <= tol: half-step exit, omega := 0
//            s^ = M s;  t = J s^;  omega = (t,s)/(t,t)
//            x += alpha p^ + omega s^;  r = s - omega t;  rho' = (r^,r);  beta = (rho'/rho)(alpha/omega)
//            stop on ||r|| <= tol
//
// Every scalar -- rho, alpha, omega, beta, tol, the latches and the sums they are formed from -- lives in BcgsWork::state on the
// device (the k_inner_hess pattern of tp_inner.hip): a streaming kernel writes per-wave partials, k_bcgs_reduce sums them in a
// fixed order, the sums are all-reduced over the slabs in-stream, and a one-wavefront kernel turns them into the coefficients
// the next streaming kernel reads.  The host waits ONCE per iteration, on an event behind the last of them, and reads ||r||^2
// and the latches from pinned memory.
//
// Latches.  A coefficient that cannot be formed -- a zero or non-finite denominator, or any latch already set -- is an exact
// 0.0, and a streaming kernel that finds a coefficient 0.0 does not READ the vector it would have scaled (p = r, s = r, r = s,
// x unchanged): never 0 x stale, never a division by zero.  What holds after a breakdown or a NaN: x keeps its last finite value
// (alpha and omega are forced to 0 before k_bcgs_update runs), and every work vector is rewritten before its next read (by the
// next solve: r^, r from b; p through beta = 0; v, t, p^, s^ as outputs).  The work vectors themselves need NOT stay finite to
// the end of the iteration in flight: with a non-finite (r^,v) alpha is 0 and s = r is finite, but when ||s||^2 or a (t,.) sum
// is the first non-finite quantity, s already holds it, M s and J M s run on it, and r = s is stored non-finite.
//
// Launches follow tp_linalg.hip / tp_inner.hip: TP_BLOCK threads, xcd_grid blocks remapped by xcd_tid, so each XCD streams one
// contiguous eighth of every vector -- the same eighth in every kernel of the iteration and in the SpMV between them.  The
// partials are indexed by the remapped wave, so the order of the sums does not depend on where a block ran.
//
// Streaming kernels: one pass over memory each, BC_CH items per lane, an item being one double or -- when the plane size is even
// and every pointer 16-byte aligned -- an aligned pair (one 16-byte load / store per lane).  Sums run over owned cells of all
// fields; two-stage, fixed order, no floating-point atomics: reproducible run to run.
#include "tp_common.hpp"
#include <cmath>
#include <algorithm>
#include <cstdlib>

namespace tp {

constexpr int BC_CH = 4;               // items per lane of the streaming kernels
// layout of BcgsWork::state (doubles)
constexpr int BS_SUM = 0;              // sums of the reduction in flight (at most two)
constexpr int BS_RHO = 2, BS_ALPHA = 3, BS_OMEGA = 4, BS_BETA = 5, BS_TOL = 6, BS_RR = 7;
constexpr int BS_DONE = 8;             // latch: ||r|| <= tol
constexpr int BS_BRK = 9;              // latch: (r^,v) == 0 in the iteration in flight
constexpr int BS_NAN = 10;             // latch: a sum was not finite
constexpr int BS_HALF = 11;            // latch: ||s|| <= tol (half-step exit)
constexpr int BS_NEXT = 12;            // rho == 0 (or omega == 0 without convergence): the NEXT iteration cannot start
constexpr int BS_SS = 13;              // ||s||^2 of the iteration in flight
constexpr int BS_SIZE = 16;
// what the host reads per iteration (doubles in tp_ctx::h_pin)
constexpr int BH_RR = 0, BH_DONE = 1, BH_BRK = 2, BH_NAN = 3, BH_HALF = 4, BH_NEXT = 5, BH_SS = 6, BH_N = 8;

template <int W>
struct alignas(8 * W) BcPack {
    double v[W];
};

__device__ __forceinline__ double bc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// item t (W consecutive owned entries of one field plane; nown is a multiple of W) -> index of its first entry.  nf <= 3.
template <int W>
__device__ __forceinline__ long bc_index(const GridDev &g, long t) {
    const long e = t * W;
    const long f = (long)(e >= g.nown) + (long)(e >= 2 * g.nown);
    return f * g.ntot + g.np + (e - f * g.nown);
}
template <int W>
__device__ __forceinline__ BcPack<W> bc_ld(const double *p, long i) { return *reinterpret_cast<const BcPack<W> *>(p + i); }
template <int W>
__device__ __forceinline__ void bc_st(double *p, long i, const BcPack<W> &v) { *reinterpret_cast<BcPack<W> *>(p + i) = v; }

// the items of this lane: idx[j] (tail lanes: item 0, a valid address that is loaded, never stored and never summed)
#define BC_ITEMS                                                                                 \
    const long wave = xcd_tid() >> 6;                                                            \
    const int lane = threadIdx.x & 63;                                                           \
    if (wave >= nwaves) return;                                                                  \
    const long nit = g.nown * nf / W;                                                            \
    long idx[BC_CH];                                                                             \
    bool ok[BC_CH];                                                                              \
    _Pragma("unroll") for (int j = 0; j < BC_CH; ++j) {                                          \
        const long t = (wave * BC_CH + j) * 64 + lane;                                           \
        ok[j] = t < nit;                                                                         \
        idx[j] = bc_index<W>(g, ok[j] ? t : 0);                                                  \
    }

// p = r + beta (p - omega v); beta == 0 (first iteration, or a latch): p = r, and p, v are not read
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_p(GridDev g, int nf, const double *__restrict__ st, const double *__restrict__ r,
                                                const double *__restrict__ v, double *__restrict__ p, long nwaves) {
    BC_ITEMS
    const double beta = st[BS_BETA], omega = st[BS_OMEGA];
    BcPack<W> rr[BC_CH], pp[BC_CH], vv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) rr[j] = bc_ld<W>(r, idx[j]);
    if (beta != 0.0) {
#pragma unroll
        for (int j = 0; j < BC_CH; ++j) { pp[j] = bc_ld<W>(p, idx[j]); vv[j] = bc_ld<W>(v, idx[j]); }
#pragma unroll
        for (int j = 0; j < BC_CH; ++j)
#pragma unroll
            for (int q = 0; q < W; ++q) rr[j].v[q] = rr[j].v[q] + beta * (pp[j].v[q] - omega * vv[j].v[q]);
    }
#pragma unroll
    for (int j = 0; j < BC_CH; ++j)
        if (ok[j]) bc_st<W>(p, idx[j], rr[j]);
}

// partial[wave] = <a, b>
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_dot(GridDev g, int nf, const double *__restrict__ a, const double *__restrict__ b,
                                                  double *__restrict__ partial, long nwaves) {
    BC_ITEMS
    BcPack<W> av[BC_CH], bv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) { av[j] = bc_ld<W>(a, idx[j]); bv[j] = bc_ld<W>(b, idx[j]); }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < BC_CH; ++j)
#pragma unroll
        for (int q = 0; q < W; ++q) s += ok[j] ? av[j].v[q] * bv[j].v[q] : 0.0;
    s = bc_wave_sum(s);
    if (lane == 0) partial[wave] = s;
}

// s = r - alpha v (alpha == 0: s = r, v is not read) and partial[wave] = <s, s>
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_s(GridDev g, int nf, const double *__restrict__ st, const double *__restrict__ r,
                                                const double *__restrict__ v, double *__restrict__ s, double *__restrict__ partial,
                                                long nwaves) {
    BC_ITEMS
    const double alpha = st[BS_ALPHA];
    BcPack<W> rr[BC_CH], vv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) rr[j] = bc_ld<W>(r, idx[j]);
    if (alpha != 0.0) {
#pragma unroll
        for (int j = 0; j < BC_CH; ++j) vv[j] = bc_ld<W>(v, idx[j]);
#pragma unroll
        for (int j = 0; j < BC_CH; ++j)
#pragma unroll
            for (int q = 0; q < W; ++q) rr[j].v[q] = rr[j].v[q] - alpha * vv[j].v[q];
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) {
        if (ok[j]) bc_st<W>(s, idx[j], rr[j]);
#pragma unroll
        for (int q = 0; q < W; ++q) acc += ok[j] ? rr[j].v[q] * rr[j].v[q] : 0.0;
    }
    acc = bc_wave_sum(acc);
    if (lane == 0) partial[wave] = acc;
}

// partial[wave] = <t, s>, partial[nwaves + wave] = <t, t>: one pass over t and s
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_dot2(GridDev g, int nf, const double *__restrict__ t, const double *__restrict__ s,
                                                   double *__restrict__ partial, long nwaves) {
    BC_ITEMS
    BcPack<W> tv[BC_CH], sv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) { tv[j] = bc_ld<W>(t, idx[j]); sv[j] = bc_ld<W>(s, idx[j]); }
    double ts = 0.0, tt = 0.0;
#pragma unroll
    for (int j = 0; j < BC_CH; ++j)
#pragma unroll
        for (int q = 0; q < W; ++q) {
            ts += ok[j] ? tv[j].v[q] * sv[j].v[q] : 0.0;
            tt += ok[j] ? tv[j].v[q] * tv[j].v[q] : 0.0;
        }
    ts = bc_wave_sum(ts);
    tt = bc_wave_sum(tt);
    if (lane == 0) { partial[wave] = ts; partial[nwaves + wave] = tt; }
}

// x += alpha p^ + omega s^ ; r = s - omega t ; partial[wave] = <r^, r>, partial[nwaves + wave] = <r, r>.  A coefficient that is
// 0.0 drops its term and the load of its vector (alpha == omega == 0: x is neither read nor written).
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_update(GridDev g, int nf, const double *__restrict__ st, const double *__restrict__ ph,
                                                     const double *__restrict__ sh, const double *__restrict__ s,
                                                     const double *__restrict__ t, const double *__restrict__ rh,
                                                     double *__restrict__ x, double *__restrict__ r, double *__restrict__ partial,
                                                     long nwaves) {
    BC_ITEMS
    const double alpha = st[BS_ALPHA], omega = st[BS_OMEGA];
    BcPack<W> sv[BC_CH], hv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) { sv[j] = bc_ld<W>(s, idx[j]); hv[j] = bc_ld<W>(rh, idx[j]); }
    if (alpha != 0.0 || omega != 0.0) {
        BcPack<W> xv[BC_CH], a[BC_CH];
#pragma unroll
        for (int j = 0; j < BC_CH; ++j) xv[j] = bc_ld<W>(x, idx[j]);
        if (alpha != 0.0) {
#pragma unroll
            for (int j = 0; j < BC_CH; ++j) a[j] = bc_ld<W>(ph, idx[j]);
#pragma unroll
            for (int j = 0; j < BC_CH; ++j)
#pragma unroll
                for (int q = 0; q < W; ++q) xv[j].v[q] = xv[j].v[q] + alpha * a[j].v[q];
        }
        if (omega != 0.0) {
#pragma unroll
            for (int j = 0; j < BC_CH; ++j) a[j] = bc_ld<W>(sh, idx[j]);
#pragma unroll
            for (int j = 0; j < BC_CH; ++j)
#pragma unroll
                for (int q = 0; q < W; ++q) xv[j].v[q] = xv[j].v[q] + omega * a[j].v[q];
#pragma unroll
            for (int j = 0; j < BC_CH; ++j) a[j] = bc_ld<W>(t, idx[j]);
#pragma unroll
            for (int j = 0; j < BC_CH; ++j)
#pragma unroll
                for (int q = 0; q < W; ++q) sv[j].v[q] = sv[j].v[q] - omega * a[j].v[q];
        }
#pragma unroll
        for (int j = 0; j < BC_CH; ++j)
            if (ok[j]) bc_st<W>(x, idx[j], xv[j]);
    }
    double rho = 0.0, rr = 0.0;
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) {
        if (ok[j]) bc_st<W>(r, idx[j], sv[j]);
#pragma unroll
        for (int q = 0; q < W; ++q) {
            rho += ok[j] ? hv[j].v[q] * sv[j].v[q] : 0.0;
            rr += ok[j] ? sv[j].v[q] * sv[j].v[q] : 0.0;
        }
    }
    rho = bc_wave_sum(rho);
    rr = bc_wave_sum(rr);
    if (lane == 0) { partial[wave] = rho; partial[nwaves + wave] = rr; }
}

// r = b and r^ = b over owned cells, partial[wave] = <b, b>: the start of a solve in one pass
template <int W>
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_start(GridDev g, int nf, const double *__restrict__ b, double *__restrict__ r,
                                                    double *__restrict__ rh, double *__restrict__ partial, long nwaves) {
    BC_ITEMS
    BcPack<W> bv[BC_CH];
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) bv[j] = bc_ld<W>(b, idx[j]);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < BC_CH; ++j) {
        if (ok[j]) { bc_st<W>(r, idx[j], bv[j]); bc_st<W>(rh, idx[j], bv[j]); }
#pragma unroll
        for (int q = 0; q < W; ++q) acc += ok[j] ? bv[j].v[q] * bv[j].v[q] : 0.0;
    }
    acc = bc_wave_sum(acc);
    if (lane == 0) partial[wave] = acc;
}

// second stage of the sums: one workgroup per output, fixed order (k_inner_reduce of tp_inner.hip)
__global__ __launch_bounds__(TP_BLOCK) void k_bcgs_reduce(const double *__restrict__ partial, long nwaves, double *__restrict__ out) {
    __shared__ double sh[4];
    const double *p = partial + (long)blockIdx.x * nwaves;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long i = threadIdx.x;
    for (; i + 3 * TP_BLOCK < nwaves; i += 4 * TP_BLOCK) {
        s0 += p[i]; s1 += p[i + TP_BLOCK]; s2 += p[i + 2 * TP_BLOCK]; s3 += p[i + 3 * TP_BLOCK];
    }
    for (; i < nwaves; i += TP_BLOCK) s0 += p[i];
    const double s = bc_wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- the scalar steps: one wavefront each, lane 0 works ----------------------------------------------------------------
__device__ __forceinline__ bool bc_latched(const double *st) {
    return st[BS_DONE] != 0.0 || st[BS_BRK] != 0.0 || st[BS_NAN] != 0.0 || st[BS_NEXT] != 0.0;
}
__device__ __forceinline__ void bc_publish(const double *st, double *pin) {
    if (!pin) return;
    pin[BH_RR] = st[BS_RR]; pin[BH_DONE] = st[BS_DONE]; pin[BH_BRK] = st[BS_BRK]; pin[BH_NAN] = st[BS_NAN];
    pin[BH_HALF] = st[BS_HALF]; pin[BH_NEXT] = st[BS_NEXT]; pin[BH_SS] = st[BS_SS];
}

// start of a solve: sum[0] = (b,b) = rho = ||r||^2; tol; every latch cleared; beta = 0 makes the first p = r
__global__ __launch_bounds__(64) void k_bcgs_init(double *__restrict__ st, double rtol, double atol, double *__restrict__ pin) {
    if (threadIdx.x != 0) return;
    const double b2 = st[BS_SUM];
    const bool ok = isfinite(b2);
    st[BS_RHO] = ok ? b2 : 0.0;
    st[BS_RR] = b2;
    st[BS_SS] = 0.0;
    st[BS_ALPHA] = 0.0; st[BS_OMEGA] = 0.0; st[BS_BETA] = 0.0;
    st[BS_TOL] = ok ? fmax(rtol * sqrt(b2), atol) : 0.0;
    st[BS_DONE] = (ok && b2 == 0.0) ? 1.0 : 0.0;
    st[BS_BRK] = 0.0;
    st[BS_NAN] = ok ? 0.0 : 1.0;
    st[BS_HALF] = 0.0;
    st[BS_NEXT] = 0.0;
    bc_publish(st, pin);
}

// sum[0] = (r^,v): alpha = rho / (r^,v)
__global__ __launch_bounds__(64) void k_bcgs_alpha(double *__restrict__ st) {
    if (threadIdx.x != 0) return;
    const double rv = st[BS_SUM];
    double alpha = 0.0;
    if (!isfinite(rv)) st[BS_NAN] = 1.0;
    else if (rv == 0.0) st[BS_BRK] = 1.0;
    if (!bc_latched(st)) {
        alpha = st[BS_RHO] / rv;
        if (!isfinite(alpha)) { st[BS_NAN] = 1.0; alpha = 0.0; }
    }
    st[BS_ALPHA] = alpha;
}

// sum[0] = (s,s): the half-step exit
__global__ __launch_bounds__(64) void k_bcgs_half(double *__restrict__ st) {
    if (threadIdx.x != 0) return;
    const double ss = st[BS_SUM];
    st[BS_SS] = ss;
    if (!isfinite(ss)) st[BS_NAN] = 1.0;
    else if (!bc_latched(st) && sqrt(ss) <= st[BS_TOL]) st[BS_HALF] = 1.0;
}

// sum[0] = (t,s), sum[1] = (t,t): omega = (t,s)/(t,t); 0 on the half-step exit, with (t,t) == 0 and under any latch
__global__ __launch_bounds__(64) void k_bcgs_omega(double *__restrict__ st) {
    if (threadIdx.x != 0) return;
    const double ts = st[BS_SUM], tt = st[BS_SUM + 1];
    double omega = 0.0;
    if (!isfinite(ts) || !isfinite(tt)) st[BS_NAN] = 1.0;
    if (!bc_latched(st) && st[BS_HALF] == 0.0 && tt != 0.0) {
        omega = ts / tt;
        if (!isfinite(omega)) { st[BS_NAN] = 1.0; omega = 0.0; }
    }
    if (st[BS_NAN] != 0.0) st[BS_ALPHA] = 0.0;         // (x keeps its last finite value)
    st[BS_OMEGA] = omega;
}

// sum[0] = (r^,r) = the next rho, sum[1] = (r,r): convergence, the next beta, and what the host reads
__global__ __launch_bounds__(64) void k_bcgs_end(double *__restrict__ st, double *__restrict__ pin) {
    if (threadIdx.x != 0) return;
    const double rhon = st[BS_SUM], rr = st[BS_SUM + 1];
    const double rho = st[BS_RHO], alpha = st[BS_ALPHA], omega = st[BS_OMEGA];
    st[BS_RR] = rr;
    if (!isfinite(rhon) || !isfinite(rr)) st[BS_NAN] = 1.0;
    else if (!bc_latched(st)) {
        if (sqrt(rr) <= st[BS_TOL]) st[BS_DONE] = 1.0;
        else if (rhon == 0.0 || omega == 0.0) st[BS_NEXT] = 1.0;       // (omega == 0 above the tolerance: t = J M s = 0 for s != 0)
    }
    double beta = 0.0;
    if (!bc_latched(st)) {
        beta = (rhon / rho) * (alpha / omega);
        if (!isfinite(beta)) { st[BS_NAN] = 1.0; beta = 0.0; }
        st[BS_RHO] = rhon;
    }
    st[BS_BETA] = beta;
    bc_publish(st, pin);
    // the half-step latch belongs to ONE iteration.  A half-step exit leaves r = s with the same partials, so DONE is set with
    // it; should that ever not hold, the next k_bcgs_omega must not find it
    if (st[BS_DONE] == 0.0) st[BS_HALF] = 0.0;
}

// ---- host side -------------------------------------------------------------------------------------------------------
constexpr int BCGS_NVEC = 7;           // r^, r, p, v, s, p^, s^ (t lives in w2, which no preconditioner application touches)

static long bc_nwaves(const GridDev &g, int nf, int W) { return (g.nown * nf / W + 64L * BC_CH - 1) / (64L * BC_CH); }

void bcgs_check_options(const tp_options &o) {
    TP_REQUIRE(o.ksp_kind == 0 || o.ksp_kind == 1, "ksp_kind must be 0 (fgmres) or 1 (bcgs)");
}

static void bcgs_ensure(tp_ctx *c) {
    BcgsWork &W = c->bcgs;
    const size_t nv = (size_t)c->b * c->g.ntot;
    if (W.vec.n < BCGS_NVEC * nv) W.vec.alloc(BCGS_NVEC * nv);      // once per context: the recorded pc_apply programs hold p, p^, s, s^
    const size_t np = 2 * (size_t)bc_nwaves(c->g, c->b, 1);
    if (W.partial.n < np) W.partial.alloc(np);
    if (W.state.n < (size_t)BS_SIZE) W.state.alloc(BS_SIZE);
}

void ksp_info(tp_ctx *c, int64_t out[4]) {
    out[0] = c->opt.ksp_kind;
    out[1] = (int64_t)((c->V.n + c->Z.n + c->bcgs.vec.n + c->kstage.n) * sizeof(double) + (c->Vs.n + c->Zs.n) * sizeof(float));
    out[2] = c->bcgs.vec.n ? BCGS_NVEC : 0;
    out[3] = c->pc_graph_epoch == c->graph_epoch ? (int64_t)c->pc_programs.size() : 0;
}

#define BC_LAUNCH(KERNEL, ...)                                                                   \
    do {                                                                                         \
        if (wide) hipLaunchKernelGGL(KERNEL<2>, gw, bl, 0, c->stream, __VA_ARGS__);              \
        else hipLaunchKernelGGL(KERNEL<1>, gw, bl, 0, c->stream, __VA_ARGS__);                   \
    } while (0)

// BiCGStab from x0 = 0 to the relative tolerance rtol (the latch on the device receives it through k_bcgs_init).  Returns the KSP reason: 2 converged, -3 ksp_max_it reached, -5 breakdown, -9 NaN or Inf.
int bcgs(tp_ctx *c, const double *bvec, double *x, int *its_out, double *rnorm_out, double rtol) {
    const GridDev &g = c->g;
    const int B = c->b;
    const long nv = (long)B * g.ntot;
    const int maxit = c->opt.ksp_max_it;
    TP_REQUIRE(B <= 3, "bcgs: at most three fields");
    ensure_work(c);
    bcgs_ensure(c);
    BcgsWork &W = c->bcgs;
    double *rh = W.vec.p, *r = rh + nv, *p = r + nv, *v = p + nv, *s = v + nv, *ph = s + nv, *sh = ph + nv, *t = c->w2.p;
    double *st = W.state.p, *part = W.partial.p;
    // 16-byte items: every owned range starts on an even entry and every vector on a 16-byte boundary
    bool wide = g.np % 2 == 0;
    for (const double *q : {bvec, (const double *)x, (const double *)rh, (const double *)t})
        wide = wide && ((uintptr_t)q % 16 == 0);
    wide = wide && (nv % 2 == 0);
    static const bool allow_wide = tp_switch_flag(TP_SW_BCGS_WIDE);
    wide = wide && allow_wide;
    const long nw = bc_nwaves(g, B, wide ? 2 : 1);
    const dim3 gw = xcd_grid(nw * 64, TP_BLOCK), bl(TP_BLOCK), one(1), wv(64);
    const bool use_pin = tp_use_pin();
    double *pin = use_pin ? c->h_pin : nullptr;
    double hb[BH_N] = {0};
    // sums -> (all-reduced) state; every rank forms the same coefficients and latches from the same sums
    auto reduce = [&](int n) {
        hipLaunchKernelGGL(k_bcgs_reduce, dim3(n), bl, 0, c->stream, (const double *)part, nw, st + BS_SUM);
        TP_HIP(hipGetLastError());
        allreduce_sum(c, st + BS_SUM, n);
    };
    // the one host wait of an iteration: behind the scalar kernel that published ||r||^2 and the latches
    auto wait = [&]() {
        if (pin) {
            TP_HIP(hipEventRecord(c->ev_h, c->stream));
            TP_HIP(hipEventSynchronize(c->ev_h));
            memcpy(hb, pin, sizeof(hb));
            return;
        }
        double h[BS_SIZE];
        TP_HIP(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        TP_HIP(hipStreamSynchronize(c->stream));
        hb[BH_RR] = h[BS_RR]; hb[BH_DONE] = h[BS_DONE]; hb[BH_BRK] = h[BS_BRK]; hb[BH_NAN] = h[BS_NAN];
        hb[BH_HALF] = h[BS_HALF]; hb[BH_NEXT] = h[BS_NEXT]; hb[BH_SS] = h[BS_SS];
    };
    vec_zero(c, x, nv);
    BC_LAUNCH(k_bcgs_start, g, B, bvec, r, rh, part, nw);
    reduce(1);
    hipLaunchKernelGGL(k_bcgs_init, one, wv, 0, c->stream, st, rtol, c->opt.ksp_atol, pin);
    TP_HIP(hipGetLastError());
    wait();
    *its_out = 0;
    *rnorm_out = std::sqrt(hb[BH_RR]);
    if (hb[BH_NAN] != 0.0) return -9;
    if (hb[BH_DONE] != 0.0) return 2;                      // b = 0
    for (int its = 1;; ++its) {
        BC_LAUNCH(k_bcgs_p, g, B, (const double *)st, (const double *)r, (const double *)v, p, nw);
        pc_apply(c, p, ph);                                                       // p^ = M p
        krylov_apply(c, ph, v);                                                    // v = J p^ (plus the wells' rank-1 terms)
        BC_LAUNCH(k_bcgs_dot, g, B, (const double *)rh, (const double *)v, part, nw);
        reduce(1);
        hipLaunchKernelGGL(k_bcgs_alpha, one, wv, 0, c->stream, st);
        BC_LAUNCH(k_bcgs_s, g, B, (const double *)st, (const double *)r, (const double *)v, s, part, nw);
        reduce(1);
        hipLaunchKernelGGL(k_bcgs_half, one, wv, 0, c->stream, st);
        pc_apply(c, s, sh);                                                       // s^ = M s
        krylov_apply(c, sh, t);                                                    // t = J s^
        BC_LAUNCH(k_bcgs_dot2, g, B, (const double *)t, (const double *)s, part, nw);
        reduce(2);
        hipLaunchKernelGGL(k_bcgs_omega, one, wv, 0, c->stream, st);
        BC_LAUNCH(k_bcgs_update, g, B, (const double *)st, (const double *)ph, (const double *)sh, (const double *)s,
                  (const double *)t, (const double *)rh, x, r, part, nw);
        reduce(2);
        hipLaunchKernelGGL(k_bcgs_end, one, wv, 0, c->stream, st, pin);
        TP_HIP(hipGetLastError());
        wait();
        const double res = std::sqrt(hb[BH_RR]);
        *rnorm_out = res;
        if (hb[BH_NAN] != 0.0) { *its_out = its - 1; return -9; }
        if (hb[BH_BRK] != 0.0) { *its_out = its - 1; return -5; }                  // (the iteration changed neither x nor r)
        *its_out = its;
        if (c->monitor) {
            // per-field norms of the true residual b - J x, as the FGMRES monitor reports them
            std::vector<double> fn(B, 0.0);
            double *rm = c->w4.p;                                                   // free between pc_apply calls
            if (c->dist) halo_exchange(c, g, x, B, g.ntot);
            krylov_resid(c, bvec, x, rm);
            for (int f = 0; f < B; ++f) {
                const double *one_f[1] = {rm + (long)f * g.ntot};
                multi_norm2sq(c, 1, 1, one_f, &fn[f]);
                fn[f] = std::sqrt(fn[f]);
            }
            c->monitor(its, res, fn.data(), B, c->monitor_user);
        }
        if (hb[BH_DONE] != 0.0) return 2;
        if (its >= maxit) return -3;
        if (hb[BH_NEXT] != 0.0) return -5;                                         // rho == 0: the next iteration cannot start
    }
}

}  // namespace tp
