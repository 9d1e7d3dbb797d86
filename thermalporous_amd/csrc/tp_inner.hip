// Inner Krylov solve of the stage-1 pressure block K(A00) / the (p,T) system block of pc_cptramg (tp_options.s1_ksp).
//
// What PETSc does when a sub-solver's ksp_type is not preonly: the AMG V-cycle becomes the preconditioner of a small inner
// iteration.  pc_apply is a captured hipGraph, so the host can neither read a norm nor decide to stop:
//   * exactly s1_max_it iterations are always LAUNCHED;
//   * every scalar -- the Hessenberg column, the Givens rotations, the residual estimate -- stays in InnerWork::state;
//   * convergence is a LATCH on the device: the first time the recurrence residual is <= max(s1_rtol ||rhs||, s1_atol) (or the
//     new direction vanishes: happy breakdown) the one-wavefront kernel k_inner_hess stores that iteration number j*; the
//     final kernels back-substitute over the first j* columns only and form out = sum_{i<j*} y_i Z_i.
// The result is the iterate right-preconditioned GMRES with classical Gram-Schmidt returns when it stops at j*
// (oracle/linalg.py:fgmres); the iterations launched after j* are wasted work, not different arithmetic.
// Reductions are two-stage with a fixed summation order (no floating-point atomics): two runs, and two ranks holding the
// same replicated system, agree bit for bit.  Vectors are nf planes of g.ntot doubles; sums run over owned cells.
#include "tp_common.hpp"
#include <algorithm>

namespace tp {

constexpr int IN_MAXK = 32;            // largest s1_max_it of the fgmres variant
constexpr int IN_CH = 8;               // entries per lane of the fused reductions (as TP_MD_CHUNK's default in tp_linalg.hip)
constexpr int IN_U = 4;                // basis vectors in flight together (MD_U of tp_linalg.hip)
// layout of InnerWork::state (doubles), derived from IN_MAXK; each array starts on a multiple of 8 doubles
constexpr int in_up8(int n) { return (n + 7) / 8 * 8; }
constexpr int ST_H = 0;                                // h_0 .. h_j, <w,w>          (IN_MAXK + 1 entries)
constexpr int ST_HN2 = in_up8(ST_H + IN_MAXK + 1);     // ||w - V h||^2 of the current iteration
constexpr int ST_BETA2 = ST_HN2 + 1;                   // ||rhs||^2
constexpr int ST_TOL = ST_HN2 + 2, ST_RES = ST_HN2 + 3;
constexpr int ST_JSTAR = ST_HN2 + 4;                   // latch: -1 while iterating, else the number of columns the result uses
constexpr int ST_G = ST_HN2 + 8;                       // rotated right-hand side, IN_MAXK + 1
constexpr int ST_CS = in_up8(ST_G + IN_MAXK + 1);      // rotations
constexpr int ST_SN = in_up8(ST_CS + IN_MAXK);
constexpr int ST_Y = in_up8(ST_SN + IN_MAXK);          // solution of the triangular system, zero from j* on
constexpr int ST_R = in_up8(ST_Y + IN_MAXK);           // rotated Hessenberg columns, column j at ST_R + j*IN_MAXK
constexpr int ST_SIZE = ST_R + IN_MAXK * IN_MAXK;
static_assert(IN_MAXK <= 63, "k_inner_hess / k_inner_backsolve handle a column with the lanes of ONE wavefront");
static_assert(ST_H + IN_MAXK + 1 <= ST_HN2 && ST_JSTAR < ST_G && ST_G + IN_MAXK + 1 <= ST_CS && ST_CS + IN_MAXK <= ST_SN &&
              ST_SN + IN_MAXK <= ST_Y && ST_Y + IN_MAXK <= ST_R, "InnerWork::state arrays overlap");

__device__ __forceinline__ double in_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// owned entry t of an nf-plane vector -> its index (tail lanes: entry 0, a valid address, used with weight 0 -- which is 0
// only because every stored basis vector is finite: k_inner_scale writes them with its guarded scale)
__device__ __forceinline__ long in_index(const GridDev &g, long t) {
    const long f = t / g.nown, i = t - f * g.nown;
    return f * g.ntot + g.np + i;
}

// (a) one pass over w: partial[i][wave] = <V_i, w> for i < k, partial[k][wave] = <w, w>.  A wave keeps IN_CH entries of w per
// lane in registers and streams the k basis vectors past them, IN_U vectors (IN_U*IN_CH independent loads per lane) at a time.
__global__ __launch_bounds__(256) void k_inner_dots(GridDev g, int nf, const double *__restrict__ V, long vstride, int k,
                                                    const double *__restrict__ w, double *__restrict__ partial, long nwaves) {
    const long wave = ((long)blockIdx.x * TP_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= nwaves) return;
    const long nall = g.nown * nf;
    long idx[IN_CH];
    double wv[IN_CH];
#pragma unroll
    for (int j = 0; j < IN_CH; ++j) {
        const long t = (wave * IN_CH + j) * 64 + lane;
        const bool ok = t < nall;
        idx[j] = in_index(g, ok ? t : 0);
        wv[j] = ok ? w[idx[j]] : 0.0;
    }
    int i = 0;
    for (; i + IN_U <= k; i += IN_U) {
        double v[IN_U][IN_CH], s[IN_U];
#pragma unroll
        for (int u = 0; u < IN_U; ++u)
#pragma unroll
            for (int j = 0; j < IN_CH; ++j) v[u][j] = V[(long)(i + u) * vstride + idx[j]];
#pragma unroll
        for (int u = 0; u < IN_U; ++u) {
            s[u] = 0.0;
#pragma unroll
            for (int j = 0; j < IN_CH; ++j) s[u] += v[u][j] * wv[j];
        }
#pragma unroll
        for (int u = 0; u < IN_U; ++u) s[u] = in_wave_sum(s[u]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < IN_U; ++u) partial[(long)(i + u) * nwaves + wave] = s[u];
        }
    }
    for (; i < k; ++i) {
        const double *Vi = V + (long)i * vstride;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < IN_CH; ++j) s += Vi[idx[j]] * wv[j];
        s = in_wave_sum(s);
        if (lane == 0) partial[(long)i * nwaves + wave] = s;
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < IN_CH; ++j) s += wv[j] * wv[j];
    s = in_wave_sum(s);
    if (lane == 0) partial[(long)k * nwaves + wave] = s;
}

// second stage of the sums: one workgroup per output, fixed order
__global__ __launch_bounds__(256) void k_inner_reduce(const double *__restrict__ partial, long nwaves, double *__restrict__ out) {
    __shared__ double sh[4];
    const double *p = partial + (long)blockIdx.x * nwaves;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long i = threadIdx.x;
    for (; i + 3 * 256 < nwaves; i += 4 * 256) {
        s0 += p[i]; s1 += p[i + 256]; s2 += p[i + 2 * 256]; s3 += p[i + 3 * 256];
    }
    for (; i < nwaves; i += 256) s0 += p[i];
    const double s = in_wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// (b) one pass: w -= sum_{i<k} h_i V_i with h read from the device buffer, and the per-wave partial of ||w||^2 of the result
__global__ __launch_bounds__(256) void k_inner_axpy_norm(GridDev g, int nf, const double *__restrict__ V, long vstride, int k,
                                                         const double *__restrict__ h, double *w, double *__restrict__ partial,
                                                         long nwaves) {
    const long wave = ((long)blockIdx.x * TP_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= nwaves) return;
    const long nall = g.nown * nf;
    long idx[IN_CH];
    bool ok[IN_CH];
    double s[IN_CH], w0[IN_CH];
#pragma unroll
    for (int j = 0; j < IN_CH; ++j) {
        const long t = (wave * IN_CH + j) * 64 + lane;
        ok[j] = t < nall;
        idx[j] = in_index(g, ok[j] ? t : 0);
        s[j] = 0.0;
        w0[j] = w[idx[j]];
    }
    int q = 0;
    for (; q + IN_U <= k; q += IN_U) {
        double v[IN_U][IN_CH], hq[IN_U];
#pragma unroll
        for (int u = 0; u < IN_U; ++u) {
            hq[u] = h[q + u];
#pragma unroll
            for (int j = 0; j < IN_CH; ++j) v[u][j] = V[(long)(q + u) * vstride + idx[j]];
        }
#pragma unroll
        for (int u = 0; u < IN_U; ++u)
#pragma unroll
            for (int j = 0; j < IN_CH; ++j) s[j] += hq[u] * v[u][j];
    }
    for (; q < k; ++q) {
        const double hq = h[q];
#pragma unroll
        for (int j = 0; j < IN_CH; ++j) s[j] += hq * V[(long)q * vstride + idx[j]];
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < IN_CH; ++j) {
        if (ok[j]) {
            const double wn = w0[j] - s[j];
            w[idx[j]] = wn;
            acc += wn * wn;
        }
    }
    acc = in_wave_sum(acc);
    if (lane == 0) partial[wave] = acc;
}

// y = x / sqrt(*n2) over owned cells with the guarded scale of k_scale_dev_norm (tp_linalg.hip): a zero or non-finite norm
// scales by 0, so after a happy breakdown (or with rhs = 0) the iterations still launched push zeros
__global__ __launch_bounds__(256) void k_inner_scale(GridDev g, int nf, const double *__restrict__ n2p, const double *x, double *y) {
    const long t = (long)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (t >= g.nown * nf) return;
    const double n2 = *n2p;
    const double a = (n2 > 0.0 && isfinite(n2)) ? 1.0 / sqrt(n2) : 0.0;
    const long c = in_index(g, t);
    y[c] = a * x[c];
}

// start of a solve (one wavefront): beta = ||rhs||, tolerance, g_0 = beta; rhs = 0 (or not finite) latches at once with j* = 0
__global__ __launch_bounds__(64) void k_inner_init(double *__restrict__ st, double rtol, double atol) {
    const int lane = threadIdx.x;
    if (lane < IN_MAXK) st[ST_Y + lane] = 0.0;
    if (lane != 0) return;
    const double b2 = st[ST_BETA2];
    const bool ok = b2 > 0.0 && isfinite(b2);
    const double beta = ok ? sqrt(b2) : 0.0;
    st[ST_G] = beta;
    st[ST_RES] = beta;
    st[ST_TOL] = fmax(rtol * beta, atol);
    st[ST_JSTAR] = ok ? -1.0 : 0.0;
}

// iteration j (one wavefront): previous Givens rotations on the new Hessenberg column (h_0..h_j, ||w||), the new rotation, the
// residual estimate |g_{j+1}| and the latch.  The lanes fetch the column and the rotations into LDS in parallel; the
// recurrence itself is serial and runs on lane 0 out of LDS.  Same operations, in the same order, as oracle/linalg.py:fgmres.
__global__ __launch_bounds__(64) void k_inner_hess(double *__restrict__ st, int j) {
    __shared__ double col[IN_MAXK + 2], cs[IN_MAXK], sn[IN_MAXK];
    if (st[ST_JSTAR] >= 0.0) return;                       // latched: nothing changes any more (wave-uniform)
    const int lane = threadIdx.x;
    if (lane <= j) col[lane] = st[ST_H + lane];
    if (lane < j) { cs[lane] = st[ST_CS + lane]; sn[lane] = st[ST_SN + lane]; }
    __syncthreads();
    if (lane == 0) {
        const double hn2 = st[ST_HN2];
        const double hn = sqrt(hn2);
        col[j + 1] = hn;
        for (int i = 0; i < j; ++i) {
            const double t = cs[i] * col[i] + sn[i] * col[i + 1];
            col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
            col[i] = t;
        }
        const double d = hypot(col[j], col[j + 1]);
        const double c_ = col[j] / d, s_ = col[j + 1] / d;
        col[j] = d;
        const double gj = st[ST_G + j];
        const double gn = -s_ * gj, res = fabs(gn);
        if (!isfinite(res) || !isfinite(d)) {
            st[ST_JSTAR] = (double)j;                      // this column is unusable: the result is the iterate before it
        } else {
            st[ST_CS + j] = c_;
            st[ST_SN + j] = s_;
            st[ST_G + j + 1] = gn;
            st[ST_G + j] = c_ * gj;
            st[ST_RES] = res;
            if (res <= st[ST_TOL] || !(hn2 > 0.0)) st[ST_JSTAR] = (double)(j + 1);      // converged, or happy breakdown
        }
    }
    __syncthreads();
    if (lane <= j) st[ST_R + j * IN_MAXK + lane] = col[lane];
}

// end of a solve (one wavefront): y = R^-1 g over the first j* columns (j* = k when nothing latched), the device counters
__global__ __launch_bounds__(64) void k_inner_backsolve(double *__restrict__ st, int k, long long *__restrict__ stats) {
    __shared__ double R[IN_MAXK * IN_MAXK], y[IN_MAXK];
    const int lane = threadIdx.x;
    const double js = st[ST_JSTAR];
    const int n = js >= 0.0 ? (int)js : k;
    for (int e = lane; e < n * IN_MAXK; e += 64) R[e] = st[ST_R + e];
    if (lane < IN_MAXK) y[lane] = lane < n ? st[ST_G + lane] : 0.0;
    __syncthreads();
    if (lane == 0) {
        for (int i = n - 1; i >= 0; --i) {
            double s = y[i];
            for (int q = i + 1; q < n; ++q) s -= R[q * IN_MAXK + i] * y[q];
            y[i] = s / R[i * IN_MAXK + i];
        }
        st[ST_JSTAR] = (double)n;
        stats[0] += 1;
        stats[1] += n;
        if (js < 0.0 && st[ST_RES] > st[ST_TOL]) stats[2] += 1;
    }
    __syncthreads();
    if (lane < IN_MAXK) st[ST_Y + lane] = y[lane];
}

// out = sum_{i<j*} y_i Z_i over owned cells (j* and y from the device)
__global__ __launch_bounds__(256) void k_inner_combine(GridDev g, int nf, const double *__restrict__ Z, long zstride,
                                                       const double *__restrict__ st, double *__restrict__ out) {
    const long t = (long)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (t >= g.nown * nf) return;
    const long c = in_index(g, t);
    const int n = (int)st[ST_JSTAR];
    double s = 0.0;
    int i = 0;
    for (; i + IN_U <= n; i += IN_U) {
        double v[IN_U];
#pragma unroll
        for (int u = 0; u < IN_U; ++u) v[u] = Z[(long)(i + u) * zstride + c];
#pragma unroll
        for (int u = 0; u < IN_U; ++u) s += st[ST_Y + i + u] * v[u];
    }
    for (; i < n; ++i) s += st[ST_Y + i] * Z[(long)i * zstride + c];
    out[c] = s;
}

// richardson: x += e over owned cells
__global__ __launch_bounds__(256) void k_inner_add(GridDev g, int nf, const double *__restrict__ e, double *x) {
    const long t = (long)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (t >= g.nown * nf) return;
    const long c = in_index(g, t);
    x[c] += e[c];
}
__global__ __launch_bounds__(64) void k_inner_count(long long *__restrict__ stats, int its) {
    if (threadIdx.x == 0) { stats[0] += 1; stats[1] += its; }
}

// y = z + alpha * A x for the 2x2 block of scalar 7-point stencils (pc_cptramg): both planes in one pass over x
__global__ __launch_bounds__(256) void k_inner_spmv2(GridDev g, Stencil A00, Stencil A01, Stencil A10, Stencil A11,
                                                     const double *__restrict__ x, double *__restrict__ y, double alpha,
                                                     const double *__restrict__ z) {
    const long tid = xcd_tid();
    if (tid >= g.nown) return;
    const long c = g.np + tid, nt = g.ntot;
    const long off[7] = {0, -1, 1, -(long)g.n0, (long)g.n0, -g.np, g.np};
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double x0 = x[c + off[k]], x1 = x[nt + c + off[k]];
        s0 += A00.slot(k)[c] * x0 + A01.slot(k)[c] * x1;
        s1 += A10.slot(k)[c] * x0 + A11.slot(k)[c] * x1;
    }
    y[c] = (z ? z[c] : 0.0) + alpha * s0;
    y[nt + c] = (z ? z[nt + c] : 0.0) + alpha * s1;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static long in_nwaves(const GridDev &g, int nf) { return (g.nown * nf + 64L * IN_CH - 1) / (64L * IN_CH); }
static dim3 in_wave_grid(long nw) { return dim3((unsigned)((nw * 64 + 255) / 256)); }

void inner_check_options(const tp_options &o) {
    TP_REQUIRE(o.s1_ksp >= 0 && o.s1_ksp <= 2, "s1_ksp must be 0 (preonly), 1 (richardson) or 2 (fgmres)");
    if (o.s1_ksp == 0) return;
    TP_REQUIRE(o.pc_kind != 4, "pc_bilu has no stage-1 solver: s1_ksp must be preonly");
    TP_REQUIRE(o.s1_max_it >= 1, "s1_max_it must be >= 1");
    TP_REQUIRE(o.s1_ksp != 2 || o.s1_max_it <= IN_MAXK, "s1_ksp fgmres: s1_max_it <= 32 (GMRES without restart)");
    TP_REQUIRE(o.s1_rtol >= 0.0 && o.s1_atol >= 0.0, "s1_rtol and s1_atol must be >= 0");
}

int vcycles_per_apply(const tp_ctx *c) {
    if (c->opt.pc_kind == 4) return 0;
    const int extra = c->opt.s1_ksp ? c->opt.s1_max_it - 1 : 0;      // per inner solve
    const int stages = c->opt.pc_order == 3 ? 2 : 1;                  // S stages of the order (pc_order 3 = SIS)
    const int ctr = c->opt.pc_ctr ? 1 : 0;                            // the T stage: always one V-cycle, no inner solve
    if (c->opt.fs_additive) return stages * (2 + extra) + ctr;
    if (schur_of(c->opt) && c->opt.schur_fact) return stages * (2 + extra) + ctr;     // lower, upper, diag: K(A00) once
    if (schur_of(c->opt)) return stages * (3 + 2 * extra) + ctr;      // full: K(A00) is applied twice
    return stages * (1 + extra) + ctr;
}

void inner_ensure(tp_ctx *c) {
    if (c->opt.s1_ksp == 0) return;
    InnerWork &W = c->inner;
    const int nf = sysamg_of(c->opt) ? 2 : 1, k = c->opt.s1_max_it;
    const GridDev &g = c->dist ? c->gfull : c->g;
    const size_t n = (size_t)nf * g.ntot;
    const size_t nV = c->opt.s1_ksp == 2 ? (size_t)(k + 1) * n : 2 * n, nZ = c->opt.s1_ksp == 2 ? (size_t)k * n : 0;
    const size_t nP = (size_t)(IN_MAXK + 2) * in_nwaves(g, nf);
    bool grew = false;
    if (W.V.n < nV) { W.V.alloc(nV); grew = true; }
    if (W.Z.n < nZ) { W.Z.alloc(nZ); grew = true; }
    if (W.partial.n < nP) { W.partial.alloc(nP); grew = true; }
    if (W.state.n < (size_t)ST_SIZE) { W.state.alloc(ST_SIZE); grew = true; }
    if (W.stats.n < 4) { W.stats.alloc(4); grew = true; }
    if (grew) c->graph_epoch++;          // captured pc_apply graphs hold the old addresses
}

void inner_reset_stats(tp_ctx *c) {
    if (c->inner.stats.n) TP_HIP(hipMemsetAsync(c->inner.stats.p, 0, c->inner.stats.n * sizeof(long long), c->stream));
}

// y = z + alpha * A x
static void inner_matvec(tp_ctx *c, const InnerOp &op, int nf, const double *x, double *y, double alpha, const double *z) {
    if (nf == 1) { spmv_scalar(c, op.g, op.A[0][0], x, y, alpha, z); return; }
    hipLaunchKernelGGL(k_inner_spmv2, xcd_grid(op.g.nown), dim3(256), 0, c->stream, op.g, op.A[0][0], op.A[0][1], op.A[1][0],
                       op.A[1][1], x, y, alpha, z);
    TP_HIP(hipGetLastError());
}

void inner_solve(tp_ctx *c, const InnerOp &op, const std::function<void(const double *, double *)> &prec, const double *rhs,
                 double *out, int nf) {
    if (c->opt.s1_ksp == 0) { prec(rhs, out); return; }
    InnerWork &W = c->inner;
    const GridDev &g = op.g;
    const int k = c->opt.s1_max_it;
    const long n = (long)nf * g.ntot, nall = g.nown * nf;
    TP_REQUIRE(nf == 1 || nf == 2, "inner_solve: one plane (pressure) or two ((p,T) system)");
    TP_REQUIRE(W.state.n >= (size_t)ST_SIZE && W.stats.n >= 4 && (long)W.V.n >= (c->opt.s1_ksp == 2 ? (k + 1) * n : 2 * n) &&
               (long)W.Z.n >= (c->opt.s1_ksp == 2 ? k * n : 0), "inner_solve: workspace not sized (ensure_work)");
    const dim3 bl(256), ge = grid_for(nall);
    if (c->opt.s1_ksp == 1) {
        // richardson from x0 = 0: x = V(rhs) ; x += V(rhs - A x), k - 1 times
        double *r = W.V.p, *e = W.V.p + n;
        prec(rhs, out);
        for (int it = 1; it < k; ++it) {
            inner_matvec(c, op, nf, out, r, -1.0, rhs);
            prec(r, e);
            hipLaunchKernelGGL(k_inner_add, ge, bl, 0, c->stream, g, nf, (const double *)e, out);
        }
        hipLaunchKernelGGL(k_inner_count, dim3(1), dim3(64), 0, c->stream, W.stats.p, k);
        TP_HIP(hipGetLastError());
        return;
    }
    // right-preconditioned GMRES(k), classical Gram-Schmidt, no restart
    TP_REQUIRE(k <= IN_MAXK, "s1_max_it <= 32");
    const long nw = in_nwaves(g, nf);
    TP_REQUIRE((long)W.partial.n >= (long)(k + 1) * nw, "inner_solve: reduction workspace not sized");
    const dim3 gw = in_wave_grid(nw);
    double *st = W.state.p, *part = W.partial.p;
    // beta^2 = <rhs, rhs> ; v_0 = rhs / beta
    hipLaunchKernelGGL(k_inner_dots, gw, bl, 0, c->stream, g, nf, rhs, 0L, 0, rhs, part, nw);
    hipLaunchKernelGGL(k_inner_reduce, dim3(1), bl, 0, c->stream, (const double *)part, nw, st + ST_BETA2);
    hipLaunchKernelGGL(k_inner_init, dim3(1), dim3(64), 0, c->stream, st, c->opt.s1_rtol, c->opt.s1_atol);
    hipLaunchKernelGGL(k_inner_scale, ge, bl, 0, c->stream, g, nf, (const double *)(st + ST_BETA2), rhs, W.V.p);
    for (int j = 0; j < k; ++j) {
        double *vj = W.V.p + (long)j * n, *zj = W.Z.p + (long)j * n, *w = W.V.p + (long)(j + 1) * n;
        prec(vj, zj);                                              // z_j = M^-1 v_j
        inner_matvec(c, op, nf, zj, w, 1.0, nullptr);              // w = A z_j
        hipLaunchKernelGGL(k_inner_dots, gw, bl, 0, c->stream, g, nf, (const double *)W.V.p, n, j + 1, (const double *)w, part, nw);
        hipLaunchKernelGGL(k_inner_reduce, dim3(j + 2), bl, 0, c->stream, (const double *)part, nw, st + ST_H);
        hipLaunchKernelGGL(k_inner_axpy_norm, gw, bl, 0, c->stream, g, nf, (const double *)W.V.p, n, j + 1,
                           (const double *)(st + ST_H), w, part, nw);
        hipLaunchKernelGGL(k_inner_reduce, dim3(1), bl, 0, c->stream, (const double *)part, nw, st + ST_HN2);
        hipLaunchKernelGGL(k_inner_hess, dim3(1), dim3(64), 0, c->stream, st, j);
        if (j + 1 < k)                                             // v_{j+1} = w / ||w|| (a pass of its own)
            hipLaunchKernelGGL(k_inner_scale, ge, bl, 0, c->stream, g, nf, (const double *)(st + ST_HN2), (const double *)w, w);
    }
    hipLaunchKernelGGL(k_inner_backsolve, dim3(1), dim3(64), 0, c->stream, st, k, W.stats.p);
    hipLaunchKernelGGL(k_inner_combine, ge, bl, 0, c->stream, g, nf, (const double *)W.Z.p, n, (const double *)st, out);
    TP_HIP(hipGetLastError());
}

}  // namespace tp
