// Structured semicoarsening AMG for the stage-1 pressure (and temperature) operators.
//
// Reference: the `v_cycle` dicts (singlephase.py:303-307, twophase.py:478-482) = one hypre BoomerAMG
// V-cycle per application, set up again at every Newton step (preconditioners.py:878).  hypre is not
// reproducible; this is the build's own AMG, designed for the machine: every level is a 7-point
// stencil on a box stored as 7 coalesced planes (no index arrays), set-up is one kernel per level
// (cheap enough to redo every Newton step), coarsening direction per level is decided on the host
// from mean face couplings (no device sync).  Algorithm (mirrored by oracle/linalg.py:SemiAMG):
//   C points = even indices along the level's axis a;  F point g:  w-(g) = -a_-(g)/c(g),
//   w+(g) = -a_+(g)/c(g),  c(g) = a_0(g) + sum of cross-axis off-diagonals;  R = P^T;
//   coarse row at C point f (F neighbours g-, g+):
//     A_c[-a] = a_-(f) w-(g-),  A_c[+a] = a_+(f) w+(g+),
//     A_c[d]  = a_d(f) + w+(g-) a_d(g-) + w-(g+) a_d(g+)            (cross slots),
//     A_c[0]  = -sum(off-diagonals) + rho(f) + w+(g-) rho(g-) + w-(g+) rho(g+),  rho = row sums.
//   Cycle shape: V(nu,nu) on the first amg_full_levels levels, V(coarse_pre, coarse_post) = V(0,1) below,
//   V(0, tail_post) on the levels of <= 1024 cells; every second level in between is a pure transfer level
//   (amg_mid_skip) folded into its parent's launches; damped Jacobi; dense inverse on the coarsest grid.
//
// Below the first three levels the V-cycle is bound by the ~5 us floor of a dependent kernel, not by bytes, so it
// is organised to minimise launches AND dependent memory round trips inside them:
//   * levels >= 200 000 cells: separate streaming kernels (pre-smoothing pair, residual, restriction,
//     prolongation, sweeps), XCD-aware block order, 75-80 % of HBM peak each;
//   * smaller levels: fused kernels -- [residual + restriction] and [prolongation + first post-sweep]; the cell
//     functions are branch-free (clamped addresses, unconditional loads, arithmetic selects) so that every load
//     of a kernel is issued in one batch;
//   * all levels at or below `tail_cells` cells run inside ONE single-workgroup kernel (down-sweep, dense coarse
//     solve, up-sweep) with workgroup barriers between phases, vectors in LDS, read-only arrays touched up
//     front -- for the small 2-D configurations the whole V-cycle is a single launch.
// Multi-GPU: levels [0, dist_levels) are this rank's slab of the global level (halo exchange in front of every
// kernel that reads across the slab boundary); the rest of the hierarchy is gathered and replicated.
#include "tp_common.hpp"
#include <algorithm>
#include <cstdlib>

namespace tp {

// Operator storage type R: double, or float (amg_single: the AMG is only a preconditioner inside the flexible
// Krylov method, so its operators, weights and inverse diagonals can be stored in fp32 -- 7 of the ~11 planes
// every smoothing sweep streams -- while all vectors and all arithmetic stay fp64).
template <class R>
struct StencilT {
    R *base;
    long slot_stride;
    __host__ __device__ const R *slot(int s) const { return base + (long)s * slot_stride; }
};

__device__ __forceinline__ void cell_ijk(const GridDev &g, long tid, int &i0, int &i1, int &i2) {
    // 32-bit unsigned divisions (every slab has fewer than 2^31 cells, tp_create): a 64-bit division is ~150 instructions on
    // this ISA, and the few-thousand-cell levels of a V-cycle are bound by exactly that kind of per-cell index arithmetic
    const unsigned t = (unsigned)tid, np = (unsigned)g.np, n0 = (unsigned)g.n0;
    const unsigned q2 = t / np, rem = t - q2 * np, q1 = rem / n0;
    i2 = (int)q2;
    i1 = (int)q1;
    i0 = (int)(rem - q1 * n0);
}

// ---- set-up kernels --------------------------------------------------------------------------------
// interpolation weights of every cell w.r.t. axis a (only odd cells are used) + invd = omega/diag
template <class R>
__global__ void k_amg_weights(GridDev g, StencilT<R> A, int axis, double omega, R *wm, R *wp, R *invd,
                              unsigned long long *ratio_slots) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = tid < g.nown;
    const long c = g.np + (in ? tid : 0);
    const double a0 = A.slot(0)[c];
    if (in) invd[c] = (R)(omega / a0);
    if (ratio_slots) {
        // dominance ratio sum_{s>=1}|a_s| / |a_0| of the row, max over the level (tp_options.amg_dom_tau): wave max by
        // shuffles, workgroup max through LDS, then ONE atomic per WORKGROUP on one of 64 slots (non-negative doubles order
        // like their bit patterns).  One atomic per wave -- 17 500 on 64 addresses for C4's level 0 -- serialised in the L2
        // and made this kernel 54 us instead of the 15 us its 90 MB take.
        __shared__ double wmax[16];
        double so = 0.0;
#pragma unroll
        for (int s = 1; s < 7; ++s) so += fabs((double)A.slot(s)[c]);
        double r = in ? so / fabs(a0) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = fmax(r, __shfl_down(r, o, 64));
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = wmax[0];
            for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, wmax[w]);
            atomicMax(&ratio_slots[blockIdx.x & 63], (unsigned long long)__double_as_longlong(m));
        }
    }
    if (!in || axis < 0) return;
    double cc = a0;
#pragma unroll
    for (int s = 1; s < 7; ++s)
        if ((s - 1) / 2 != axis) cc += A.slot(s)[c];
    wm[c] = (R)(-A.slot(1 + 2 * axis)[c] / cc);
    wp[c] = (R)(-A.slot(2 + 2 * axis)[c] / cc);
}

// coarse operator: one thread per coarse cell
template <class R>
__global__ void k_amg_coarsen(GridDev gf, GridDev gc, StencilT<R> A, int axis, const R *wm, const R *wp, R *Ac,
                              long cstride) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= gc.nown) return;
    int I[3];
    cell_ijk(gc, tid, I[0], I[1], I[2]);
    const long cc = gc.np + tid;
    int F[3] = {I[0], I[1], I[2]};
    F[axis] = 2 * I[axis] + par_of(gf, axis);
    const int nfa = axis == 0 ? gf.n0 : (axis == 1 ? gf.n1 : gf.n2);
    const long stride = axis == 0 ? 1 : (axis == 1 ? gf.n0 : gf.np);
    const long f = gf.np + (long)F[0] + (long)gf.n0 * F[1] + gf.np * F[2];
    const bool hm = F[axis] - 1 >= 0 || open_lo(gf, axis), hp = F[axis] + 1 < nfa || open_hi(gf, axis);
    const long gm = hm ? f - stride : f, gp = hp ? f + stride : f;      // clamped: every load below is unconditional
    const double Pm = hm ? (double)wp[gm] : 0.0;     // P[g-, I] = w+(g-)
    const double Pp = hp ? (double)wm[gp] : 0.0;     // P[g+, I] = w-(g+)
    const double Wm = hm ? (double)wm[gm] : 0.0, Wp = hp ? (double)wp[gp] : 0.0;
    double rho_f = 0.0, rho_m = 0.0, rho_p = 0.0;
    double out[7];
    double offsum = 0.0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const double af = A.slot(s)[f];
        const double lm = A.slot(s)[gm], lp = A.slot(s)[gp];
        const double am = hm ? lm : 0.0, ap = hp ? lp : 0.0;
        rho_f += af; rho_m += am; rho_p += ap;
        if (s == 0) continue;
        double v;
        if (s == 1 + 2 * axis)      v = af * Wm;
        else if (s == 2 + 2 * axis) v = af * Wp;
        else                        v = af + Pm * am + Pp * ap;
        out[s] = v;
        offsum += v;
    }
    out[0] = -offsum + rho_f + Pm * rho_m + Pp * rho_p;
#pragma unroll
    for (int s = 0; s < 7; ++s) Ac[(long)s * cstride + cc] = (R)out[s];
}

// coarsest grid: dense inverse by Gauss-Jordan in one workgroup (diagonally dominant: no pivoting)
template <class R>
__global__ void k_amg_dense_inverse(GridDev g, StencilT<R> A, int n, double *M, double *Minv) {
    const long off[7] = {0, -1, 1, -(long)g.n0, (long)g.n0, -g.np, g.np};
    for (int e = threadIdx.x; e < n * n; e += blockDim.x) { M[e] = 0.0; Minv[e] = (e / n == e % n) ? 1.0 : 0.0; }
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const long c = g.np + r;
        int i0, i1, i2;
        cell_ijk(g, r, i0, i1, i2);
        const bool has[7] = {true, i0 > 0, i0 < g.n0 - 1, i1 > 0, i1 < g.n1 - 1, i2 > 0, i2 < g.n2 - 1};
        for (int s = 0; s < 7; ++s)
            if (has[s]) M[(long)r * n + (r + off[s])] += A.slot(s)[c];
    }
    __syncthreads();
    for (int p = 0; p < n; ++p) {
        const double piv = M[(long)p * n + p];
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            M[(long)p * n + e] /= piv;
            Minv[(long)p * n + e] /= piv;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
            const int r = e / n, q = e % n;
            if (r == p) continue;
            const double fct = M[(long)r * n + p];
            Minv[(long)r * n + q] -= fct * Minv[(long)p * n + q];
            if (q != p) M[(long)r * n + q] -= fct * M[(long)p * n + q];
        }
        __syncthreads();
        for (int r = threadIdx.x; r < n; r += blockDim.x)
            if (r != p) M[(long)r * n + p] = 0.0;
        __syncthreads();
    }
}

// same, with the augmented matrix [M | I] held in LDS (n <= 64: 64 KiB, rows padded to 64 columns so that an element index
// splits into (row, column) by shift and mask) -- no global round trips, 1024 threads, three barriers per pivot: the pivot
// column is copied aside first, so the rank-1 update of a pivot is ONE phase for both halves.  Same operations in the same
// order as the global-memory kernel (bit-identical inverse); C4: 136 -> ~30 us per hierarchy and set-up.
template <class R>
__global__ __launch_bounds__(1024) void k_amg_dense_inverse_lds(GridDev g, StencilT<R> A, int n, double *Minv_out) {
    __shared__ double M[64 * 64];
    __shared__ double I[64 * 64];
    __shared__ double col[64];
    const int t = threadIdx.x, T = blockDim.x;
    const long off[7] = {0, -1, 1, -(long)g.n0, (long)g.n0, -g.np, g.np};
    for (int e = t; e < 64 * 64; e += T) { M[e] = 0.0; I[e] = ((e >> 6) == (e & 63)) ? 1.0 : 0.0; }
    __syncthreads();
    for (int r = t; r < n; r += T) {
        const long c = g.np + r;
        int i0, i1, i2;
        cell_ijk(g, r, i0, i1, i2);
        const bool has[7] = {true, i0 > 0, i0 < g.n0 - 1, i1 > 0, i1 < g.n1 - 1, i2 > 0, i2 < g.n2 - 1};
        for (int s = 0; s < 7; ++s)
            if (has[s]) M[r * 64 + (int)(r + off[s])] += (double)A.slot(s)[c];
    }
    __syncthreads();
    for (int p = 0; p < n; ++p) {
        if (t < n) col[t] = M[t * 64 + p];
        __syncthreads();
        const double piv = col[p];
        if (t < n) M[p * 64 + t] /= piv;
        else if (t >= 64 && t < 64 + n) I[p * 64 + (t - 64)] /= piv;
        __syncthreads();
        // eliminate column p from every other row: thread (r, q) updates both halves (M[r][p] becomes fct - fct * 1 = 0)
        for (int e = t; e < n * 64; e += T) {
            const int r = e >> 6, q = e & 63;
            if (r == p || q >= n) continue;
            const double fct = col[r];
            I[e] -= fct * I[p * 64 + q];
            M[e] = (q == p) ? 0.0 : M[e] - fct * M[p * 64 + q];
        }
        __syncthreads();
    }
    for (int e = t; e < n * n; e += T) Minv_out[e] = I[(e / n) * 64 + e % n];
}

// The MFMA experiment of north_star ("MFMA only in the batched small dense block factor/solve"): the same inverse as a BLOCKED
// Gauss-Jordan, four pivots at a time, whose trailing update [M | I] -= C R (C: the 64 x 4 multipliers, R: the 4 x 128 scaled
// pivot rows) is a rank-4 GEMM on v_mfma_f64_16x16x4_f64 -- 4 x 8 output tiles of 16 x 16, two per wave of a 1024-thread
// workgroup.  Operand maps (cdna_hip_programming.md): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// C/D[row = (lane >> 4) + 4 reg][col = lane & 15].  16 block steps of three barriers instead of 64 pivots of three; not
// bit-identical with the scalar kernel (different association), same inverse to round-off.  The default since it won (31 against 58 us on C4);
// TP_AMG_DENSE_MFMA=0 selects the scalar kernel; the measured comparison is in DESIGN.md 4.5.
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
template <class R>
__global__ __launch_bounds__(1024) void k_amg_dense_inverse_mfma(GridDev g, StencilT<R> A, int n, double *Minv_out) {
    extern __shared__ double lds[];
    double *X = lds;                       // [64][128]: [M | I], row stride 128
    double *Rb = X + 64 * 128;             // [4][128] scaled pivot rows
    double *Cb = Rb + 4 * 128;             // [64][4] multipliers (pivot rows: 0)
    double *Pi = Cb + 64 * 4;              // [4][4] inverse of the pivot block
    const int t = threadIdx.x, T = blockDim.x, lane = t & 63, wave = t >> 6;
    const long off[7] = {0, -1, 1, -(long)g.n0, (long)g.n0, -g.np, g.np};
    for (int e = t; e < 64 * 128; e += T) {
        const int r = e >> 7, q = e & 127;
        X[e] = (q == r + 64 || (q == r && r >= n)) ? 1.0 : 0.0;          // identity half; unit diagonal in the padding rows
    }
    __syncthreads();
    for (int r = t; r < n; r += T) {
        const long c = g.np + r;
        int i0, i1, i2;
        cell_ijk(g, r, i0, i1, i2);
        const bool has[7] = {true, i0 > 0, i0 < g.n0 - 1, i1 > 0, i1 < g.n1 - 1, i2 > 0, i2 < g.n2 - 1};
        for (int s = 0; s < 7; ++s)
            if (has[s]) X[r * 128 + (int)(r + off[s])] += (double)A.slot(s)[c];
    }
    __syncthreads();
    for (int p0 = 0; p0 < 64; p0 += 4) {
        // (1) inverse of the 4 x 4 pivot block: Gauss-Jordan in the registers of one thread
        if (t == 0) {
            double P[4][4], Q[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { P[i][j] = X[(p0 + i) * 128 + p0 + j]; Q[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const double ip = 1.0 / P[p][p];
#pragma unroll
                for (int j = 0; j < 4; ++j) { P[p][j] *= ip; Q[p][j] *= ip; }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i == p) continue;
                    const double f = P[i][p];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { P[i][j] -= f * P[p][j]; Q[i][j] -= f * Q[p][j]; }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) Pi[i * 4 + j] = Q[i][j];
        }
        __syncthreads();
        // (2) R = P^-1 [M | I](pivot rows, :) and the multipliers C = M(:, pivot columns), zero in the pivot rows
        if (t < 512) {
            const int i = t >> 7, q = t & 127;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) v += Pi[i * 4 + m] * X[(p0 + m) * 128 + q];
            Rb[i * 128 + q] = v;
        } else if (t < 768) {
            const int r = (t - 512) >> 2, j = t & 3;
            Cb[r * 4 + j] = (r >= p0 && r < p0 + 4) ? 0.0 : X[r * 128 + p0 + j];
        }
        __syncthreads();
        // (3) [M | I] -= C R on the matrix cores: wave w owns the tiles (row tile w >> 2, column tiles 2 (w & 3), + 1);
        //     the pivot rows (C = 0 there) take R itself
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int rt = wave >> 2, ct = 2 * (wave & 3) + h;
            const double a = -Cb[(rt * 16 + (lane & 15)) * 4 + (lane >> 4)];
            const double b = Rb[(lane >> 4) * 128 + ct * 16 + (lane & 15)];
            mfma_d4 acc;
            double *xp = X + (rt * 16 + (lane >> 4)) * 128 + ct * 16 + (lane & 15);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = xp[q * 4 * 128];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = rt * 16 + (lane >> 4) + 4 * q;
                xp[q * 4 * 128] = (row >= p0 && row < p0 + 4) ? Rb[(row - p0) * 128 + ct * 16 + (lane & 15)] : acc[q];
            }
        }
        __syncthreads();
    }
    for (int e = t; e < n * n; e += T) Minv_out[e] = X[(e / n) * 128 + 64 + e % n];
}

// ---- per-cell building blocks of the cycle (shared by the per-level kernels and the tail kernel) ------
template <class R>
struct LevelDevT {
    GridDev g;
    StencilT<R> op;
    const R *invd, *wm, *wp;
    double *b, *x, *x2, *e;
    int axis;
    int pre, post;           // smoothing sweeps of this level: V(pre, post); post == 0: pure transfer level
    int pad_;
    double omega;            // damping the set-up built invd with: invd[c] = (R)(omega / diag[c]) at every owned cell (k_amg_weights)
};

// omega / diag of an OWNED cell c without reading the stored plane: a kernel that streams the diagonal anyway recomputes in
// registers what k_amg_weights stored -- the same correctly rounded division, the same rounding to R, so the same bits -- and
// saves one plane in eleven of a Jacobi sweep.  (REG = false: the stored plane, TP_AMG_INVD_LOAD=1; the line, Gauss-Seidel and
// tail kernels always read the plane; pre2_cell, which needs it at neighbours too, has its own form of this.)
template <class R, bool REG>
__device__ __forceinline__ double invd_from(const LevelDevT<R> &L, R s) {      // s: the cell's diagonal (REG), or its stored omega / diag
    if constexpr (REG) return (double)(R)(L.omega / (double)s);
    else return (double)s;
}
template <class R, bool REG>
__device__ __forceinline__ double invd_at(const LevelDevT<R> &L, long c) {
    return invd_from<R, REG>(L, REG ? L.op.slot(0)[c] : L.invd[c]);
}

__device__ __forceinline__ void nb_offsets(const GridDev &g, long (&off)[7]) {
    off[0] = 0; off[1] = -1; off[2] = 1; off[3] = -(long)g.n0; off[4] = g.n0; off[5] = -g.np; off[6] = g.np;
}

// two damped-Jacobi sweeps from a zero initial guess:  x1 = invd b ;  x2 = x1 + invd (b - A x1)
// (REG: omega / diag at the cell and its six neighbours from the diagonal plane the sweep streams anyway, as invd_at forms it; a
// neighbour whose diagonal is zero -- a halo cell of a level that is not slab-distributed, where the stored plane holds the zero
// it was allocated with -- gets 0.0, and either form multiplies it by the exact zero coefficient towards a boundary)
template <class R, bool REG>
__device__ __forceinline__ double pre2_cell(const LevelDevT<R> &L, const double *__restrict__ b, long tid) {
    const long c = L.g.np + tid;
    long off[7];
    nb_offsets(L.g, off);
    double s = 0.0, ic = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const long n = c + off[k];
        double iv;
        if constexpr (REG) {
            const double d = (double)L.op.slot(0)[n];
            const double q = (double)(R)(L.omega / d);
            iv = d != 0.0 ? q : 0.0;
        } else {
            iv = (double)L.invd[n];
        }
        if (k == 0) ic = iv;
        s += L.op.slot(k)[c] * (iv * b[n]);
    }
    const double x1 = ic * b[c];
    return x1 + ic * (b[c] - s);
}

// one damped-Jacobi update from its operands: the row's coefficients a, the iterate v at the cell and its six neighbours (slot
// order), omega / diag and the right-hand side.  The ONE statement of the sweep's arithmetic: jacobi_cell and the tiled
// k_amg_prolong_jacobi_tile both call it, so the compiler contracts the two paths alike and their results agree bit for bit.
template <class R>
__device__ __forceinline__ double jacobi_update(const R (&a)[7], const double (&v)[7], double iv, double bc) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += a[k] * v[k];
    return v[0] + iv * (bc - s);
}

template <class R, bool REG = false>
__device__ __forceinline__ double jacobi_cell(const LevelDevT<R> &L, const double *__restrict__ b,
                                              const double *__restrict__ x, long tid) {
    const long c = L.g.np + tid;
    long off[7];
    nb_offsets(L.g, off);
    R a[7];
    double v[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { a[k] = L.op.slot(k)[c]; v[k] = x[c + off[k]]; }
    return jacobi_update<R>(a, v, invd_at<R, REG>(L, c), b[c]);
}

template <class R>
__device__ __forceinline__ double resid_at(const LevelDevT<R> &L, const double *__restrict__ b,
                                           const double *__restrict__ x, long c) {
    long off[7];
    nb_offsets(L.g, off);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += L.op.slot(k)[c] * x[c + off[k]];
    return b[c] - s;
}

// (P^T (b - A x)) at coarse cell tidc
template <class R>
__device__ __forceinline__ double resid_restrict_cell(const LevelDevT<R> &Lf, const GridDev &gc,
                                                      const double *__restrict__ b, const double *__restrict__ x,
                                                      long tidc) {
    int I[3];
    cell_ijk(gc, tidc, I[0], I[1], I[2]);
    const int a = Lf.axis;
    int F[3] = {I[0], I[1], I[2]};
    const GridDev &gf = Lf.g;
    F[a] = 2 * I[a] + par_of(gf, a);       // (slab-axis levels of a multi-GPU hierarchy use the unfused path)
    const int nfa = a == 0 ? gf.n0 : (a == 1 ? gf.n1 : gf.n2);
    const long stride = a == 0 ? 1 : (a == 1 ? gf.n0 : gf.np);
    const long f = gf.np + (long)F[0] + (long)gf.n0 * F[1] + gf.np * F[2];
    const bool hm = F[a] - 1 >= 0, hp = F[a] + 1 < nfa;
    const long fm = hm ? f - stride : f, fp = hp ? f + stride : f;
    const double vm = (double)Lf.wp[fm] * resid_at(Lf, b, x, fm), vp = (double)Lf.wm[fp] * resid_at(Lf, b, x, fp);
    return resid_at(Lf, b, x, f) + (hm ? vm : 0.0) + (hp ? vp : 0.0);
}

// (P^T r) at coarse cell tidc, r given as a vector
template <class R>
__device__ __forceinline__ double restrict_cell(const LevelDevT<R> &Lf, const GridDev &gc, const double *__restrict__ r,
                                                long tidc) {
    int I[3];
    cell_ijk(gc, tidc, I[0], I[1], I[2]);
    const int a = Lf.axis;
    int F[3] = {I[0], I[1], I[2]};
    const GridDev &gf = Lf.g;
    F[a] = 2 * I[a] + par_of(gf, a);
    const int nfa = a == 0 ? gf.n0 : (a == 1 ? gf.n1 : gf.n2);
    const long stride = a == 0 ? 1 : (a == 1 ? gf.n0 : gf.np);
    const long f = gf.np + (long)F[0] + (long)gf.n0 * F[1] + gf.np * F[2];
    // branch-free (see prolong_jacobi_cell): clamped addresses, unconditional loads, selected results
    const bool hm = F[a] - 1 >= 0 || open_lo(gf, a), hp = F[a] + 1 < nfa || open_hi(gf, a);
    const long fm = hm ? f - stride : f, fp = hp ? f + stride : f;
    const double vm = (double)Lf.wp[fm] * r[fm], vp = (double)Lf.wm[fp] * r[fp];
    return r[f] + (hm ? vm : 0.0) + (hp ? vp : 0.0);
}

// coarse-grid correction fused with the first post-smoothing sweep:
//   x' = x + P ec ;  out = x' + invd (b - A x')
// BRANCH-FREE: (P ec) at each of the 7 stencil points is alpha*ec[left] + beta*ec[right] with (alpha, beta) =
// (1, 0) at a C point and (w-, w+) at an F point, every address clamped into its array and every load issued
// unconditionally.  Written with `if (C point) return ...` per neighbour the loads sit behind divergent branches
// and execute as seven dependent round trips (~5 us of a 9.6 us kernel on the 10^5-cell levels); like this they are
// one batch.  Neighbours that do not exist are multiplied by their zero stencil coefficient (every level keeps
// exact zeros towards physical boundaries), so no existence tests are needed -- only memory-safe indices.
template <class R, bool MASK = true>
__device__ __forceinline__ double prolong_val(const LevelDevT<R> &Lf, const GridDev &gc, const double *__restrict__ ec,
                                              int F0, int F1, int F2) {
    const GridDev &g = Lf.g;
    const int a = Lf.axis;
    const int p = par_of(g, a);
    const int Fa = a == 0 ? F0 : (a == 1 ? F1 : F2);
    const int Ia = (Fa - p) >> 1;
    const bool isF = (Fa + p) & 1;
    const int I0 = a == 0 ? Ia : F0, I1 = a == 1 ? Ia : F1, I2 = a == 2 ? Ia : F2;
    const long ci = gc.np + (long)I0 + (long)gc.n0 * I1 + gc.np * I2;
    const long cf = g.np + (long)F0 + (long)g.n0 * F1 + g.np * F2;
    const long cs = a == 0 ? 1 : (a == 1 ? gc.n0 : gc.np);
    const int nca = a == 0 ? gc.n0 : (a == 1 ? gc.n1 : gc.n2);
    const bool hasR = isF && (Ia + 1 < nca || open_hi(gc, a));
    const double wm = (double)Lf.wm[cf], wp = (double)Lf.wp[cf];
    const double e0 = ec[ci], e1 = ec[hasR ? ci + cs : ci];
    // 0/1 FACTORS, not selects: `isF ? expr : e0` lets the compiler sink the weight loads into a branch on isF, and the seven
    // calls of a stencil then execute as seven dependent load batches (29 branches and 42 vmcnt waits in k_amg_prolong2_jacobi's
    // ISA: 8.3 us for 4096 cells).  A product with a loaded value cannot be skipped; 1.0 * x and x + 0.0 * y are exact.
    // (MASK = false: the select form, for the bandwidth-bound top levels, where the loads a C point can skip are traffic:
    // k_amg_prolong_add 7.6 -> 9.5 us on C4's level 0 with factors, k_amg_prolong2_jacobi 8.3 -> 5.9 us on the small levels)
    if constexpr (!MASK) return isF ? wm * e0 + (hasR ? wp * e1 : 0.0) : e0;
    const double fF = isF ? 1.0 : 0.0, fR = hasR ? 1.0 : 0.0;
    return (1.0 - fF) * e0 + fF * (wm * e0 + fR * (wp * e1));
}

// x' = x + P ec at the fine cell (F0, F1, F2), rounded once: what k_amg_prolong_add stores, and what k_amg_prolong_jacobi_tile
// keeps on chip instead -- one statement for both, so that they hold the same bits
template <class R>
__device__ __forceinline__ double prolong_added(const LevelDevT<R> &Lf, const GridDev &gc, const double *__restrict__ ec,
                                                const double *x, int F0, int F1, int F2) {
    return x[Lf.g.np + (long)F0 + (long)Lf.g.n0 * F1 + Lf.g.np * F2] + prolong_val<R, false>(Lf, gc, ec, F0, F1, F2);
}

template <class R, bool REG = false>
__device__ __forceinline__ double prolong_jacobi_cell(const LevelDevT<R> &Lf, const GridDev &gc,
                                                      const double *__restrict__ b, const double *x,
                                                      const double *__restrict__ ec, long tid) {
    const GridDev &g = Lf.g;
    int i0, i1, i2;
    cell_ijk(g, tid, i0, i1, i2);
    const long c = g.np + tid;
    // memory-safe neighbour coordinates (halo planes along axis 2 are part of the arrays)
    const int m0 = max(i0 - 1, 0), p0 = min(i0 + 1, g.n0 - 1);
    const int m1 = max(i1 - 1, 0), p1 = min(i1 + 1, g.n1 - 1);
    const int m2 = max(i2 - 1, g.nb_lo ? -1 : 0), p2 = min(i2 + 1, g.nb_hi ? g.n2 : g.n2 - 1);
    double v[7];
    v[0] = prolong_val(Lf, gc, ec, i0, i1, i2);
    v[1] = prolong_val(Lf, gc, ec, m0, i1, i2);
    v[2] = prolong_val(Lf, gc, ec, p0, i1, i2);
    v[3] = prolong_val(Lf, gc, ec, i0, m1, i2);
    v[4] = prolong_val(Lf, gc, ec, i0, p1, i2);
    v[5] = prolong_val(Lf, gc, ec, i0, i1, m2);
    v[6] = prolong_val(Lf, gc, ec, i0, i1, p2);
    if (x) {            // (uniform over the launch) x == nullptr: no pre-smoothing, the level's iterate is zero
        const long cn[7] = {c, c + (m0 - i0), c + (p0 - i0), c + (long)g.n0 * (m1 - i1), c + (long)g.n0 * (p1 - i1),
                            c + g.np * (m2 - i2), c + g.np * (p2 - i2)};
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] += x[cn[k]];
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += (double)Lf.op.slot(k)[c] * v[k];
    return v[0] + invd_at<R, REG>(Lf, c) * (b[c] - s);
}

// ---- two levels at once: a smoothed level l followed by a pure transfer level l+1 (amg_mid_skip) ------------
// Replicated grids only (no slab parity).  Branch-free like the single-level versions.
// (P_l^T r) at the level-(l+1) cell (I0,I1,I2), by coordinates
template <class R>
__device__ __forceinline__ double restrict_at(const LevelDevT<R> &Lf, const double *__restrict__ r, int I0, int I1, int I2) {
    const GridDev &gf = Lf.g;
    const int a = Lf.axis;
    const int F0 = a == 0 ? 2 * I0 : I0, F1 = a == 1 ? 2 * I1 : I1, F2 = a == 2 ? 2 * I2 : I2;
    const int Fa = a == 0 ? F0 : (a == 1 ? F1 : F2);
    const int nfa = a == 0 ? gf.n0 : (a == 1 ? gf.n1 : gf.n2);
    const long stride = a == 0 ? 1 : (a == 1 ? gf.n0 : gf.np);
    const long f = gf.np + (long)F0 + (long)gf.n0 * F1 + gf.np * F2;
    const bool hm = Fa - 1 >= 0, hp = Fa + 1 < nfa;
    const long fm = hm ? f - stride : f, fp = hp ? f + stride : f;
    const double vm = (double)Lf.wp[fm] * r[fm], vp = (double)Lf.wm[fp] * r[fp];
    return r[f] + (hm ? vm : 0.0) + (hp ? vp : 0.0);
}
// (P_{l+1}^T P_l^T r) at the level-(l+2) cell tid2
template <class R>
__device__ __forceinline__ double restrict2_cell(const LevelDevT<R> &L0, const LevelDevT<R> &L1, const GridDev &g2,
                                                 const double *__restrict__ r, long tid2) {
    int I[3];
    cell_ijk(g2, tid2, I[0], I[1], I[2]);
    const GridDev &g1 = L1.g;
    const int a = L1.axis;
    int M[3] = {I[0], I[1], I[2]};
    M[a] = 2 * I[a];
    const int n1a = a == 0 ? g1.n0 : (a == 1 ? g1.n1 : g1.n2);
    const long stride = a == 0 ? 1 : (a == 1 ? g1.n0 : g1.np);
    const long m = g1.np + (long)M[0] + (long)g1.n0 * M[1] + g1.np * M[2];
    const bool hm = M[a] - 1 >= 0, hp = M[a] + 1 < n1a;
    int Mm[3] = {M[0], M[1], M[2]}, Mp[3] = {M[0], M[1], M[2]};
    Mm[a] -= hm ? 1 : 0;
    Mp[a] += hp ? 1 : 0;
    const double v0 = restrict_at(L0, r, M[0], M[1], M[2]);
    const double vm = (double)L1.wp[hm ? m - stride : m] * restrict_at(L0, r, Mm[0], Mm[1], Mm[2]);
    const double vp = (double)L1.wm[hp ? m + stride : m] * restrict_at(L0, r, Mp[0], Mp[1], Mp[2]);
    return v0 + (hm ? vm : 0.0) + (hp ? vp : 0.0);
}
// (P_l P_{l+1} e2) at the level-l cell (F0,F1,F2) (clamped coordinates)
template <class R>
__device__ __forceinline__ double prolong2_val(const LevelDevT<R> &L0, const LevelDevT<R> &L1, const GridDev &g2,
                                               const double *__restrict__ e2, int F0, int F1, int F2) {
    const GridDev &g = L0.g, &g1 = L1.g;
    const int a = L0.axis;
    const int Fa = a == 0 ? F0 : (a == 1 ? F1 : F2);
    const int Ia = Fa >> 1;
    const bool isF = Fa & 1;
    const int n1a = a == 0 ? g1.n0 : (a == 1 ? g1.n1 : g1.n2);
    const bool hasR = isF && (Ia + 1 < n1a);
    const int I0 = a == 0 ? Ia : F0, I1 = a == 1 ? Ia : F1, I2 = a == 2 ? Ia : F2;
    const int J0 = I0 + (a == 0 && hasR), J1 = I1 + (a == 1 && hasR), J2 = I2 + (a == 2 && hasR);
    const long cf = g.np + (long)F0 + (long)g.n0 * F1 + g.np * F2;
    const double wm = (double)L0.wm[cf], wp = (double)L0.wp[cf];
    const double v0 = prolong_val(L1, g2, e2, I0, I1, I2), v1 = prolong_val(L1, g2, e2, J0, J1, J2);
    const double fF = isF ? 1.0 : 0.0, fR = hasR ? 1.0 : 0.0;          // (factors, not selects: see prolong_val)
    return (1.0 - fF) * v0 + fF * (wm * v0 + fR * (wp * v1));
}
// x' = P_l P_{l+1} e2 ;  out = x' + invd (b - A x')     (level l has no pre-smoothing)
template <class R, bool REG = false>
__device__ __forceinline__ double prolong2_jacobi_cell(const LevelDevT<R> &L0, const LevelDevT<R> &L1, const GridDev &g2,
                                                       const double *__restrict__ b, const double *__restrict__ e2,
                                                       long tid) {
    const GridDev &g = L0.g;
    int i0, i1, i2;
    cell_ijk(g, tid, i0, i1, i2);
    const long c = g.np + tid;
    const int m0 = max(i0 - 1, 0), p0 = min(i0 + 1, g.n0 - 1);
    const int m1 = max(i1 - 1, 0), p1 = min(i1 + 1, g.n1 - 1);
    const int m2 = max(i2 - 1, 0), p2 = min(i2 + 1, g.n2 - 1);
    double v[7];
    v[0] = prolong2_val(L0, L1, g2, e2, i0, i1, i2);
    v[1] = prolong2_val(L0, L1, g2, e2, m0, i1, i2);
    v[2] = prolong2_val(L0, L1, g2, e2, p0, i1, i2);
    v[3] = prolong2_val(L0, L1, g2, e2, i0, m1, i2);
    v[4] = prolong2_val(L0, L1, g2, e2, i0, p1, i2);
    v[5] = prolong2_val(L0, L1, g2, e2, i0, i1, m2);
    v[6] = prolong2_val(L0, L1, g2, e2, i0, i1, p2);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += (double)L0.op.slot(k)[c] * v[k];
    return v[0] + invd_at<R, REG>(L0, c) * (b[c] - s);
}

// ---- per-level kernels (big levels) -----------------------------------------------------------------
template <class R, bool REG>
__global__ __launch_bounds__(256) void k_amg_pre(LevelDevT<R> L, const double *b, int two, double *out) {
    const long tid = xcd_tid();
    if (tid >= L.g.nown) return;
    const long c = L.g.np + tid;
    out[c] = two ? pre2_cell<R, REG>(L, b, tid) : invd_at<R, REG>(L, c) * b[c];
}
template <class R, bool REG>
__global__ __launch_bounds__(256) void k_amg_jacobi(LevelDevT<R> L, const double *b, const double *x, double *out) {
    const long tid = xcd_tid();
    if (tid >= L.g.nown) return;
    out[L.g.np + tid] = jacobi_cell<R, REG>(L, b, x, tid);
}
template <class R>
__global__ __launch_bounds__(256) void k_amg_resid_restrict(LevelDevT<R> Lf, GridDev gc, const double *b,
                                                            const double *x, double *rc) {
    const long tid = xcd_tid();
    if (tid >= gc.nown) return;
    rc[gc.np + tid] = resid_restrict_cell(Lf, gc, b, x, tid);
}
template <class R, bool REG>
__global__ __launch_bounds__(256) void k_amg_prolong_jacobi(LevelDevT<R> Lf, GridDev gc, const double *b,
                                                            const double *x, const double *ec, double *out) {
    const long tid = xcd_tid();
    if (tid >= Lf.g.nown) return;
    out[Lf.g.np + tid] = prolong_jacobi_cell<R, REG>(Lf, gc, b, x, ec, tid);
}

template <class R>
__global__ __launch_bounds__(256) void k_amg_restrict2(LevelDevT<R> L0, LevelDevT<R> L1, GridDev g2, const double *r,
                                                       double *rc) {
    const long tid = xcd_tid();
    if (tid >= g2.nown) return;
    rc[g2.np + tid] = restrict2_cell(L0, L1, g2, r, tid);
}
template <class R, bool REG>
__global__ __launch_bounds__(256) void k_amg_prolong2_jacobi(LevelDevT<R> L0, LevelDevT<R> L1, GridDev g2, const double *b,
                                                             const double *e2, double *out) {
    const long tid = xcd_tid();
    if (tid >= L0.g.nown) return;
    out[L0.g.np + tid] = prolong2_jacobi_cell<R, REG>(L0, L1, g2, b, e2, tid);
}

// unfused variants for the top levels, where the fused kernels are issue-bound rather than HBM-bound
template <class R>
__global__ __launch_bounds__(256) void k_amg_resid(LevelDevT<R> L, const double *__restrict__ b,
                                                   const double *__restrict__ x, double *__restrict__ r) {
    const long tid = xcd_tid();
    if (tid >= L.g.nown) return;
    r[L.g.np + tid] = resid_at(L, b, x, L.g.np + tid);
}
template <class R>
__global__ __launch_bounds__(256) void k_amg_restrict(LevelDevT<R> Lf, GridDev gc, const double *__restrict__ r,
                                                      double *__restrict__ rc) {
    const long tid = xcd_tid();
    if (tid >= gc.nown) return;
    rc[gc.np + tid] = restrict_cell(Lf, gc, r, tid);
}
// Residual + restriction of a top level in ONE launch that neither stores the residual (k_amg_resid -> k_amg_restrict: a
// plane written and read back) nor recomputes it (k_amg_resid_restrict: three residuals per coarse cell, issue-bound up here).
// Every thread owns K FINE cells of a tile: r = b - A x by resid_at, loads coalesced along axis 0 as in k_amg_resid; the
// products wp r and wm r -- restrict_cell's vm of the C cell after it and vp of the C cell before it, the same two operands, so
// the same bits -- go to LDS, and after one barrier the owners of the C cells add r + (hm ? vm : 0) + (hp ? vp : 0) in
// restrict_cell's order.  Restriction couples cells along the coarsening axis a only, so a tile shares nothing with its
// neighbours but the single F cell at each end along a, which both evaluate:
//   a = 1, 2: a tile is W cells of a row x H cells along a (row: a line of n0 cells for a = 1, a whole plane for a = 2;
//             W H <= K TP_BLOCK, H odd, slot s = j TP_BLOCK + thread is cell (s % W, s / W)), starts and ends on an F cell and
//             writes its (H - 1) / 2 C cells per column: H residuals for H - 1 cells of the level;
//   a = 0:    (FLAT) a tile is TP_BLOCK consecutive cells of the level, cut anywhere -- C/F parity comes from each cell's own i0,
//             a line's last cell never pairs with the next line's first -- and writes the C cells among its inner TP_BLOCK - 2.
// Cells outside the level (a tile's overhang) compute on clamped addresses and are never selected: no branch around a load.
// Launched where the transfer does not cross a slab boundary (par_of = 0, no open ends: vcycle_impl keeps the two launches there).
struct RrTile {
    int W, H;               // tile: W cells along the row, H along the coarsening axis
    int nr, nfa;            // row length, fine extent along the coarsening axis
    unsigned ntw, nta;      // tiles per row, tiles along the coarsening axis
    unsigned ntiles;
    long sa, so;            // fine strides: along the coarsening axis, from row set to row set (a = 1: plane to plane)
    long csa, cso;          // the same on the coarse grid
};
template <class R, bool FLAT, int K>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_resid_restrict_tile(LevelDevT<R> Lf, GridDev gc, RrTile T,
                                                                      const double *__restrict__ b,
                                                                      const double *__restrict__ x, double *__restrict__ rc) {
    constexpr int NS = K * TP_BLOCK;                                // cells of a tile at most: K per thread
    __shared__ double s_m[NS], s_p[NS];
    const unsigned nb = gridDim.x, bi = blockIdx.x;
    const unsigned tile = (bi & 7u) * (nb >> 3) + (bi >> 3);       // xcd_tid's block order: neighbouring tiles share an L2
    if (tile >= T.ntiles) return;                                   // (whole workgroups of the grid's padding)
    const int t = (int)threadIdx.x;
    const GridDev &g = Lf.g;
    double r[K];
    long cc[K];             // the coarse cell a slot writes if its fine cell is a C cell
    bool outc[K], hm[K], hp[K];
    int lm[K], lp[K];       // LDS slots of the F neighbours
    unsigned tw = 0, ta = 0, to = 0;
    if constexpr (!FLAT) {
        const unsigned rest = tile / T.ntw;
        tw = tile - rest * T.ntw;
        to = rest / T.nta;
        ta = rest - to * T.nta;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = j * TP_BLOCK + t;
        long c, cw;         // the fine cell of this slot, clamped into the level; where it reads its weights
        if constexpr (FLAT) {
            const long raw = (long)tile * (TP_BLOCK - 2) - 1 + t;
            const long tid = raw < 0 ? 0 : (raw < g.nown ? raw : g.nown - 1);
            int i0, i1, i2;
            cell_ijk(g, tid, i0, i1, i2);
            c = g.np + tid;
            cc[j] = gc.np + (long)(i0 >> 1) + (long)gc.n0 * i1 + gc.np * i2;
            outc[j] = raw == tid && t >= 1 && t <= TP_BLOCK - 2 && !(i0 & 1);
            hm[j] = i0 - 1 >= 0;
            hp[j] = i0 + 1 < g.n0;
            lm[j] = max(t - 1, 0);
            lp[j] = min(t + 1, TP_BLOCK - 1);
            cw = c;
        } else {
            const int h = (int)((unsigned)s / (unsigned)T.W), w = s - h * T.W;
            const int q = (int)tw * T.W + w, fa = (int)ta * (T.H - 1) - 1 + h;
            const int qc = min(q, T.nr - 1), fc = min(max(fa, 0), T.nfa - 1);
            c = g.np + (long)qc + T.sa * fc + T.so * to;
            cc[j] = gc.np + (long)qc + T.csa * (fc >> 1) + T.cso * to;
            outc[j] = q == qc && fa == fc && h < T.H && (h & 1);    // (H - 1 is even: odd h <=> even fa <=> C cell)
            hm[j] = fa - 1 >= 0;
            hp[j] = fa + 1 < T.nfa;
            lm[j] = s >= T.W ? s - T.W : s;
            lp[j] = s + T.W < NS ? s + T.W : s;
            // whole rows are C rows here and nobody reads a C cell's products: it loads the weights of the F cell next to it, a
            // line the F row's own threads fetch anyway, so that half of the two weight planes never leaves HBM
            cw = c + ((h & 1) ? (hp[j] ? T.sa : -T.sa) : 0);
        }
        r[j] = resid_at(Lf, b, x, c);
        s_m[s] = (double)Lf.wp[cw] * r[j];
        s_p[s] = (double)Lf.wm[cw] * r[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double vm = s_m[lm[j]], vp = s_p[lp[j]];
        if (outc[j]) rc[cc[j]] = r[j] + (hm[j] ? vm : 0.0) + (hp[j] ? vp : 0.0);
    }
}
// the tile of a level, RR_K cells per thread.  Rows: planes for a = 2 (W = 32), lines of n0 cells for a = 1 (W in [16, 36], the
// one that wastes the fewest slots on the lines' ends and the tile's last row).  H: the tiles along a share its coarse cells
// evenly, so that the last one does not hang over the level's end (C4, 5100-cell planes: 32 x 15 on 220 and 110 planes).
constexpr int RR_K = 2;
static RrTile rr_tile(const GridDev &gf, const GridDev &gc, int a) {
    RrTile T = {};
    if (a == 0) {
        T.ntiles = (unsigned)((gf.nown + TP_BLOCK - 3) / (TP_BLOCK - 2));
        return T;
    }
    const int NS = RR_K * TP_BLOCK;
    T.nr = a == 1 ? gf.n0 : (int)gf.np;
    T.nfa = a == 1 ? gf.n1 : gf.n2;
    T.sa = a == 1 ? gf.n0 : gf.np;
    T.so = a == 1 ? gf.np : 0;
    T.csa = a == 1 ? gc.n0 : gc.np;
    T.cso = a == 1 ? gc.np : 0;
    T.W = 32;
    if (a == 1) {
        double best = 0.0;
        for (int W = 16; W <= 36; ++W) {
            const int H = (NS / W - 1) | 1;
            const double e = (double)T.nr / ((double)((T.nr + W - 1) / W) * W) * (W * (H - 1));
            if (e > best) { best = e; T.W = W; }
        }
    }
    const long nca = (T.nfa + 1) / 2, per_max = (((NS / T.W - 1) | 1) - 1) / 2;
    T.nta = (unsigned)((nca + per_max - 1) / per_max);
    T.H = 2 * (int)((nca + T.nta - 1) / T.nta) + 1;
    T.ntw = (unsigned)((T.nr + T.W - 1) / T.W);
    T.ntiles = T.ntw * T.nta * (unsigned)(a == 1 ? gf.n2 : 1);
    return T;
}
// x = P ec: the up-sweep of a pure transfer level
template <class R>
__global__ __launch_bounds__(256) void k_amg_prolong_set(LevelDevT<R> Lf, GridDev gc, const double *__restrict__ ec,
                                                         double *__restrict__ out) {
    const long tid = xcd_tid();
    if (tid >= Lf.g.nown) return;
    int i0, i1, i2;
    cell_ijk(Lf.g, tid, i0, i1, i2);
    out[Lf.g.np + tid] = prolong_val<R, false>(Lf, gc, ec, i0, i1, i2);
}
template <class R>
__global__ __launch_bounds__(256) void k_amg_prolong_add(LevelDevT<R> Lf, GridDev gc, const double *__restrict__ ec,
                                                         double *x) {
    const long tid = xcd_tid();
    if (tid >= Lf.g.nown) return;
    int i0, i1, i2;
    cell_ijk(Lf.g, tid, i0, i1, i2);
    x[Lf.g.np + tid] = prolong_added<R>(Lf, gc, ec, x, i0, i1, i2);
}

// Coarse correction + first post-sweep of a top level in ONE launch that neither stores the corrected iterate x' = x + P ec
// (k_amg_prolong_add -> k_amg_jacobi: a plane written and read back) nor forms it seven times per cell (k_amg_prolong_jacobi:
// issue-bound up here).  A workgroup owns a RUN of TP_BLOCK consecutive cells of one plane (flat in-plane index q = i0 + n0 i1, cut
// anywhere: lines of any length), one cell per thread:
//   - x' of the run (prolong_added, the value k_amg_prolong_add stores) goes to LDS together with the run's halo -- the n0 cells
//     before and the n0 cells after it, which hold the -+n0 neighbours of its first and last cells and the -+1 neighbours of its
//     ends --, formed by the same expression, at most NH per thread (2 n0 <= NH TP_BLOCK); after ONE barrier the four in-plane
//     neighbours come from LDS;
//   - x' of the two out-of-plane neighbours is formed directly, by the same expression;
//   - jacobi_update adds the row in jacobi_cell's order.
// x' is formed 3 + 2 n0 / TP_BLOCK times per cell instead of 7 (C4, n0 = 85: 3.66), in prolong_val's select form: the weight
// loads a C cell skips are traffic up here.  The row's own operands are requested after the first two x', in front of the others
// (measured: DESIGN.md 4.5).  Every coordinate is clamped into the level and every address is in its array: cells outside the
// level (the overhang of a plane's last run, a halo slot beyond the plane's ends, the planes below the first and above the last)
// compute on real cells and are either never selected or multiplied by the exact zero coefficient every level keeps towards a
// physical boundary.  The whole workgroup reaches the barrier; only whole workgroups of the grid's padding return, before it.
// Levels that are not slab-distributed only (par_of = 0, no open ends: vcycle_impl keeps the two launches and the halo exchange
// between them there).
constexpr int PJ_NH_MAX = 4;                // n0 <= PJ_NH_MAX TP_BLOCK / 2 = 512 (vcycle_impl: wider levels keep the two launches)
template <class R, bool REG, int NH>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_prolong_jacobi_tile(LevelDevT<R> Lf, GridDev gc, unsigned nruns, unsigned ntiles,
                                                                      const double *__restrict__ b,
                                                                      const double *__restrict__ x,
                                                                      const double *__restrict__ ec, double *__restrict__ out) {
    __shared__ double s_x[(NH + 1) * TP_BLOCK];                     // n0 halo cells, the run, n0 halo cells
    const unsigned nb = gridDim.x, bi = blockIdx.x;
    const unsigned tile = (bi & 7u) * (nb >> 3) + (bi >> 3);       // xcd_tid's block order: neighbouring runs share an L2
    if (tile >= ntiles) return;                                     // (whole workgroups of the grid's padding)
    const int t = (int)threadIdx.x;
    const GridDev &g = Lf.g;
    const int n0 = g.n0, npl = (int)g.np;
    const int k = (int)(tile / nruns);
    const int q0 = (int)(tile - (unsigned)k * nruns) * TP_BLOCK;
    const int q = q0 + t, qc = min(q, npl - 1);
    const int i1 = (int)((unsigned)qc / (unsigned)n0), i0 = qc - i1 * n0;
    const long c = g.np + (long)qc + g.np * k;
    const double xm = prolong_added<R>(Lf, gc, ec, x, i0, i1, max(k - 1, 0));
    const double xc = prolong_added<R>(Lf, gc, ec, x, i0, i1, k);
    R a[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) a[s] = Lf.op.slot(s)[c];
    const R ivs = REG ? a[0] : Lf.invd[c];
    const double bc = b[c];
    const double xp = prolong_added<R>(Lf, gc, ec, x, i0, i1, min(k + 1, g.n2 - 1));
    s_x[n0 + t] = xc;
#pragma unroll
    for (int m = 0; m < NH; ++m) {
        const int h = m * TP_BLOCK + t;
        const int r = h < n0 ? h : h + TP_BLOCK;                    // slot r holds the plane's cell q0 - n0 + r
        const int qh = min(max(q0 - n0 + r, 0), npl - 1);
        const int h1 = (int)((unsigned)qh / (unsigned)n0);
        const double xh = prolong_added<R>(Lf, gc, ec, x, qh - h1 * n0, h1, k);
        if (h < 2 * n0) s_x[r] = xh;
    }
    __syncthreads();
    const double v[7] = {xc, s_x[n0 + t - 1], s_x[n0 + t + 1], s_x[t], s_x[2 * n0 + t], xm, xp};
    const double y = jacobi_update<R>(a, v, invd_from<R, REG>(Lf, ivs), bc);
    if (q < npl) out[c] = y;
}
// ---- line relaxation along axis 0 (tp_options.amg_line_levels) ------------------------------------------------
// x <- x + omega T^-1 (b - A x), T = tridiag(A[1], A[0], A[2]) along axis 0: one independent system per line (i1, i2), solved
// by the Thomas algorithm with factors computed once per set-up.  Axis 0 is the fastest in memory, so G consecutive lines
// (flattened index i1 + n1 i2) are one contiguous run of G n0 doubles: a workgroup owns such a run.  The factor streams are
// stored line-transposed, [group][i0][line of the group], so that with lane <-> line and step <-> i0 every step's loads are
// contiguous over the lanes.
struct LineDev {
    const double *m, *invd, *ap;   // m_i = a-_i / d~_{i-1} (m_0 = 0), 1 / d~_i, a+_i
    int G, S;                      // lines per workgroup; line stride of the LDS image in doubles (odd: ds_read_b64 of lane-per-
                                   // line addresses j S + i hits 32 different bank pairs per half-wave)
};

// set-up: d~_0 = a0_0, m_i = a-_i / d~_{i-1}, d~_i = a0_i - m_i a+_{i-1}.  One lane per line, one workgroup per group: the stores are
// contiguous over the lanes; the loads walk each lane's own line (neighbouring steps share cache lines), once per set-up.
template <class R>
__global__ __launch_bounds__(64) void k_amg_line_factor(GridDev g, StencilT<R> A, int G, double *m, double *invd, double *ap) {
    const long nlines = (long)g.n1 * g.n2;
    const long line = (long)blockIdx.x * G + threadIdx.x;
    if ((int)threadIdx.x >= G || line >= nlines) return;
    const int n0 = g.n0;
    const long c = g.np + line * n0;
    long q = (long)blockIdx.x * n0 * G + threadIdx.x;
    double d = (double)A.slot(0)[c];
    m[q] = 0.0;
    invd[q] = 1.0 / d;
    ap[q] = (double)A.slot(2)[c];
    for (int i = 1; i < n0; ++i) {
        q += G;
        const double mi = (double)A.slot(1)[c + i] / d;
        d = (double)A.slot(0)[c + i] - mi * (double)A.slot(2)[c + i - 1];
        m[q] = mi;
        invd[q] = 1.0 / d;
        ap[q] = (double)A.slot(2)[c + i];
    }
}

// one sweep, out = x + omega T^-1 (b - A x); ZERO: the first sweep from the zero guess, out = omega T^-1 b (x is not read).
// Like k_amg_jacobi it reads only the OLD iterate (x != out) and depends on no other workgroup.
//   A: every thread, cell by cell: the full 7-point residual into the LDS image [line][i0]
//   B: lane j < lines of the group: forward y_i = r_i - m_i y_{i-1}, backward e_i = (y_i - a+_i e_{i+1}) / d~_i, in place
//   C: every thread: out = x + omega e
template <class R, bool ZERO>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_line_sweep(LevelDevT<R> L, LineDev F, double omega, const double *__restrict__ b,
                                                             const double *__restrict__ x, double *__restrict__ out) {
    extern __shared__ double img[];          // G x S
    const int n0 = L.g.n0, G = F.G, S = F.S, t = threadIdx.x;
    const long nlines = (long)L.g.n1 * L.g.n2, line0 = (long)blockIdx.x * G;
    const int nl = (int)(nlines - line0 < G ? nlines - line0 : G);          // ragged last group
    const int ncell = nl * n0;
    const long c0 = L.g.np + line0 * n0;
    for (int idx = t; idx < ncell; idx += TP_BLOCK) {
        const unsigned j = (unsigned)idx / (unsigned)n0, i = (unsigned)idx - j * (unsigned)n0;
        double r;
        if constexpr (ZERO) r = b[c0 + idx];
        else r = resid_at(L, b, x, c0 + idx);
        img[j * S + i] = r;
    }
    __syncthreads();
    if (t < nl) {
        double *y = img + t * S;
        const long q0 = (long)blockIdx.x * n0 * G + t;
        double v = y[0];
#pragma unroll 4
        for (int i = 1; i < n0; ++i) {
            v = y[i] - F.m[q0 + (long)i * G] * v;
            y[i] = v;
        }
        v *= F.invd[q0 + (long)(n0 - 1) * G];
        y[n0 - 1] = v;
#pragma unroll 4
        for (int i = n0 - 2; i >= 0; --i) {
            const long q = q0 + (long)i * G;
            v = (y[i] - F.ap[q] * v) * F.invd[q];
            y[i] = v;
        }
    }
    __syncthreads();
    for (int idx = t; idx < ncell; idx += TP_BLOCK) {
        const unsigned j = (unsigned)idx / (unsigned)n0, i = (unsigned)idx - j * (unsigned)n0;
        const double e = omega * img[j * S + i];
        if constexpr (ZERO) out[c0 + idx] = e;
        else out[c0 + idx] = x[c0 + idx] + e;
    }
}

// ---- red-black Gauss-Seidel (tp_options.amg_gs_levels) ---------------------------------------------------------
// Cell (i0, i1, i2) is red (colour 0) when i0 + i1 + i2 is even, black (colour 1) otherwise: the six neighbours of a cell of a
// 7-point stencil have the other colour, so the cells of one colour do not couple and a half-sweep over one colour,
//     x_i <- x_i + (b_i - (A x)_i) / a0_i      (no damping),
// is order-independent.  The colour comes from the cell's indices, not from the parity of its linear index (they differ as
// soon as n0 or n0 n1 is even).  One thread per cell in the XCD-aware order, like k_amg_jacobi, and the same cache lines: every
// lane loads its stencil row, b and the seven x values unconditionally (the halo planes make every address valid); a lane of the
// other colour stores its x unchanged, so the stores are whole lines and the level's x / x2 ping-pong as in the Jacobi path.
template <class R>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_gs_half(LevelDevT<R> L, int colour, const double *__restrict__ b,
                                                          const double *__restrict__ x, double *__restrict__ out) {
    const long tid = xcd_tid();
    if (tid >= L.g.nown) return;
    int i0, i1, i2;
    cell_ijk(L.g, tid, i0, i1, i2);
    const long c = L.g.np + tid;
    long off[7];
    nb_offsets(L.g, off);
    const double a0 = (double)L.op.slot(0)[c], xc = x[c];
    double s = a0 * xc;
#pragma unroll
    for (int k = 1; k < 7; ++k) s += (double)L.op.slot(k)[c] * x[c + off[k]];
    const double upd = xc + (b[c] - s) / a0;
    out[c] = (((i0 + i1 + i2) & 1) == colour) ? upd : xc;
}

// the whole first forward sweep from the zero guess in one launch (the pattern of pre2_cell): red  x = b / a0;  black
// x = (b - sum_k a_k x_n) / a0  with the six red neighbours' x_n = b_n / a0_n recomputed from b and the neighbours' diagonals.
// A neighbour outside the box (its coefficient is zero) is read at the cell's own address, so that no quotient is formed from a
// halo plane's zero diagonal.
template <class R>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_gs_first(LevelDevT<R> L, const double *__restrict__ b, double *__restrict__ out) {
    const long tid = xcd_tid();
    if (tid >= L.g.nown) return;
    int i0, i1, i2;
    cell_ijk(L.g, tid, i0, i1, i2);
    const long c = L.g.np + tid;
    long off[7];
    nb_offsets(L.g, off);
    const bool in[7] = {true, i0 > 0, i0 + 1 < L.g.n0, i1 > 0, i1 + 1 < L.g.n1, i2 > 0, i2 + 1 < L.g.n2};
    const double a0 = (double)L.op.slot(0)[c], bc = b[c];
    double s = 0.0;
#pragma unroll
    for (int k = 1; k < 7; ++k) {
        const long n = in[k] ? c + off[k] : c;
        s += (double)L.op.slot(k)[c] * (b[n] / (double)L.op.slot(0)[n]);
    }
    out[c] = (((i0 + i1 + i2) & 1) ? bc - s : bc) / a0;
}

// ---- the tail: all small levels in one workgroup --------------------------------------------------------
// down-sweep, coarse solve and up-sweep of the levels [l0, nlev) by one workgroup of 1024 threads; `lv`: descriptors in LDS.
// Ends behind a workgroup barrier.
template <class R>
__device__ __forceinline__ void tail_sweeps(const LevelDevT<R> *lv, int l0, int nlev, int trunc, int ncoarse,
                                            const double *Minv, const double *b_top, double *e_top) {
    constexpr int T = 1024;            // (the launch's block size, as a constant: no blockDim fetch -- tp_common.hpp:xcd_tid)
    const int t = threadIdx.x;
    // down-sweep
    for (int l = l0; l < nlev - 1; ++l) {
        const LevelDevT<R> L = lv[l];
        const GridDev gc = lv[l + 1].g;
        const double *b = (l == l0) ? b_top : L.b;
        double *rc = lv[l + 1].b;
        if (L.pre == 0) {                      // V(0,post): x = 0, the residual is b itself
            for (long i = t; i < gc.nown; i += T) rc[gc.np + i] = restrict_cell(L, gc, b, i);
            __syncthreads();
            continue;
        }
        double *cur = L.x, *oth = L.x2;
        for (long i = t; i < L.g.nown; i += T)
            cur[L.g.np + i] = L.pre >= 2 ? pre2_cell<R, false>(L, b, i) : L.invd[L.g.np + i] * b[L.g.np + i];
        __syncthreads();
        for (int k = 2; k < L.pre; ++k) {
            for (long i = t; i < L.g.nown; i += T) oth[L.g.np + i] = jacobi_cell(L, b, cur, i);
            __syncthreads();
            double *tmp = cur; cur = oth; oth = tmp;
        }
        for (long i = t; i < gc.nown; i += T) rc[gc.np + i] = resid_restrict_cell(L, gc, b, cur, i);
        __syncthreads();
    }
    // coarsest grid: dense solve
    {
        const LevelDevT<R> Lc = lv[nlev - 1];
        const double *b = (nlev - 1 == l0) ? b_top : Lc.b;
        double *e = (nlev - 1 == l0) ? e_top : Lc.e;
        if (trunc >= 0) {                 // relaxation-only level: x = x1 + invd (b - A x1), x1 = invd b
            for (long i = t; i < Lc.g.nown; i += T) e[Lc.g.np + i] = pre2_cell<R, false>(Lc, b, i);
            __syncthreads();
        } else {
        // 16 lanes per row: coalesced reads of the row, 4 independent products per lane, shuffle reduction
        // (one lane per row walked its 64 entries one dependent L2 round trip at a time: ~30 us of a 44 us kernel)
        const int grp = t >> 4, gl = t & 15;
        for (int r = grp; r < ncoarse; r += T >> 4) {
            double s = 0.0;
            for (int q = gl; q < ncoarse; q += 16) s += Minv[(long)r * ncoarse + q] * b[Lc.g.np + q];
            s += __shfl_xor(s, 8, 64);
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 1, 64);
            if (gl == 0) e[Lc.g.np + r] = s;
        }
        __syncthreads();
        }
    }
    // up-sweep
    for (int l = nlev - 2; l >= l0; --l) {
        const LevelDevT<R> L = lv[l];
        const GridDev gc = lv[l + 1].g;
        const double *b = (l == l0) ? b_top : L.b;
        double *out = (l == l0) ? e_top : L.e;
        const double *ec = lv[l + 1].e;
        // where the pre-smoothed iterate lives: x after an even number of extra sweeps, else x2; none if pre == 0
        const int extra = L.pre >= 2 ? L.pre - 2 : 0;
        const double *src = L.pre == 0 ? nullptr : ((extra % 2 == 0) ? L.x : L.x2);
        if (L.post == 0) {                          // pure transfer level (amg_mid_skip): x = P ec
            for (long i = t; i < L.g.nown; i += T) {
                int i0, i1, i2;
                cell_ijk(L.g, i, i0, i1, i2);
                out[L.g.np + i] = prolong_val(L, gc, ec, i0, i1, i2);
            }
            __syncthreads();
            continue;
        }
        double *dst = (L.post == 1) ? out : (src == L.x ? L.x2 : L.x);
        for (long i = t; i < L.g.nown; i += T) dst[L.g.np + i] = prolong_jacobi_cell(L, gc, b, src, ec, i);
        __syncthreads();
        for (int k = 1; k < L.post; ++k) {
            src = dst;
            dst = (k == L.post - 1) ? out : (src == L.x ? L.x2 : L.x);
            for (long i = t; i < L.g.nown; i += T) dst[L.g.np + i] = jacobi_cell(L, b, src, i);
            __syncthreads();
        }
    }
}

// BUILD = false: one workgroup, e_top = (tail) b_top.
// BUILD = true: the batched launch that forms the dense tail operator (Amg::tdense).  Workgroup g takes the unit vectors
// e_j, j = g, g + gridDim.x, ... as right-hand sides -- generated here, in the level-l0 b vector the plain tail never
// uses -- and stores each result as COLUMN j of the row-major n x n matrix Tm (a scattered store once per set-up, so that
// k_amg_tail_dense reads rows coalesced).  Its level vectors are the workgroup's own: LDS, or a slice of `scratch`
// (4 x vec_doubles per workgroup, zero in the halo planes, which nothing ever writes) when they do not fit.
struct TailBuild {
    double *Tm = nullptr, *scratch = nullptr;
    int vec_doubles = 0;
};
template <class R, bool BUILD>
__global__ __launch_bounds__(1024) void k_amg_tail(const LevelDevT<R> *lv, int l0, int nlev_all, int trunc, int ncoarse,
                                                   const double *Minv, const double *b_top, double *e_top,
                                                   int lds_doubles, TailBuild tb) {
    // trunc >= l0: the hierarchy ends at level `trunc` with two damped-Jacobi sweeps instead of the dense solve
    const int nlev = trunc >= 0 ? trunc + 1 : nlev_all;
    extern __shared__ double dyn[];          // 4 x lds_doubles: the b, e, x, x2 vectors of every tail level
    constexpr int T = 1024;            // (the launch's block size, as a constant: no blockDim fetch -- tp_common.hpp:xcd_tid)
    const int t = threadIdx.x;
    // level descriptors live in LDS: every phase below starts with LDS reads, not a global round trip
    static_assert(sizeof(LevelDevT<R>) % sizeof(long) == 0, "LevelDev must be a whole number of words");
    __shared__ long slv_raw[40 * sizeof(LevelDevT<R>) / sizeof(long)];
    {
        const int wpl = (int)(sizeof(LevelDevT<R>) / sizeof(long));
        const long *src = reinterpret_cast<const long *>(lv);
        for (int i = l0 * wpl + t; i < nlev * wpl; i += T) slv_raw[i] = src[i];
        if (lds_doubles > 0)
            for (int i = t; i < 4 * lds_doubles; i += T) dyn[i] = 0.0;      // (halo planes must read as zero)
        __syncthreads();
    }
    if (lds_doubles > 0 || BUILD) {
        // the tail's vectors live in LDS: a phase boundary is then an LDS store + barrier + LDS load instead of a
        // global store that must drain (s_waitcnt vmcnt(0)) before the barrier and an L2 round trip after it.
        // Done by re-pointing the LDS copy of the level descriptors; the sweeps below do not change.
        // (BUILD without LDS: the same re-pointing, to this workgroup's slice of the scratch)
        if (t == 0) {
            LevelDevT<R> *w = reinterpret_cast<LevelDevT<R> *>(slv_raw);
            double *base = dyn;
            long vd = lds_doubles;
            if (BUILD && lds_doubles == 0) { vd = tb.vec_doubles; base = tb.scratch + (long)blockIdx.x * 4 * vd; }
            long off = 0;
            for (int l = l0; l < nlev; ++l) {
                w[l].b = base + off;
                w[l].e = base + vd + off;
                w[l].x = base + 2 * vd + off;
                w[l].x2 = base + 3 * vd + off;
                off += w[l].g.ntot;
            }
        }
        __syncthreads();
    }
    lv = reinterpret_cast<const LevelDevT<R> *>(slv_raw);
    // Touch every read-only array of the tail (operators, inverse diagonals, weights, the dense inverse) NOW, all
    // at once: they were written by the set-up long ago and have left the L2; otherwise each of the ~10 phases below
    // starts with its own HBM + TLB round trip (~3 us of a ~4 us phase).
    {
        double sink = 0.0;
        for (int l = l0; l < nlev; ++l) {
            const LevelDevT<R> &L = lv[l];
            for (long i = L.g.np + t; i < L.g.np + L.g.nown; i += T) {
#pragma unroll
                for (int k = 0; k < 7; ++k) sink += (double)L.op.slot(k)[i];
                sink += (double)L.invd[i];
                if (L.axis >= 0) sink += (double)L.wm[i] + (double)L.wp[i];
            }
        }
        if (trunc < 0)
            for (int i = t; i < ncoarse * ncoarse; i += T) sink += Minv[i];
        if (sink == 1.2345678e-300) (BUILD ? tb.Tm : e_top)[0] = sink;       // never true: keeps the loads alive
    }
    if constexpr (!BUILD) {
        tail_sweeps(lv, l0, nlev, trunc, ncoarse, Minv, b_top, e_top);
    } else {
        double *ub = lv[l0].b, *ue = lv[l0].e;
        const long np = lv[l0].g.np;
        const int n = (int)lv[l0].g.nown;
        for (int j = blockIdx.x; j < n; j += gridDim.x) {
            if (t == 0) ub[np + j] = 1.0;
            __syncthreads();
            tail_sweeps(lv, l0, nlev, trunc, ncoarse, Minv, ub, ue);
            for (int i = t; i < n; i += T) tb.Tm[(long)i * n + j] = ue[np + i];
            if (t == 0) ub[np + j] = 0.0;
            __syncthreads();
        }
    }
}

// e_top = T b_top, the tail as ONE dense mat-vec spread over the chip: one wavefront per row of the row-major n x n
// matrix (n <= 64 NK), each lane NK products in ascending column order, then a fixed butterfly -- no atomics, the same bits
// on every call.  Every load is issued up front (clamped address, selected value): the kernel is one memory round trip.
template <int NK>
__global__ __launch_bounds__(TP_BLOCK) void k_amg_tail_dense(const double *__restrict__ Tm, int n, long np,
                                                             const double *__restrict__ b, double *__restrict__ e) {
    const int row = (int)blockIdx.x * (TP_BLOCK / 64) + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const double *tr = Tm + (long)row * n;
    double tv[NK], bv[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int q = lane + 64 * k, qc = q < n ? q : 0;
        tv[k] = tr[qc];
        bv[k] = b[np + qc];
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NK; ++k) s += (lane + 64 * k < n) ? tv[k] * bv[k] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) e[np + row] = s;
}

// ---- host side ------------------------------------------------------------------------------------
std::vector<std::pair<int, int>> rank_slabs(const tp_ctx *c) {
    std::vector<std::pair<int, int>> slabs(c->dist ? c->grid.nranks : 0);
    for (size_t r = 0; r < slabs.size(); ++r) slab_of(c, (int)r, slabs[r].first, slabs[r].second);
    return slabs;
}

// Line relaxation (tp_options.amg_line_levels): the ONE place its layout rules live.  Lines per workgroup G of a level with
// lines of n0 cells: the LDS image of a workgroup, G lines at a stride of S = n0 | 1 doubles, stays within 48 KiB (three
// workgroups per CU beside each other, and below the 64 KiB a kernel may use without opting in); at most 64 (one lane per line:
// the substitution is one wavefront) and no more than the level has lines.  n0 = 85 (C4): 64 lines; n0 = 340 (config 5): 18.
static constexpr long LINE_LDS_BYTES = 48 * 1024;
static int line_stride(int n0) { return n0 | 1; }
static int line_group(const GridDev &g) {
    const long fit = LINE_LDS_BYTES / ((long)sizeof(double) * line_stride(g.n0));
    return (int)std::max(0L, std::min({64L, fit, (long)g.n1 * g.n2}));
}

void amg_line_check_options(const tp_options &o, int nranks) {
    const int L = o.amg_line_levels;
    TP_REQUIRE(L >= 0, "amg_line_levels must be >= 0");
    if (L == 0) return;
    TP_REQUIRE(L <= o.amg_full_levels, "amg_line_levels must not exceed amg_full_levels: line levels are V(nu,nu) levels, never pure-transfer or paired ones");
    TP_REQUIRE(!o.amg_single, "amg_line_levels (line relaxation) keeps its factor streams in fp64: not with amg_single");
    TP_REQUIRE(o.pc_kind != 3, "amg_line_levels (line relaxation) is implemented for the scalar hierarchies: not with pc_kind 3 (pc_cptramg, the system AMG)");
    TP_REQUIRE(o.schur_a11 != 2, "amg_line_levels (line relaxation) is not implemented for schur_a11 = 2 (schur_selfp)");
    TP_REQUIRE(nranks <= 1, "amg_line_levels (line relaxation) is implemented for one slab: not with nranks > 1");
}

// Red-black Gauss-Seidel (tp_options.amg_gs_levels / amg_gs_sweeps): ranges and what this implementation excludes.
void amg_gs_check_options(const tp_options &o, int nranks) {
    const int L = o.amg_gs_levels, g = o.amg_gs_sweeps;
    TP_REQUIRE(L >= 0, "amg_gs_levels must be >= 0");
    TP_REQUIRE(g >= 1 && g <= 4, "amg_gs_sweeps must be in 1..4");
    TP_REQUIRE(L > 0 || g == 1, "amg_gs_sweeps must be 1 while amg_gs_levels is 0: the sweep count would be ignored");
    if (L == 0) return;
    TP_REQUIRE(L <= o.amg_full_levels, "amg_gs_levels must not exceed amg_full_levels: Gauss-Seidel levels are V(g,g) levels, never pure-transfer or paired ones");
    TP_REQUIRE(o.amg_line_levels == 0, "amg_gs_levels (red-black Gauss-Seidel) and amg_line_levels (line relaxation) exclude one another: one smoother per level");
    TP_REQUIRE(!o.amg_single, "amg_gs_levels (red-black Gauss-Seidel) is implemented for fp64 operators: not with amg_single");
    TP_REQUIRE(o.pc_kind != 3, "amg_gs_levels (red-black Gauss-Seidel) is implemented for the scalar hierarchies: not with pc_kind 3 (pc_cptramg, the system AMG)");
    TP_REQUIRE(o.schur_a11 != 2, "amg_gs_levels (red-black Gauss-Seidel) is not implemented for schur_a11 = 2 (schur_selfp)");
    TP_REQUIRE(nranks <= 1, "amg_gs_levels (red-black Gauss-Seidel) is implemented for one slab: not with nranks > 1");
}

// g0: the grid the hierarchy coarsens -- the slab itself on one GPU, the GLOBAL grid on several.  There the top
// levels (more than gather_cells cells, at least two planes on every rank) stay distributed over the slabs
// and the rest of the hierarchy is built on the gathered global grid, replicated on every rank; a problem
// smaller than gather_cells is replicated from the top (dist_levels = 0: its V-cycle is launch-latency
// bound and would only get slower with a halo exchange between sweeps).
AmgPlan amg_plan(const GridDev &g0, const double strength[3], const tp_options &o, int me,
                 const std::vector<std::pair<int, int>> &slabs, long gather_cells, long tail_cells) {
    AmgPlan P;
    int m[3] = {g0.n0, g0.n1, g0.n2};
    {   // schedule: coarsen the axis of the strongest coupling, which halves its strength and doubles the others'
        int n[3] = {m[0], m[1], m[2]};
        double s[3];
        for (int a = 0; a < 3; ++a) s[a] = n[a] > 1 ? strength[a] : -1.0;
        while ((long)n[0] * n[1] * n[2] > std::max(1, o.amg_min_cells) && P.sched.size() < 40) {
            int best = -1;
            for (int a = 0; a < 3; ++a)
                if (n[a] > 1 && (best < 0 || s[a] > s[best])) best = a;
            if (best < 0) break;
            P.sched.push_back(best);
            n[best] = (n[best] + 1) / 2;
            for (int q = 0; q < 3; ++q) s[q] = (q == best) ? s[q] * 0.5 : s[q] * 2.0;
        }
    }
    std::vector<std::pair<int, int>> cur = slabs;          // owned global planes of every rank at the current level
    if (cur.empty()) cur = {{0, m[2]}};
    bool still = !slabs.empty() && gather_cells >= 0;
    const int nu = std::max(1, o.amg_nu);
    for (size_t l = 0; l <= P.sched.size(); ++l) {
        AmgPlan::Level L;
        if (still) {
            int minp = 1 << 30;
            for (auto &q : cur) minp = std::min(minp, q.second - q.first);
            still = (long)m[0] * m[1] * m[2] > gather_cells && minp >= 2 && l < P.sched.size();
            if (still) P.dist_levels = (int)l + 1;
        }
        P.ranges.push_back(cur);
        // a distributed level is this rank's slab of the level (live halo planes towards the neighbours);
        // every other level is the whole box with dead halo planes
        L.g = still ? make_grid(m[0], m[1], cur[me].second - cur[me].first, m[2], cur[me].first)
                    : make_grid(m[0], m[1], m[2], m[2], 0);
        // cycle shape: V(nu,nu) on the first levels, V(coarse_pre, coarse_post) below, and V(coarse_pre, tail_post) on
        // the levels of <= 1024 cells (a property of the level size, so that the oracle can mirror it)
        const bool full = (int)l < o.amg_full_levels;
        const bool small = L.g.np * (long)L.g.gn2 <= 1024;
        L.pre = full ? nu : std::max(0, o.amg_coarse_pre);
        L.post = full ? nu : std::max(1, small ? o.amg_tail_post : o.amg_coarse_post);
        // mid levels (neither full nor small): every second one is a pure transfer level -- the hierarchy then coarsens
        // two directions per smoothing level there, which costs no Krylov iterations (454 -> 456 on C4) and lets the
        // cycle fuse the two transfers
        if (o.amg_mid_skip && !full && !small && (((int)l - o.amg_full_levels) & 1)) { L.pre = 0; L.post = 0; }
        if (l < P.sched.size()) {
            L.axis = P.sched[l];
            m[L.axis] = (m[L.axis] + 1) / 2;
            if (L.axis == 2)
                for (auto &q : cur) q = {(q.first + 1) / 2, (q.second + 1) / 2};     // even global planes survive
        }
        P.lv.push_back(L);
    }
    P.tail_level = (int)P.lv.size() - 1;
    for (size_t l = (size_t)P.dist_levels; l < P.lv.size(); ++l)
        if (P.lv[l].g.nown <= tail_cells) { P.tail_level = (int)l; break; }
    // line levels: above the tail, among the first amg_line_levels levels (all of them V(nu,nu): amg_line_check_options), n0 >= 2
    for (int l = 0; l < std::min(o.amg_line_levels, P.tail_level); ++l)
        if (P.lv[l].g.n0 >= 2) {
            P.lv[l].line_g = line_group(P.lv[l].g);
            TP_REQUIRE(P.lv[l].line_g >= 1, "amg_line_levels: a line of this level does not fit the LDS budget of the line sweep");
        }
    // Gauss-Seidel levels: above the tail, among the first amg_gs_levels levels (all of them full levels: amg_gs_check_options);
    // such a level is V(g, g)
    for (int l = 0; l < std::min(o.amg_gs_levels, P.tail_level); ++l)
        P.lv[l].gs = P.lv[l].pre = P.lv[l].post = o.amg_gs_sweeps;
    return P;
}

static long line_groups(const AmgPlan::Level &P) { return ((long)P.g.n1 * P.g.n2 + P.line_g - 1) / P.line_g; }
static size_t line_stream_doubles(const AmgPlan::Level &P) { return (size_t)line_groups(P) * P.g.n0 * P.line_g; }
static LineDev line_of(const Amg *amg, int level) {
    const AmgPlan::Level &P = amg->plan.lv[level];
    const size_t n = line_stream_doubles(P);
    const double *f = amg->lv[level]->linef.p;
    return LineDev{f, f + n, f + 2 * n, P.line_g, line_stride(P.g.n0)};
}

void amg_line_info(const Amg *amg, int64_t out[4]) {
    out[0] = out[3] = 0;
    for (size_t l = 0; l < amg->lv.size(); ++l)
        if (amg->plan.lv[l].line_g > 0) { out[0]++; out[3] += (int64_t)amg->lv[l]->linef.n * (int64_t)sizeof(double); }
    out[1] = amg->plan.lv[0].line_g;
    out[2] = amg->plan.lv[0].g.n0;
}

void amg_gs_info(const Amg *amg, int64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (size_t l = 0; l < amg->lv.size(); ++l)
        if (amg->plan.lv[l].gs > 0) { out[0]++; out[1] = amg->plan.lv[l].gs; }
    if (amg->plan.lv[0].gs > 0) {          // even and odd index sums of a box differ by one cell exactly when every extent is odd
        const GridDev &g = amg->plan.lv[0].g;
        const int64_t n = (int64_t)g.n0 * g.n1 * g.n2;
        out[2] = (n + ((g.n0 & 1) && (g.n1 & 1) && (g.n2 & 1) ? 1 : 0)) / 2;
        out[3] = n - out[2];
    }
}

template <class R>
static LevelDevT<R> dev_of(const Amg *amg, int level) {
    const AmgLevel *L = amg->lv[level];
    LevelDevT<R> d;
    d.pre = amg->plan.lv[level].pre;
    d.post = amg->plan.lv[level].post;
    d.pad_ = 0;
    d.g = L->g;
    d.op.base = (R *)L->op.base;
    d.op.slot_stride = L->op.slot_stride;
    d.invd = (const R *)L->invd.p; d.wm = (const R *)L->wm.p; d.wp = (const R *)L->wp.p;
    d.b = L->b.p; d.x = L->x.p; d.x2 = L->x2.p; d.e = L->e.p;
    d.axis = L->axis;
    d.omega = amg->omega;
    return d;
}

void amg_build(tp_ctx *c, Amg *&amg, const GridDev &g0, const double strength[3], long gather_cells) {
    delete amg;
    amg = new Amg();
    c->graph_epoch++;            // a new hierarchy may reuse the old one's addresses: never replay graphs across a rebuild
    amg->single = c->opt.amg_single != 0;
    const long tail_cells = tp_switch_int(TP_SW_AMG_TAIL_CELLS);
    amg->plan = amg_plan(g0, strength, c->opt, c->dist ? c->grid.rank : 0, rank_slabs(c), gather_cells, tail_cells);
    for (const AmgPlan::Level &P : amg->plan.lv) {
        AmgLevel *L = new AmgLevel();
        L->g = P.g;
        L->axis = P.axis;
        amg->lv.push_back(L);
    }
    // carve every level's buffers out of one arena (32-double = 256-byte aligned slices)
    {
        auto pad = [](size_t v) { return (v + 31) & ~(size_t)31; };
        size_t total = 0;
        for (size_t l = 0; l < amg->lv.size(); ++l) {
            const size_t nt = pad((size_t)amg->lv[l]->g.ntot);
            total += ((l > 0 || amg->single) ? 7 : 0) * nt + 5 * nt + (amg->lv[l]->axis >= 0 ? 2 * nt : 0);
        }
        amg->arena.alloc(total);
        double *q = amg->arena.p;
        auto take = [&](DBuf<double> &d, size_t nd, size_t step) { d.view(q, nd); q += step; };
        for (size_t l = 0; l < amg->lv.size(); ++l) {
            AmgLevel *L = amg->lv[l];
            const size_t nt = (size_t)L->g.ntot, ntp = pad(nt);
            // operator/weight buffers are sized for doubles and hold floats when amg_single (slot stride in elements)
            if (l > 0 || amg->single) {
                take(L->A, 7 * nt, 7 * ntp);
                L->op.base = L->A.p;
                L->op.slot_stride = (long)nt;
            }
            take(L->invd, nt, ntp);
            take(L->b, nt, ntp); take(L->x, nt, ntp); take(L->x2, nt, ntp); take(L->e, nt, ntp);
            if (L->axis >= 0) { take(L->wm, nt, ntp); take(L->wp, nt, ntp); }
        }
    }
    // factor streams of the line levels: allocated here, once, and rewritten in place by every set-up (captured graphs keep them)
    for (size_t l = 0; l < amg->lv.size(); ++l) {
        const AmgPlan::Level &P = amg->plan.lv[l];
        if (P.line_g > 0) amg->lv[l]->linef.alloc(3 * line_stream_doubles(P));
    }
    amg->ncoarse = (int)amg->lv.back()->g.nown;
    TP_REQUIRE(amg->ncoarse <= 1024, "coarsest AMG grid too large for the dense solve");
    amg->ratio_dev.alloc(64 * 8);                       // 8 levels x 64 slots is more than amg_full_levels ever needs
    TP_HIP(hipHostMalloc((void **)&amg->ratio_host, 64 * 8 * sizeof(double)));
    TP_HIP(hipEventCreateWithFlags(&amg->ev_ratio, hipEventDisableTiming));
    amg->coarse_inv.alloc((size_t)2 * amg->ncoarse * amg->ncoarse);
    amg->fuse_below = tp_switch_int(TP_SW_AMG_FUSE_BELOW);
    amg->lvdev.alloc(amg->lv.size() * sizeof(LevelDevT<double>));
    // the tail keeps its vectors (b, e, x, x2 of every level) in LDS when they fit next to the level descriptors
    long tot = 0;
    for (size_t l = (size_t)amg->plan.tail_level; l < amg->lv.size(); ++l) tot += amg->lv[l]->g.ntot;
    const bool lds_on = tp_switch_flag(TP_SW_AMG_TAIL_LDS);
    amg->tail_lds = (lds_on && 4 * tot * (long)sizeof(double) <= 120 * 1024) ? (int)tot : 0;
    if (tp_switch_int(TP_SW_DEBUG) >= 1) fprintf(stderr, "[tp] amg tail: level %d of %zu, %ld doubles per vector set, lds %d\n", amg->plan.tail_level, amg->lv.size(), tot, amg->tail_lds);
    if (amg->tail_lds > 0) {
        const int bytes = 120 * 1024;      // per-function limit shared by every hierarchy: always the maximum
        const void *fns[4] = {reinterpret_cast<const void *>(&k_amg_tail<double, false>),
                              reinterpret_cast<const void *>(&k_amg_tail<float, false>),
                              reinterpret_cast<const void *>(&k_amg_tail<double, true>),
                              reinterpret_cast<const void *>(&k_amg_tail<float, true>)};
        for (const void *f : fns) TP_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    }
    // dense tail (Amg::tdense): worthwhile when the tail spans at least two levels, possible for n <= 1024 (k_amg_tail_dense).
    // Allocated here, once, and rewritten in place by every set-up: the captured pc_apply graphs keep its address.
    const long ntop = amg->lv[amg->plan.tail_level]->g.nown;
    amg->tail_vec = tot;
    amg->tdense_eligible = (int)amg->lv.size() - amg->plan.tail_level >= 2 && ntop <= 1024;
    if (amg->tdense_eligible) {
        amg->tdense.alloc((size_t)ntop * ntop);
        amg->tdense_groups = (int)ntop;
        if (amg->tail_lds == 0) {
            // level vectors in global memory: a slice per workgroup of a scratch of at most 32 MB (allocated by the first build,
            // so a hierarchy that never forms T never pays for it); each workgroup then builds several columns
            amg->tdense_groups = (int)std::max(1L, std::min(ntop, (32L << 20) / (4 * tot * (long)sizeof(double))));
        }
    }
}

// level-0 operator: double stencil view of the Jacobian -> storage type R
template <class R>
__global__ void k_amg_import(GridDev g, Stencil A0, R *out) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= g.nown) return;
    const long c = g.np + tid;
#pragma unroll
    for (int s = 0; s < 7; ++s) out[(long)s * g.ntot + c] = (R)A0.slot(s)[c];
}

// Form T for the operators of the last set-up: the tested tail kernel on every unit vector, one batched launch on the
// current stream (the AMG side stream of pc_setup, or the main stream from amg_resolve_trunc; never inside a capture).
// The ONE condition under which T has to be formed now: the cycles since the last set-up apply it, they reach the tail, and T
// does not yet carry that set-up's number.  shape_resolved: amg->trunc is a decision (false only in the first set-up of a
// hierarchy with truncation levels, whose dominance ratios are still on their way to the host).
static bool tail_dense_needed(const Amg *amg, bool shape_resolved) {
    return amg->tdense_on && shape_resolved && amg->trunc < 0 && amg->tdense_stamp != amg->setup_id;
}

static void tail_dense_build(tp_ctx *c, Amg *amg) {
    if (amg->tail_lds == 0 && !amg->tdense_scratch.p)      // (never inside a capture: set-up or amg_resolve_trunc)
        amg->tdense_scratch.alloc((size_t)amg->tdense_groups * 4 * amg->tail_vec);
    const int lt = amg->plan.tail_level, nlev = (int)amg->lv.size(), n = amg->ncoarse;
    TailBuild tb;
    tb.Tm = amg->tdense.p;
    tb.scratch = amg->tdense_scratch.p;
    tb.vec_doubles = (int)amg->tail_vec;
    const size_t lds = (size_t)4 * amg->tail_lds * sizeof(double);
    const double *Minv = amg->coarse_inv.p + (size_t)n * n;
    if (amg->single)
        hipLaunchKernelGGL((k_amg_tail<float, true>), dim3(amg->tdense_groups), dim3(1024), lds, c->stream,
                           (const LevelDevT<float> *)amg->lvdev.p, lt, nlev, -1, n, Minv, (const double *)nullptr,
                           (double *)nullptr, amg->tail_lds, tb);
    else
        hipLaunchKernelGGL((k_amg_tail<double, true>), dim3(amg->tdense_groups), dim3(1024), lds, c->stream,
                           (const LevelDevT<double> *)amg->lvdev.p, lt, nlev, -1, n, Minv, (const double *)nullptr,
                           (double *)nullptr, amg->tail_lds, tb);
    TP_HIP(hipGetLastError());
    amg->tdense_stamp = amg->setup_id;
    amg->tdense_builds++;
}

template <class R>
static void setup_impl(tp_ctx *c, Amg *amg, const Stencil &A0) {
    AmgLevel *L0 = amg->lv[0];
    const int lg = amg->plan.dist_levels;
    amg->omega = c->opt.amg_omega;      // what k_amg_weights below builds invd with (LevelDevT::omega)
    if (sizeof(R) == sizeof(double)) {
        L0->op = A0;                     // zero-copy view of the Jacobian planes
    } else {
        hipLaunchKernelGGL(k_amg_import<R>, grid_for(L0->g.nown), dim3(256), 0, c->stream, L0->g, A0, (R *)L0->A.p);
        L0->op.base = L0->A.p;
        L0->op.slot_stride = L0->g.ntot;
    }
    // relaxation-only truncation: dominance ratios of the V(nu,nu) levels (slab-distributed levels: maximum over the ranks)
    const int nratio = c->opt.amg_dom_tau > 0.0 ? std::min({c->opt.amg_full_levels, (int)amg->lv.size() - 1, 8}) : 0;
    if (nratio > 0) TP_HIP(hipMemsetAsync(amg->ratio_dev.p, 0, sizeof(double) * 64 * nratio, c->stream));
    for (size_t l = 0; l < amg->lv.size(); ++l) {
        AmgLevel *L = amg->lv[l];
        const StencilT<R> op{(R *)L->op.base, L->op.slot_stride};
        const bool want_ratio = (int)l < nratio;
        hipLaunchKernelGGL(k_amg_weights<R>, grid_for(L->g.nown, want_ratio ? 1024 : 256), dim3(want_ratio ? 1024 : 256), 0, c->stream, L->g, op, L->axis,
                           c->opt.amg_omega, (R *)L->wm.p, (R *)L->wp.p, (R *)L->invd.p,
                           (int)l < nratio ? (unsigned long long *)amg->ratio_dev.p + 64 * l : (unsigned long long *)nullptr);
        if constexpr (sizeof(R) == sizeof(double)) {
            if (amg->plan.lv[l].line_g > 0) {      // line level: Thomas factors of every line, in this hierarchy's stream chain
                const LineDev F = line_of(amg, (int)l);
                hipLaunchKernelGGL(k_amg_line_factor<R>, dim3((unsigned)line_groups(amg->plan.lv[l])), dim3(64), 0, c->stream, L->g, op,
                                   F.G, const_cast<double *>(F.m), const_cast<double *>(F.invd), const_cast<double *>(F.ap));
            }
        }
        if ((int)l < lg) {
            // distributed level: the cycle reads inverse diagonals and weights of the neighbours' boundary planes,
            // coarsening along the slab axis also their operator rows
            halo_exchange_raw(c, L->g, L->invd.p, 1, 0, sizeof(R));
            halo_exchange_raw(c, L->g, L->wm.p, 1, 0, sizeof(R));
            halo_exchange_raw(c, L->g, L->wp.p, 1, 0, sizeof(R));
            if (L->axis == 2) halo_exchange_raw(c, L->g, L->op.base, 7, (size_t)L->op.slot_stride * sizeof(R), sizeof(R));
        }
        if (L->axis >= 0) {
            AmgLevel *Lc = amg->lv[l + 1];
            const AmgPlan::View cv = amg->plan.coarse_view((int)l, c->grid.rank);
            hipLaunchKernelGGL(k_amg_coarsen<R>, grid_for(cv.g.nown), dim3(256), 0, c->stream, L->g, cv.g, op, L->axis,
                               (const R *)L->wm.p, (const R *)L->wp.p, (R *)Lc->A.p + cv.off, Lc->g.ntot);
            if ((int)l + 1 == lg)        // first replicated level: everybody gets everybody's rows
                gather_ranges(c, Lc->A.p, Lc->g.np, amg->plan.ranges[lg], 7, (size_t)Lc->g.ntot * sizeof(R), sizeof(R));
        }
    }
    AmgLevel *Lc = amg->lv.back();
    const int n = amg->ncoarse;
    const StencilT<R> opc{(R *)Lc->op.base, Lc->op.slot_stride};
    if (n <= 64) {
        const bool mfma = tp_switch_flag(TP_SW_AMG_DENSE_MFMA);  // (read per set-up: A/B in one process)
        if (mfma) {
            const int bytes = (64 * 128 + 4 * 128 + 64 * 4 + 16) * (int)sizeof(double);
            TP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_amg_dense_inverse_mfma<R>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            hipLaunchKernelGGL(k_amg_dense_inverse_mfma<R>, dim3(1), dim3(1024), bytes, c->stream, Lc->g, opc, n,
                               amg->coarse_inv.p + (size_t)n * n);
        } else {
            hipLaunchKernelGGL(k_amg_dense_inverse_lds<R>, dim3(1), dim3(1024), 0, c->stream, Lc->g, opc, n,
                               amg->coarse_inv.p + (size_t)n * n);
        }
    }
    else
        hipLaunchKernelGGL(k_amg_dense_inverse<R>, dim3(1), dim3(256), 0, c->stream, Lc->g, opc, n, amg->coarse_inv.p,
                           amg->coarse_inv.p + (size_t)n * n);
    std::vector<LevelDevT<R>> h;
    for (size_t l = 0; l < amg->lv.size(); ++l) h.push_back(dev_of<R>(amg, (int)l));
    amg->lvhost.assign((const char *)h.data(), (const char *)h.data() + h.size() * sizeof(LevelDevT<R>));
    TP_HIP(hipMemcpyAsync(amg->lvdev.p, amg->lvhost.data(), amg->lvhost.size(), hipMemcpyHostToDevice, c->stream));
    if (nratio > 0) {
        if (lg > 0) allreduce_max(c, amg->ratio_dev.p, 64 * nratio);      // every rank takes the same decision
        TP_HIP(hipMemcpyAsync(amg->ratio_host, amg->ratio_dev.p, sizeof(double) * 64 * nratio, hipMemcpyDeviceToHost, c->stream));
        TP_HIP(hipEventRecord(amg->ev_ratio, c->stream));
        amg->ratio_pending = true;
    } else if (amg->trunc != -1) {
        amg->trunc = -1;
        c->graph_epoch++;
    }
    // dense tail: used where it is exact -- relaxation-only truncation is decided among the first nratio levels, so with
    // tail_level >= nratio it ends the cycle above the tail or not at all.  T is formed now unless the last resolved cycle
    // shape never reached the tail, or, at the first set-up, no shape has been resolved yet (amg_resolve_trunc forms it
    // when the cycles turn out to need it).  (switch read per set-up: A/B in one process)
    amg->setup_id++;
    const bool dense_env = tp_switch_flag(TP_SW_AMG_TAIL_DENSE);
    const bool dense = dense_env && amg->tdense_eligible && amg->plan.tail_level >= nratio;
    if (dense != amg->tdense_on) {
        amg->tdense_on = dense;
        c->graph_epoch++;            // another kernel in the captured cycles
    }
    if (tail_dense_needed(amg, nratio == 0 || amg->setup_id > 1)) tail_dense_build(c, amg);
    TP_HIP(hipGetLastError());
}

// Called before the first cycle after a set-up (never inside a stream capture): waits for the ratios and fixes the
// truncation level.  Returns true when the cycle shape changed (captured pc_apply graphs are then stale).
bool amg_resolve_trunc(tp_ctx *c, Amg *amg) {
    if (!amg || !amg->ratio_pending) return false;
    TP_HIP(hipEventSynchronize(amg->ev_ratio));
    amg->ratio_pending = false;
    const int nratio = std::min({c->opt.amg_full_levels, (int)amg->lv.size() - 1, 8});
    int t = -1;
    for (int l = 0; l < nratio; ++l) {
        double r = 0.0;
        for (int q = 0; q < 64; ++q) r = std::max(r, amg->ratio_host[64 * l + q]);
        if (l == 0) amg->ratio0 = r;
        if (r <= c->opt.amg_dom_tau) { t = l; break; }
    }
    const bool changed = t != amg->trunc;
    amg->trunc = t;
    // the set-up skipped T because the previous cycles ended above the tail; these will not
    if (tail_dense_needed(amg, true)) tail_dense_build(c, amg);      // (on the main stream, in front of the first cycle)
    return changed;
}

void amg_setup(tp_ctx *c, Amg *amg, const Stencil &A0) {
    static_assert(sizeof(LevelDevT<float>) == sizeof(LevelDevT<double>), "descriptor size");
    if (amg->single) setup_impl<float>(c, amg, A0);
    else setup_impl<double>(c, amg, A0);
}

// Multi-GPU, levels [0, lg): the same kernels on this rank's slab of the level, with a halo exchange in front of
// every kernel that reads a neighbour's value across the slab boundary.  Levels >= lg: the gathered global
// grid, every rank computing the same thing.  (b's halo planes are overwritten by the exchange.)
template <class R>
static void vcycle_impl(tp_ctx *c, Amg *amg, const double *b, double *x) {
    const int nlev = (int)amg->lv.size(), lt = amg->plan.tail_level, lg = amg->plan.dist_levels;
    const int trunc = amg->trunc;               // >= 0: that level ends the cycle with two Jacobi sweeps (amg_dom_tau)
    const int ltop = (trunc >= 0 && trunc < lt) ? trunc : lt;      // big levels [0, ltop) run their normal down/up sweeps
    const dim3 bl(256);
    std::vector<double *> xs(nlev, nullptr);       // pre-smoothed iterate of each big level (null: none)
    // level l (smoothed, no pre-sweeps) + level l+1 (pure transfer): both transfers in one launch each way
    static const bool pair_on = tp_switch_flag(TP_SW_AMG_PAIR);
    // the sweeps' centre-cell omega / diag: recomputed in registers (invd_at), or TP_AMG_INVD_LOAD=1: read from the stored plane
    static const bool invd_reg = !tp_switch_flag(TP_SW_AMG_INVD_LOAD);
    // residual + restriction of the top levels in one tiled launch; TP_AMG_RR_FUSE=0: k_amg_resid, then k_amg_restrict
    static const bool rr_fuse = tp_switch_flag(TP_SW_AMG_RR_FUSE);
#define TP_AMG_REG_LAUNCH(KERNEL, ...)                                                                         \
    do {                                                                                                       \
        if (invd_reg) hipLaunchKernelGGL((KERNEL<R, true>), __VA_ARGS__);                                      \
        else hipLaunchKernelGGL((KERNEL<R, false>), __VA_ARGS__);                                              \
    } while (0)
    // correction + first post-sweep of the top levels in one tiled launch; TP_AMG_PJ_FUSE=0: k_amg_prolong_add, then k_amg_jacobi
    static const bool pj_fuse = tp_switch_flag(TP_SW_AMG_PJ_FUSE);
#define TP_AMG_PJ_LAUNCH(NH)                                                                                                           \
    do {                                                                                                                       \
        if (invd_reg) hipLaunchKernelGGL((k_amg_prolong_jacobi_tile<R, true, NH>), gt, dim3(TP_BLOCK), 0, c->stream, Ld, cv.g, nruns, ntiles, bl_, (const double *)src, ec, dst); \
        else hipLaunchKernelGGL((k_amg_prolong_jacobi_tile<R, false, NH>), gt, dim3(TP_BLOCK), 0, c->stream, Ld, cv.g, nruns, ntiles, bl_, (const double *)src, ec, dst); \
    } while (0)
    auto paired = [&](int l) {
        if (!pair_on || l < lg || l + 2 > lt || amg->lv[l]->g.nown >= amg->fuse_below) return false;
        if (trunc >= 0 && l + 2 > trunc) return false;          // (the truncation level is among the V(nu,nu) levels: never paired)
        const AmgPlan::Level &A = amg->plan.lv[l], &B = amg->plan.lv[l + 1];
        return A.pre == 0 && A.post >= 1 && B.pre == 0 && B.post == 0;
    };
    auto hx = [&](int l, const double *v) {        // halo exchange of a level-l vector (no-op below lg)
        if (l < lg) halo_exchange(c, amg->lv[l]->g, const_cast<double *>(v), 1, 0);
    };
    // line levels (amg_line_levels; one slab, fp64 operators: amg_line_check_options): every sweep is k_amg_line_sweep
    auto is_line = [&](int l) { return amg->plan.lv[l].line_g > 0; };
    auto line_sweep = [&](int l, const double *bb, const double *xin, double *xout) {      // xin == nullptr: from the zero guess
        if constexpr (sizeof(R) == sizeof(double)) {
            const AmgPlan::Level &P = amg->plan.lv[l];
            const LineDev F = line_of(amg, l);
            const dim3 gl((unsigned)line_groups(P));
            const size_t lds = (size_t)F.G * F.S * sizeof(double);
            if (xin) hipLaunchKernelGGL((k_amg_line_sweep<R, false>), gl, dim3(TP_BLOCK), lds, c->stream, dev_of<R>(amg, l), F, c->opt.amg_omega, bb, xin, xout);
            else hipLaunchKernelGGL((k_amg_line_sweep<R, true>), gl, dim3(TP_BLOCK), lds, c->stream, dev_of<R>(amg, l), F, c->opt.amg_omega, bb, xin, xout);
        } else {
            throw Error("line relaxation (amg_line_levels) with fp32 operators (amg_single)");
        }
    };
    // Gauss-Seidel levels (amg_gs_levels; one slab, fp64 operators: amg_gs_check_options): g forward sweeps (red, black) from the
    // zero guess on the way down, g backward sweeps (black, red) on the way up; the iterate ping-pongs between x and x2
    auto is_gs = [&](int l) { return amg->plan.lv[l].gs > 0; };
    auto gs_half = [&](int l, int colour, const double *bb, const double *xin, double *xout) {
        hipLaunchKernelGGL(k_amg_gs_half<R>, xcd_grid(amg->lv[l]->g.nown), bl, 0, c->stream, dev_of<R>(amg, l), colour, bb, xin, xout);
    };
    auto gs_forward = [&](int l, const double *bb) {        // F^g(0); returns the buffer that holds it
        AmgLevel *L = amg->lv[l];
        double *cur = L->x.p, *oth = L->x2.p;
        hipLaunchKernelGGL(k_amg_gs_first<R>, xcd_grid(L->g.nown), bl, 0, c->stream, dev_of<R>(amg, l), bb, cur);
        for (int h = 2; h < 2 * amg->plan.lv[l].gs; ++h) {
            gs_half(l, h & 1, bb, cur, oth);
            std::swap(cur, oth);
        }
        return cur;
    };
    auto gs_backward = [&](int l, const double *bb, double *src, double *out) {      // out = B^g(src)
        AmgLevel *L = amg->lv[l];
        const int nh = 2 * amg->plan.lv[l].gs;
        for (int h = 0; h < nh; ++h) {
            double *dst = (h == nh - 1) ? out : (src == L->x.p ? L->x2.p : L->x.p);
            gs_half(l, 1 - (h & 1), bb, src, dst);
            src = dst;
        }
    };
    // down-sweep over the big levels
    for (int l = 0; l < ltop; ++l) {
        AmgLevel *L = amg->lv[l];
        AmgLevel *Lc = amg->lv[l + 1];
        const LevelDevT<R> Ld = dev_of<R>(amg, l);
        const AmgPlan::View cv = amg->plan.coarse_view(l, c->grid.rank);
        const double *bl_ = (l == 0) ? b : L->b.p;
        double *bc = Lc->b.p + cv.off;
        const dim3 gr = xcd_grid(L->g.nown);
        const bool slab_axis = l < lg && L->axis == 2;      // the transfer itself crosses the slab boundary
        if (paired(l)) {
            AmgLevel *L2 = amg->lv[l + 2];
            hipLaunchKernelGGL(k_amg_restrict2<R>, xcd_grid(L2->g.nown), bl, 0, c->stream, Ld,
                               dev_of<R>(amg, l + 1), L2->g, bl_, L2->b.p);
            ++l;                                    // level l+1 has nothing else to do on the way down
            continue;
        }
        if (Ld.pre == 0) {                          // V(0,post): residual = b
            if (slab_axis) hx(l, bl_);
            hipLaunchKernelGGL(k_amg_restrict<R>, xcd_grid(cv.g.nown), bl, 0, c->stream, Ld, cv.g, bl_, bc);
        } else {
            double *cur = L->x.p, *oth = L->x2.p;
            if (is_gs(l)) {
                cur = gs_forward(l, bl_);
                oth = (cur == L->x.p) ? L->x2.p : L->x.p;
            } else if (is_line(l)) {                // the sweep from the zero guess, then plain line sweeps
                line_sweep(l, bl_, nullptr, cur);
                for (int k = 1; k < Ld.pre; ++k) {
                    line_sweep(l, bl_, cur, oth);
                    std::swap(cur, oth);
                }
            } else {
            if (Ld.pre >= 2) hx(l, bl_);            // the fused double sweep reads invd*b of the neighbours
            // (slab-distributed levels keep the stored plane: their halo diagonals are not exchanged)
            if (invd_reg && l >= lg) hipLaunchKernelGGL((k_amg_pre<R, true>), gr, bl, 0, c->stream, Ld, bl_, Ld.pre >= 2 ? 1 : 0, cur);
            else hipLaunchKernelGGL((k_amg_pre<R, false>), gr, bl, 0, c->stream, Ld, bl_, Ld.pre >= 2 ? 1 : 0, cur);
            for (int k = 2; k < Ld.pre; ++k) {
                hx(l, cur);
                TP_AMG_REG_LAUNCH(k_amg_jacobi, gr, bl, 0, c->stream, Ld, bl_, (const double *)cur, oth);
                std::swap(cur, oth);
            }
            }
            xs[l] = cur;
            hx(l, cur);
            if (rr_fuse && !slab_axis && L->g.nown >= amg->fuse_below) {
                // the residual goes to its coarse cells through LDS: one launch, no residual vector (k_amg_resid_restrict_tile)
                const RrTile T = rr_tile(L->g, cv.g, L->axis);
                const dim3 gt((T.ntiles + 7u) / 8u * 8u);
                if (L->axis == 0) hipLaunchKernelGGL((k_amg_resid_restrict_tile<R, true, 1>), gt, dim3(TP_BLOCK), 0, c->stream, Ld, cv.g, T, bl_, (const double *)cur, bc);
                else hipLaunchKernelGGL((k_amg_resid_restrict_tile<R, false, RR_K>), gt, dim3(TP_BLOCK), 0, c->stream, Ld, cv.g, T, bl_, (const double *)cur, bc);
            } else if (slab_axis || L->g.nown >= amg->fuse_below) {
                hipLaunchKernelGGL(k_amg_resid<R>, gr, bl, 0, c->stream, Ld, bl_, (const double *)cur, oth);
                if (slab_axis) hx(l, oth);
                hipLaunchKernelGGL(k_amg_restrict<R>, xcd_grid(cv.g.nown), bl, 0, c->stream, Ld, cv.g, (const double *)oth, bc);
            } else {
                hipLaunchKernelGGL(k_amg_resid_restrict<R>, xcd_grid(cv.g.nown), bl, 0, c->stream, Ld, cv.g, bl_,
                                   (const double *)cur, bc);
            }
        }
        if (l + 1 == lg)        // restricted residual of every slab -> the replicated levels' right-hand side
            gather_ranges(c, Lc->b.p, Lc->g.np, amg->plan.ranges[lg], 1, 0, sizeof(double));
    }
    if (trunc >= 0 && trunc < lt) {
        // relaxation-only big level: x = x1 + invd (b - A x1), x1 = invd b (the fused double sweep), nothing below it
        AmgLevel *L = amg->lv[trunc];
        const double *bt = (trunc == 0) ? b : L->b.p;
        double *et = (trunc == 0) ? x : L->e.p;
        if (is_gs(trunc)) {                         // B^g F^g 0
            gs_backward(trunc, bt, gs_forward(trunc, bt), et);
        } else if (is_line(trunc)) {                // its two sweeps as line sweeps
            line_sweep(trunc, bt, nullptr, L->x.p);
            line_sweep(trunc, bt, L->x.p, et);
        } else {
        hx(trunc, bt);                              // the fused double sweep reads invd*b of the neighbours
        if (invd_reg && trunc >= lg) hipLaunchKernelGGL((k_amg_pre<R, true>), xcd_grid(L->g.nown), bl, 0, c->stream, dev_of<R>(amg, trunc), bt, 1, et);
        else hipLaunchKernelGGL((k_amg_pre<R, false>), xcd_grid(L->g.nown), bl, 0, c->stream, dev_of<R>(amg, trunc), bt, 1, et);
        }
    } else {
        // the tail: every level from lt down to the coarsest (or the truncation level) and back, one launch
        AmgLevel *Lt = amg->lv[lt];
        const double *bt = (lt == 0) ? b : Lt->b.p;
        double *et = (lt == 0) ? x : Lt->e.p;
        const int n = amg->ncoarse;
        if (amg->tdense_on) {
            // a stale operator is impossible, not unlikely: T carries the number of the set-up it was formed for
            TP_REQUIRE(trunc < 0 && amg->tdense_stamp == amg->setup_id, "the dense AMG tail was not formed for the last set-up");
            const int nt = (int)Lt->g.nown;
            const dim3 gd((unsigned)((nt + TP_BLOCK / 64 - 1) / (TP_BLOCK / 64))), bd(TP_BLOCK);
            const double *Tm = amg->tdense.p;
            if (nt <= 256) hipLaunchKernelGGL(k_amg_tail_dense<4>, gd, bd, 0, c->stream, Tm, nt, Lt->g.np, bt, et);
            else if (nt <= 512) hipLaunchKernelGGL(k_amg_tail_dense<8>, gd, bd, 0, c->stream, Tm, nt, Lt->g.np, bt, et);
            else if (nt <= 768) hipLaunchKernelGGL(k_amg_tail_dense<12>, gd, bd, 0, c->stream, Tm, nt, Lt->g.np, bt, et);
            else hipLaunchKernelGGL(k_amg_tail_dense<16>, gd, bd, 0, c->stream, Tm, nt, Lt->g.np, bt, et);
            amg->tdense_applies++;
        } else {
            hipLaunchKernelGGL((k_amg_tail<R, false>), dim3(1), dim3(1024), (size_t)4 * amg->tail_lds * sizeof(double), c->stream,
                               (const LevelDevT<R> *)amg->lvdev.p, lt, nlev, trunc, n,
                               (const double *)(amg->coarse_inv.p + (size_t)n * n), bt, et, amg->tail_lds, TailBuild());
            amg->tail_launches++;
        }
    }
    // up-sweep over the big levels
    for (int l = ltop - 1; l >= 0; --l) {
        AmgLevel *L = amg->lv[l];
        AmgLevel *Lc = amg->lv[l + 1];
        const LevelDevT<R> Ld = dev_of<R>(amg, l);
        const AmgPlan::View cv = amg->plan.coarse_view(l, c->grid.rank);
        const double *bl_ = (l == 0) ? b : L->b.p;
        double *out = (l == 0) ? x : L->e.p;
        const double *ec = Lc->e.p + cv.off;
        const dim3 gr = xcd_grid(L->g.nown);
        double *src = xs[l];                        // its halo is still the one exchanged before the residual; the tiled launch
                                                    // only reads it, the two launches add P ec to it in place
        double *dst = (Ld.post == 1) ? out : (src == L->x.p ? L->x2.p : L->x.p);
        if (l >= 1 && paired(l - 1)) continue;      // transfer-only level folded into its parent's launch
        if (paired(l)) {
            AmgLevel *L2 = amg->lv[l + 2];
            TP_AMG_REG_LAUNCH(k_amg_prolong2_jacobi, gr, bl, 0, c->stream, Ld, dev_of<R>(amg, l + 1), L2->g, bl_,
                               (const double *)L2->e.p, dst);
            for (int k = 1; k < Ld.post; ++k) {
                src = dst;
                dst = (k == Ld.post - 1) ? out : (src == L->x.p ? L->x2.p : L->x.p);
                TP_AMG_REG_LAUNCH(k_amg_jacobi, gr, bl, 0, c->stream, Ld, bl_, (const double *)src, dst);
            }
            continue;
        }
        hx(l + 1, Lc->e.p);                         // distributed coarse level: parents across the boundary
        if (Ld.post == 0) {                         // pure transfer level
            hipLaunchKernelGGL(k_amg_prolong_set<R>, gr, bl, 0, c->stream, Ld, cv.g, ec, out);
            continue;
        }
        if (is_gs(l)) {                             // the unfused sequence whatever fuse_below says: x += P ec, then the half-sweeps
            TP_REQUIRE(src, "a Gauss-Seidel level has pre-smoothing sweeps");
            hipLaunchKernelGGL(k_amg_prolong_add<R>, gr, bl, 0, c->stream, Ld, cv.g, ec, src);
            gs_backward(l, bl_, src, out);
            continue;
        }
        if (is_line(l)) {                           // the unfused sequence whatever fuse_below says: x += P ec, then line sweeps
            TP_REQUIRE(src, "a line level has pre-smoothing sweeps");
            hipLaunchKernelGGL(k_amg_prolong_add<R>, gr, bl, 0, c->stream, Ld, cv.g, ec, src);
            line_sweep(l, bl_, src, dst);
            for (int k = 1; k < Ld.post; ++k) {
                src = dst;
                dst = (k == Ld.post - 1) ? out : (src == L->x.p ? L->x2.p : L->x.p);
                line_sweep(l, bl_, src, dst);
            }
            continue;
        }
        if (pj_fuse && l >= lg && src && L->g.nown >= amg->fuse_below && 2 * L->g.n0 <= PJ_NH_MAX * TP_BLOCK) {
            // x' = src + P ec stays in LDS and registers: one launch, xs[l] is only read (k_amg_prolong_jacobi_tile)
            const unsigned nruns = (unsigned)((L->g.np + TP_BLOCK - 1) / TP_BLOCK), ntiles = nruns * (unsigned)L->g.n2;
            const dim3 gt((ntiles + 7u) / 8u * 8u);
            if (2 * L->g.n0 <= TP_BLOCK) TP_AMG_PJ_LAUNCH(1);
            else TP_AMG_PJ_LAUNCH(PJ_NH_MAX);
        } else if (src && L->g.nown >= amg->fuse_below) {
            hipLaunchKernelGGL(k_amg_prolong_add<R>, gr, bl, 0, c->stream, Ld, cv.g, ec, src);
            hx(l, src);
            TP_AMG_REG_LAUNCH(k_amg_jacobi, gr, bl, 0, c->stream, Ld, bl_, (const double *)src, dst);
        } else {
            TP_AMG_REG_LAUNCH(k_amg_prolong_jacobi, gr, bl, 0, c->stream, Ld, cv.g, bl_, (const double *)src, ec, dst);
        }
        for (int k = 1; k < Ld.post; ++k) {
            src = dst;
            dst = (k == Ld.post - 1) ? out : (src == L->x.p ? L->x2.p : L->x.p);
            hx(l, src);
            TP_AMG_REG_LAUNCH(k_amg_jacobi, gr, bl, 0, c->stream, Ld, bl_, (const double *)src, dst);
        }
    }
#undef TP_AMG_PJ_LAUNCH
#undef TP_AMG_REG_LAUNCH
    TP_HIP(hipGetLastError());
}

void amg_vcycle(tp_ctx *c, Amg *amg, const double *b, double *x) {
    TP_REQUIRE(amg && !amg->lv.empty(), "AMG not set up");
    TP_REQUIRE(!amg->ratio_pending, "amg_resolve_trunc must run after a set-up and before the first cycle");
    TP_REQUIRE(x != amg->lv[0]->x.p && x != amg->lv[0]->x2.p && b != x, "aliasing in amg_vcycle");
    if (amg->single) vcycle_impl<float>(c, amg, b, x);
    else vcycle_impl<double>(c, amg, b, x);
}

}  // namespace tp
