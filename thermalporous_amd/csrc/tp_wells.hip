// Completed wells (tp_set_wells): many perforated cells, ONE bottom-hole pressure, a total-rate target with a BHP
// limit, the hydrostatic head between the perforations.  The well's one unknown, its BHP, is eliminated exactly in the assembly:
// what remains is the 7-point Jacobian plus one rank-1 term c_w b_w^T per rate-controlled well, which only the Krylov operator
// applies (k_well_apply behind the block SpMV); the preconditioner goes on seeing the 7-point matrix.
//
// With u_k = (p_k, T_k[, S_k]) the state of the perforated cell c_k:
//   a_k     = WI_k lambda_k(u_k)              lambda: the factor source_eval multiplies the drawdown by (tp_assembly.hip)
//   theta_k = p_k - rho_w g (z_ref - z_k)     rho_w: frozen over a time step (k_well_rho, from the old state)
//   q_k     = -a_k (theta_k - bhp)            on open perforations (producer: theta_k > bhp, injector: theta_k < bhp), else 0
//   rate mode: bhp solves sum_k q_k = -+Q by active-set rounds; BHP mode (limit violated, or no mobile perforation): bhp = limit
// A perforation adds what a tp_source entry of its kind adds for the rate q_k with wt = 1 (the cell's own normalised delta):
// G(u_k) q_k, linear in the rate.  Every kernel here runs ONE WAVEFRONT PER WELL, lanes striding over the perforations; sums go
// through a fixed per-lane order and a fixed xor butterfly, so results do not depend on anything but the inputs.
#include "tp_common.hpp"
#include "tp_closures.hpp"
#include <algorithm>
#include <cmath>
#include <map>

namespace tp {

struct WellArgs {
    GridDev g;
    DevPrm q;
    const WellDev *wd;
    const long *cell;
    const double *WI, *dz, *rho;
    double *pa, *pth;             // per-perforation scratch: a_k and theta_k of this assembly
    const double *u;
    double *R, *J, *Sm;           // J, Sm null: the residual-only form of the line search's trial assemblies
    double *fc, *fb, *pq, *info;
    int *r1;
    int np;                       // perforations of all wells (stride of the per-perforation planes)
    double grav;                  // prm.g on a grid with a gravity axis, else 0
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);       // every lane ends with the same bits
    return v;
}

// lambda, and G with out = G * rate as source_eval forms it for wt = 1 (gs: schur_diag per unit rate; fw, fo: the phase split)
template <int NPH, bool SATFN>
__device__ __forceinline__ void well_eval(int kind, const DevPrm &q, const Dual3 &p, const Dual3 &T, const Dual3 &S, const DevSat *sat,
                                          Dual3 &lam, Dual3 *G, double &gs, double &fw, double &fo) {
    constexpr int B = NPH + 1;
    for (int r = 0; r < B; ++r) G[r] = Dual3(0.0);
    gs = 0.0; fw = 0.0; fo = 0.0;
    const Dual3 mo = oil_mu_t(T, q);
    if (NPH == 1) {
        lam = Dual3(1.0) / mo;
        fo = 1.0;
        if (kind == 0) {
            const Dual3 ro = oil_rho_t(p, T, q);
            G[0] = ro * q.w0;
            G[1] = ro * T * q.c_v_o;
            gs = ro.v * q.c_v_o;
        } else {
            const Dual3 roi = oil_rho_t(p, Dual3(q.T_inj), q);
            G[0] = roi * q.w0;
            G[1] = roi * (q.c_v_o * q.T_inj);
        }
        return;
    }
    const Dual3 mw = water_mu_t(T);
    if (kind == 0) {
        Dual3 lam_o, lam_w;
        if constexpr (SATFN) { lam_o = kr_o_t(S, *sat) / mo; lam_w = kr_w_t(S, *sat) / mw; }
        else { lam_o = S / mo; lam_w = (Dual3(1.0) - S) / mw; }
        lam = lam_o + lam_w;
        if (!(lam.v > 0.0)) { lam = Dual3(0.0); return; }           // both phases immobile: the perforation carries nothing
        const Dual3 ro = oil_rho_t(p, T, q), rw = water_rho_t(p, T);
        const Dual3 gw = lam_w / lam, go = lam_o / lam;
        fw = gw.v; fo = go.v;
        const Dual3 m = rw * gw * q.c_v_w + ro * go * q.c_v_o;
        G[0] = m * q.w0;
        G[1] = m * T;
        G[2] = ro * go * q.w2;
        gs = m.v;
    } else {
        lam = Dual3(1.0) / mw;
        fw = 1.0;
        const Dual3 rwi = water_rho_t(p, Dual3(q.T_inj));
        G[0] = rwi * (q.w0 * q.c_v_w);
        G[1] = rwi * (q.c_v_w * q.T_inj);
    }
}

// info per well, 8 doubles: bhp, mode (0 shut, 1 rate, 2 BHP), total, water, oil rate, rho_w, active-set rounds, open perforations
constexpr int WINFO = 8;

template <int NPH, bool SATFN>
__device__ __forceinline__ void wells_body(const WellArgs &a, const DevSat *sat) {
    constexpr int B = NPH + 1;
    const int w = blockIdx.x, lane = threadIdx.x;
    const WellDev wd = a.wd[w];
    const long nt = a.g.ntot;
    const int k0 = wd.first, k1 = wd.first + wd.count, np = a.np;
    const double rho = a.rho[w];
    const bool jac = a.J != nullptr;
    if (wd.shut || !(wd.rate > 0.0)) {                              // contributes nothing
        for (int k = k0 + lane; k < k1; k += 64) {
            a.pq[k] = 0.0; a.pq[np + k] = 0.0; a.pq[2 * np + k] = 0.0;
            if (jac)
                for (int r = 0; r < B; ++r) { a.fc[r * np + k] = 0.0; a.fb[r * np + k] = 0.0; }
        }
        if (lane == 0) {
            double *o = a.info + (long)w * WINFO;
            o[0] = wd.limit; o[1] = 0.0; o[2] = o[3] = o[4] = 0.0; o[5] = rho; o[6] = 0.0; o[7] = 0.0;
            if (jac) a.r1[w] = 0;
        }
        return;
    }
    const double sgn = wd.kind == 0 ? 1.0 : -1.0;                  // open: sgn (theta - bhp) > 0
    // Thresholds and the bhp are carried RELATIVE to the first perforation's threshold th0: pressures of ~40 MPa whose differences,
    // the drawdowns, may be a thousandth of that -- the sums below then lose digits of the drawdown, not of the pressure.
    const double th0 = a.u[a.cell[k0]] - rho * a.grav * a.dz[k0];
    // ---- pass 1: a_k and theta_k ------------------------------------------------------------------------------------------
    for (int k = k0 + lane; k < k1; k += 64) {
        const long c = a.cell[k];
        const Dual3 p(a.u[c], 0), T(a.u[nt + c], 1), S(NPH == 2 ? a.u[2 * nt + c] : 0.0, 2);
        Dual3 lam, G[B];
        double gs, fw, fo;
        well_eval<NPH, SATFN>(wd.kind, a.q, p, T, S, sat, lam, G, gs, fw, fo);
        a.pa[k] = a.WI[k] * lam.v;
        a.pth[k] = (p.v - rho * a.grav * a.dz[k]) - th0;
    }
    // ---- active-set rounds: all open, bhp from the open ones, close what that bhp shuts, until nothing changes.  The threshold
    // only moves one way (kept so by the running extreme `lim`), so the open sets are nested: at most count rounds.
    double lim = -sgn * INFINITY, bhp = wd.limit - th0, sa = 0.0;        // (bhp, lim: relative to th0 like the thresholds)
    int rounds = 0, nopen_prev = -1;
    bool rate_mode = false;
    for (int it = 0; it <= wd.count; ++it) {
        double s_a = 0.0, s_at = 0.0, s_n = 0.0;
        for (int k = k0 + lane; k < k1; k += 64) {
            const double ak = a.pa[k], th = a.pth[k];
            if (sgn * (th - lim) > 0.0) { s_a += ak; s_at += ak * th; s_n += 1.0; }
        }
        s_a = wave_sum(s_a); s_at = wave_sum(s_at); s_n = wave_sum(s_n);
        const int nopen = (int)s_n;
        if (nopen == nopen_prev) break;                             // the last bhp shut nothing: it stands
        nopen_prev = nopen;
        ++rounds;
        sa = s_a;
        if (!(s_a > 0.0)) { rate_mode = false; break; }            // nothing mobile is open: BHP mode
        bhp = (s_at - sgn * wd.rate) / s_a;
        rate_mode = true;
        lim = sgn > 0.0 ? fmax(lim, bhp) : fmin(lim, bhp);
    }
    if (rate_mode && (wd.kind == 0 ? th0 + bhp < wd.limit : th0 + bhp > wd.limit)) rate_mode = false;
    if (!rate_mode) { bhp = wd.limit - th0; lim = bhp; }
    const bool fold = wd.count == 1;                                // one perforation: c b^T is a diagonal block, folded into J
    // ---- pass 2: contributions, factors, rates ----------------------------------------------------------------------------
    double tq = 0.0, tw = 0.0, to = 0.0, tn = 0.0;
    for (int k = k0 + lane; k < k1; k += 64) {
        const long c = a.cell[k];
        const Dual3 p(a.u[c], 0), T(a.u[nt + c], 1), S(NPH == 2 ? a.u[2 * nt + c] : 0.0, 2);
        Dual3 lam, G[B];
        double gs, fw, fo;
        well_eval<NPH, SATFN>(wd.kind, a.q, p, T, S, sat, lam, G, gs, fw, fo);
        const Dual3 ak = lam * a.WI[k];
        const Dual3 th = (p - Dual3(rho * a.grav * a.dz[k])) - Dual3(th0);
        const bool open = sgn * (th.v - lim) > 0.0;
        Dual3 qk(0.0);
        if (open) qk = (Dual3(bhp) - th) * ak;
        // one perforation in rate mode carries the whole target whatever its state: q = -+Q, a constant (its c b^T, a diagonal
        // block, cancels dq/du at fixed bhp exactly)
        if (open && rate_mode && fold) qk = Dual3(-sgn * wd.rate);
        double cf[B], bf[B];
        for (int r = 0; r < B; ++r) { cf[r] = 0.0; bf[r] = 0.0; }
        if (open && rate_mode && !fold) {
            for (int r = 0; r < B; ++r) {
                cf[r] = -G[r].v * ak.v;
                bf[r] = (ak.d[r] * (th.v - bhp) + (r == 0 ? ak.v : 0.0)) / sa;
            }
        }
        for (int r = 0; r < B; ++r) {
            const Dual3 out = G[r] * qk;
            a.R[(long)r * nt + c] -= out.v;
            if (jac)
                for (int k2 = 0; k2 < B; ++k2) a.J[((long)r * B + k2) * nt + c] -= out.d[k2];
        }
        if (a.Sm) a.Sm[c] -= gs * qk.v;
        if (jac)
            for (int r = 0; r < B; ++r) { a.fc[r * np + k] = cf[r]; a.fb[r * np + k] = bf[r]; }
        a.pq[k] = qk.v; a.pq[np + k] = fw * qk.v; a.pq[2 * np + k] = fo * qk.v;
        tq += qk.v; tw += fw * qk.v; to += fo * qk.v; tn += open ? 1.0 : 0.0;
    }
    tq = wave_sum(tq); tw = wave_sum(tw); to = wave_sum(to); tn = wave_sum(tn);
    if (lane == 0) {
        double *o = a.info + (long)w * WINFO;
        o[0] = rate_mode ? th0 + bhp : wd.limit; o[1] = rate_mode ? 1.0 : 2.0; o[2] = tq; o[3] = tw; o[4] = to; o[5] = rho; o[6] = (double)rounds; o[7] = tn;
        if (jac) a.r1[w] = (rate_mode && !fold) ? 1 : 0;
    }
}
template <int NPH>
__global__ __launch_bounds__(64) void k_wells(WellArgs a) { wells_body<NPH, false>(a, nullptr); }
__global__ __launch_bounds__(64) void k_wells_sat(WellArgs a, DevSat sat) { wells_body<2, true>(a, &sat); }

// rho_w of every well from the old state: producers the mobility-weighted mixture over all perforations, injectors the injected
// fluid at (p_old of the datum perforation, T_inj).  No mobile perforation: 0 (no head).
template <int NPH, bool SATFN>
__device__ __forceinline__ void well_rho_body(GridDev g, DevPrm q, const WellDev *wds, const long *cell, const double *WI,
                                              const double *u, double *rho, const DevSat *sat) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const WellDev wd = wds[w];
    const long nt = g.ntot;
    if (wd.kind == 1) {
        if (lane == 0) {
            const double p = u[cell[wd.datum]];
            double r, rp, rT;
            if (NPH == 2) water_rho(p, q.T_inj, r, rp, rT);
            else oil_rho(p, q.T_inj, q, r, rp, rT);
            rho[w] = r;
        }
        return;
    }
    double num = 0.0, den = 0.0;
    for (int k = wd.first + lane; k < wd.first + wd.count; k += 64) {
        const long c = cell[k];
        const double p = u[c], T = u[nt + c];
        double ro, ro_p, ro_T, mo, mo_T;
        oil_rho(p, T, q, ro, ro_p, ro_T);
        oil_mu(T, q, mo, mo_T);
        if (NPH == 1) {
            num += WI[k] * ro / mo;
            den += WI[k] / mo;
        } else {
            const double S = u[2 * nt + c];
            double rw, rw_p, rw_T, mw, mw_T;
            water_rho(p, T, rw, rw_p, rw_T);
            water_mu(T, mw, mw_T);
            double kro = S, krw = 1.0 - S;
            if constexpr (SATFN) { kro = kr_o_t(Dual1{S, 1.0}, *sat).v; krw = kr_w_t(Dual1{S, 1.0}, *sat).v; }
            const double lo = kro / mo, lw = krw / mw;
            num += WI[k] * (lo * ro + lw * rw);
            den += WI[k] * (lo + lw);
        }
    }
    num = wave_sum(num); den = wave_sum(den);
    if (lane == 0) rho[w] = den > 0.0 ? num / den : 0.0;
}
template <int NPH>
__global__ __launch_bounds__(64) void k_well_rho(GridDev g, DevPrm q, const WellDev *wd, const long *cell, const double *WI,
                                                 const double *u, double *rho) {
    well_rho_body<NPH, false>(g, q, wd, cell, WI, u, rho, nullptr);
}
__global__ __launch_bounds__(64) void k_well_rho_sat(GridDev g, DevPrm q, const WellDev *wd, const long *cell, const double *WI,
                                                     const double *u, double *rho, DevSat sat) {
    well_rho_body<2, true>(g, q, wd, cell, WI, u, rho, &sat);
}

// the rank-1 terms of the Krylov operator: s_w = b_w . x over the well's cells, then y[c_k] += c_k s_w (MODE 0) or
// r[c_k] -= c_k s_w (MODE 1).  One launch for all wells, one wavefront per well; wells without a term (BHP mode, shut, one
// perforation) return on their flag.  No two wells share a cell, so the updates need no atomics.
template <int B, int MODE>
__global__ __launch_bounds__(64) void k_well_apply(long nt, const WellDev *wds, const int *r1, const long *cell, const double *fc,
                                                   const double *fb, int np, const double *__restrict__ x, double *y) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (!r1[w]) return;
    const WellDev wd = wds[w];
    const int k0 = wd.first, k1 = wd.first + wd.count;
    double s = 0.0;
    for (int k = k0 + lane; k < k1; k += 64) {
        const long c = cell[k];
#pragma unroll
        for (int r = 0; r < B; ++r) s += fb[r * np + k] * x[(long)r * nt + c];
    }
    s = wave_sum(s);
    if (MODE) s = -s;
    for (int k = k0 + lane; k < k1; k += 64) {
        const long c = cell[k];
#pragma unroll
        for (int r = 0; r < B; ++r) y[(long)r * nt + c] += fc[r * np + k] * s;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static void wells_upload_control(tp_ctx *c) {
    Wells &W = c->wells;
    std::vector<WellDev> wd(W.nw);
    for (int w = 0; w < W.nw; ++w) {
        const tp_well &t = W.wells[w];
        WellDev &d = wd[w];
        d.kind = t.kind; d.shut = t.shut; d.first = t.first; d.count = t.count; d.rate = t.rate; d.limit = t.bhp_limit;
        // the datum perforation: the one whose elevation lies nearest to z_ref (the first of equals)
        d.datum = t.first;
        for (int k = t.first; k < t.first + t.count; ++k)
            if (std::fabs(W.perfs[k].z - t.z_ref) < std::fabs(W.perfs[d.datum].z - t.z_ref)) d.datum = k;
    }
    copy_sync(c, W.wd.p, wd.data(), sizeof(WellDev) * W.nw, hipMemcpyHostToDevice);
}

void wells_rho(tp_ctx *c) {
    Wells &W = c->wells;
    if (W.nw == 0) return;
    const dim3 gr(W.nw), bl(64);
    if (c->satfn)
        hipLaunchKernelGGL(k_well_rho_sat, gr, bl, 0, c->stream, c->g, c->dprm, W.wd.p, W.cell.p, W.WI.p, c->u_old.p, W.rho.p, c->dsat);
    else if (c->nph == 2)
        hipLaunchKernelGGL(k_well_rho<2>, gr, bl, 0, c->stream, c->g, c->dprm, W.wd.p, W.cell.p, W.WI.p, c->u_old.p, W.rho.p);
    else
        hipLaunchKernelGGL(k_well_rho<1>, gr, bl, 0, c->stream, c->g, c->dprm, W.wd.p, W.cell.p, W.WI.p, c->u_old.p, W.rho.p);
    TP_HIP(hipGetLastError());
}

void wells_set(tp_ctx *c, int nw, const tp_well *wells, int np, const tp_perf *perfs) {
    TP_REQUIRE(c, "null argument");
    const char *fn = "tp_set_wells: ";
    if (nw < 0 || np < 0) throw Error(std::string(fn) + "negative count");
    Wells &W = c->wells;
    if (nw > 0) {
        if (c->grid.nranks > 1 || c->dist)
            throw Error(std::string(fn) + "wells with nranks = " + std::to_string(c->grid.nranks) +
                        " are not implemented: completed wells exist on one slab");
        TP_REQUIRE(wells && perfs, "tp_set_wells: null argument");
        const GridDev &g = c->g;
        std::vector<char> covered(np, 0);
        std::map<int64_t, int> owner;
        for (int w = 0; w < nw; ++w) {
            const tp_well &t = wells[w];
            const std::string id = "well " + std::to_string(w);
            if (t.kind != 0 && t.kind != 1) throw Error(std::string(fn) + id + ": kind = " + std::to_string(t.kind) + ": 0 (producer) or 1 (injector)");
            if (!std::isfinite(t.rate) || !std::isfinite(t.bhp_limit) || !std::isfinite(t.z_ref))
                throw Error(std::string(fn) + id + ": rate, bhp_limit and z_ref must be finite numbers");
            if (t.rate < 0.0) throw Error(std::string(fn) + id + ": rate = " + std::to_string(t.rate) + ": the total rate target, >= 0");
            if (t.count < 1 || t.first < 0 || (long)t.first + t.count > np)
                throw Error(std::string(fn) + id + ": perforations [" + std::to_string(t.first) + ", " + std::to_string((long)t.first + t.count) +
                            ") outside the array of " + std::to_string(np));
            for (int k = t.first; k < t.first + t.count; ++k) {
                const tp_perf &f = perfs[k];
                const std::string pid = id + ", perforation " + std::to_string(k - t.first);
                if (covered[k]) throw Error(std::string(fn) + pid + ": entry " + std::to_string(k) + " of the perforation array belongs to two wells");
                covered[k] = 1;
                if (!std::isfinite(f.WI) || !std::isfinite(f.z)) throw Error(std::string(fn) + pid + ": WI and z must be finite numbers");
                if (!(f.WI > 0.0)) throw Error(std::string(fn) + pid + ": WI = " + std::to_string(f.WI) + ": the connection index, > 0");
                if (f.cell < g.np || f.cell >= g.np + g.nown)
                    throw Error(std::string(fn) + pid + ": cell " + std::to_string((long long)f.cell) + " lies outside the box");
                auto ins = owner.emplace(f.cell, w);
                if (!ins.second)
                    throw Error(std::string(fn) + pid + ": cell " + std::to_string((long long)f.cell) + " is already perforated by well " +
                                std::to_string(ins.first->second) + ": a cell may carry one perforation");
            }
        }
    }
    TP_HIP(hipStreamSynchronize(c->stream));       // nothing in flight reads what is replaced
    c->jac_ready = false;
    c->pc_ready = false;
    if (nw == 0) {
        W.nw = W.np = 0;
        W.wells.clear(); W.perfs.clear();
        W.wd.free(); W.cell.free(); W.WI.free(); W.dz.free(); W.rho.free(); W.pa.free(); W.pth.free();
        W.fc.free(); W.fb.free(); W.pq.free(); W.info.free(); W.r1.free();
        return;
    }
    W.nw = nw; W.np = np;
    W.wells.assign(wells, wells + nw);
    W.perfs.assign(perfs, perfs + np);
    const size_t B = c->b;
    W.wd.alloc(nw); W.rho.alloc(nw); W.info.alloc((size_t)WINFO * nw); W.r1.alloc(nw);
    W.cell.alloc(np); W.WI.alloc(np); W.dz.alloc(np); W.pa.alloc(np); W.pth.alloc(np);
    W.fc.alloc(B * np); W.fb.alloc(B * np); W.pq.alloc((size_t)3 * np);
    std::vector<long> cell(np, c->g.np);           // (entries no well refers to: a valid cell, never read)
    std::vector<double> wi(np, 1.0), dz(np, 0.0);
    for (int w = 0; w < nw; ++w)
        for (int k = wells[w].first; k < wells[w].first + wells[w].count; ++k) {
            cell[k] = (long)perfs[k].cell;
            wi[k] = perfs[k].WI;
            dz[k] = c->grid.gaxis >= 0 ? wells[w].z_ref - perfs[k].z : 0.0;
        }
    copy_sync(c, W.cell.p, cell.data(), sizeof(long) * np, hipMemcpyHostToDevice);
    copy_sync(c, W.WI.p, wi.data(), sizeof(double) * np, hipMemcpyHostToDevice);
    copy_sync(c, W.dz.p, dz.data(), sizeof(double) * np, hipMemcpyHostToDevice);
    wells_upload_control(c);
    if (c->have_old) wells_rho(c);                 // the head density belongs to the old state that is already set
}

void wells_control(tp_ctx *c, int w, double rate, double limit, int shut) {
    TP_REQUIRE(c, "null argument");
    Wells &W = c->wells;
    const char *fn = "tp_set_well_control: ";
    if (w < 0 || w >= W.nw) throw Error(std::string(fn) + "well " + std::to_string(w) + ": the context has " + std::to_string(W.nw) + " wells");
    if (!std::isfinite(rate) || !std::isfinite(limit)) throw Error(std::string(fn) + "well " + std::to_string(w) + ": rate and bhp_limit must be finite numbers");
    if (rate < 0.0) throw Error(std::string(fn) + "well " + std::to_string(w) + ": rate = " + std::to_string(rate) + ": the total rate target, >= 0");
    TP_HIP(hipStreamSynchronize(c->stream));
    W.wells[w].rate = rate; W.wells[w].bhp_limit = limit; W.wells[w].shut = shut ? 1 : 0;
    wells_upload_control(c);
    c->jac_ready = false;
    c->pc_ready = false;
}

void wells_assemble(tp_ctx *c, bool want_jac, bool want_schur) {
    Wells &W = c->wells;
    if (W.nw == 0) return;
    WellArgs a;
    a.g = c->g; a.q = c->dprm;
    a.wd = W.wd.p; a.cell = W.cell.p; a.WI = W.WI.p; a.dz = W.dz.p; a.rho = W.rho.p;
    a.pa = W.pa.p; a.pth = W.pth.p;
    a.u = c->u.p; a.R = c->R.p;
    a.J = want_jac ? c->J.p : nullptr;
    a.Sm = (want_jac && want_schur) ? c->Sm.p : nullptr;
    a.fc = W.fc.p; a.fb = W.fb.p; a.pq = W.pq.p; a.info = W.info.p; a.r1 = W.r1.p;
    a.np = W.np;
    a.grav = c->grid.gaxis >= 0 ? c->prm.g : 0.0;
    const dim3 gr(W.nw), bl(64);
    if (c->satfn) hipLaunchKernelGGL(k_wells_sat, gr, bl, 0, c->stream, a, c->dsat);
    else if (c->nph == 2) hipLaunchKernelGGL(k_wells<2>, gr, bl, 0, c->stream, a);
    else hipLaunchKernelGGL(k_wells<1>, gr, bl, 0, c->stream, a);
    TP_HIP(hipGetLastError());
}

static void wells_apply(tp_ctx *c, const double *x, double *y, bool resid) {
    Wells &W = c->wells;
    if (W.nw == 0) return;
    const dim3 gr(W.nw), bl(64);
    const long nt = c->g.ntot;
#define WA(B, M) hipLaunchKernelGGL((k_well_apply<B, M>), gr, bl, 0, c->stream, nt, W.wd.p, W.r1.p, W.cell.p, W.fc.p, W.fb.p, W.np, x, y)
    if (c->b == 3) { if (resid) WA(3, 1); else WA(3, 0); }
    else { if (resid) WA(2, 1); else WA(2, 0); }
#undef WA
    TP_HIP(hipGetLastError());
}

// The Krylov operator A = J + sum_w c_w b_w^T (the assembled Jacobian c->J and the wells' factors of the same assembly).  Only the
// Krylov methods and tp_spmv go through these two; every use of J inside the preconditioner keeps the 7-point matrix.
void krylov_apply(tp_ctx *c, double *x, double *y, bool halo) {
    if (halo) spmv_block_halo(c, c->J.p, x, y);
    else spmv_block(c, c->J.p, x, y);
    wells_apply(c, x, y, false);
}
void krylov_resid(tp_ctx *c, const double *b, const double *x, double *r) {
    resid_block_cols(c, c->J.p, b, x, c->b, r);
    wells_apply(c, x, r, true);
}
void wells_apply_only(tp_ctx *c, const double *x, double *y) { wells_apply(c, x, y, false); }

void wells_info(tp_ctx *c, tp_well_state *out) {
    Wells &W = c->wells;
    if (W.nw == 0) return;
    TP_REQUIRE(out, "null argument");
    std::vector<double> h((size_t)WINFO * W.nw);
    copy_sync(c, h.data(), W.info.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost);
    for (int w = 0; w < W.nw; ++w) {
        const double *o = h.data() + (size_t)w * WINFO;
        tp_well_state &s = out[w];
        s.bhp = o[0]; s.mode = (int32_t)o[1]; s.rate = o[2]; s.water_rate = o[3]; s.oil_rate = o[4]; s.rho = o[5];
        s.rounds = (int32_t)o[6]; s.nopen = (int32_t)o[7];
    }
}

void wells_perf_rates(tp_ctx *c, double *rate, double *water, double *oil) {
    Wells &W = c->wells;
    if (W.np == 0) return;
    const size_t n = W.np;
    if (rate) copy_sync(c, rate, W.pq.p, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (water) copy_sync(c, water, W.pq.p + n, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (oil) copy_sync(c, oil, W.pq.p + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost);
}

void wells_factors(tp_ctx *c, double *fc, double *fb) {
    Wells &W = c->wells;
    if (W.np == 0) return;
    TP_REQUIRE(c->jac_ready, "tp_well_factors: Jacobian not assembled");
    const size_t n = (size_t)c->b * W.np;
    if (fc) copy_sync(c, fc, W.fc.p, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (fb) copy_sync(c, fb, W.fb.p, sizeof(double) * n, hipMemcpyDeviceToHost);
}

}  // namespace tp
