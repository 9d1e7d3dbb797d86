// DG0/TPFA residual + exact block Jacobian (+ temperature convection-diffusion operator S~) on the
// structured slab, hand-written for gfx950.
//
// Replaces the TSFC/PyOP2-generated cell and interior-facet kernels the reference runs for
//   F        singlephase.py:60-165,167-273 / twophase.py:67-235,237-411
//   dF/du    thermalmodel.py:36 (derivative(F,u), assembled into MatAIJ)
//   S~       preconditioners.py:11-163 (ConvDiffSchurPC), :165-333 (ConvDiffSchurTwoPhasesPC)
// and the closure laws of physicalparameters.py:37-98.
//
// One thread per owned cell (coalesced: consecutive lanes = consecutive cells along axis 0).  The
// thread evaluates the closures of its own cell once and of each face neighbour on the fly
// (7 closure evaluations per cell; the neighbour states come from L2, each state byte is fetched
// from HBM once), forms the six face fluxes with their derivatives w.r.t. both sides, and writes
// its residual entries, its diagonal block and its six off-diagonal blocks -- every Jacobian
// plane is written exactly once, fully coalesced, no atomics.  HBM-bound: ~616 B per cell
// (SURVEY.md 8d); the 3 exp + 1 pow per closure evaluation stay under the memory time.  The SATFN instantiations
// (tp_set_saturation_functions) add up to three pow per evaluation: measured in DESIGN.md 4.1.3.
#include "tp_common.hpp"
#include "tp_closures.hpp"
#include <cstdlib>
#include <cmath>
#include <algorithm>

namespace tp {

// ------------------------------------------------------------------------------------------------
template <int NPH>
struct Props {
    double p, T, S;
    double rf1, rf2;              // ro = rf1 * rf2 (oil_rho_factors)
    double ro, ro_p, ro_T;
    double Lo[4];                 // kr_o rho_o / mu_o and d/d(p,T,S)
    double rw, rw_p, rw_T;
    double Lw[4];
    double kT, kT_S;
    double mo, mw;
    double pc, pc_S, rw_S;        // SATFN only: p_c(S), its slope, and d rho_w / dS = -rw_p pc_S of rho_w(p - p_c(S), T)
};

// SATFN (tp_set_saturation_functions): kr_o, kr_w and p_c of `sat` instead of S, 1 - S and 0; water's density
// and its mobility at p_w = p - p_c(S).  The kr slopes and rw_S go into Lo[3] and Lw[3].  The false branch is the code as it was.
template <int NPH, bool SATFN = false>
__device__ __forceinline__ Props<NPH> eval_props(double p, double T, double S, double phi, double kTs,
                                                 const DevPrm &q, const DevSat *sat = nullptr) {
    Props<NPH> r;
    r.p = p; r.T = T; r.S = S;
    oil_rho_factors(p, T, q, r.rf1, r.rf2);
    oil_rho_from(r.rf1, r.rf2, r.ro, r.ro_p, r.ro_T);
    double mo, mo_T;
    oil_mu(T, q, mo, mo_T);
    r.mo = mo;
    if constexpr (SATFN) {
        static_assert(NPH == 2, "saturation functions need a saturation");
        const Dual1 Sd{S, 1.0};
        const Dual1 kro = kr_o_t(Sd, *sat), krw = kr_w_t(Sd, *sat), pc = pc_t(Sd, *sat);
        r.pc = pc.v; r.pc_S = pc.d;
        water_rho(p - pc.v, T, r.rw, r.rw_p, r.rw_T);
        r.rw_S = -r.rw_p * pc.d;
        double mw, mw_T;
        water_mu(T, mw, mw_T);
        r.mw = mw;
        r.Lw[0] = krw.v * r.rw / mw;
        r.Lw[1] = krw.v * r.rw_p / mw;
        r.Lw[2] = krw.v * (r.rw_T / mw - r.rw * mw_T / (mw * mw));
        r.Lw[3] = krw.d * r.rw / mw + krw.v * r.rw_S / mw;
        r.Lo[0] = kro.v * r.ro / mo;
        r.Lo[1] = kro.v * r.ro_p / mo;
        r.Lo[2] = kro.v * (r.ro_T / mo - r.ro * mo_T / (mo * mo));
        r.Lo[3] = kro.d * r.ro / mo;
        r.kT = phi * (S * q.ko + (1.0 - S) * q.kw) + (1.0 - phi) * q.kr;
        r.kT_S = phi * (q.ko - q.kw);
    } else if (NPH == 2) {
        water_rho(p, T, r.rw, r.rw_p, r.rw_T);
        double mw, mw_T;
        water_mu(T, mw, mw_T);
        r.mw = mw;
        const double kw_ = 1.0 - S;
        r.Lw[0] = kw_ * r.rw / mw;
        r.Lw[1] = kw_ * r.rw_p / mw;
        r.Lw[2] = kw_ * (r.rw_T / mw - r.rw * mw_T / (mw * mw));
        r.Lw[3] = -r.rw / mw;
        r.Lo[0] = S * r.ro / mo;
        r.Lo[1] = S * r.ro_p / mo;
        r.Lo[2] = S * (r.ro_T / mo - r.ro * mo_T / (mo * mo));
        r.Lo[3] = r.ro / mo;
        r.kT = phi * (S * q.ko + (1.0 - S) * q.kw) + (1.0 - phi) * q.kr;   // twophase.py:135,311
        r.kT_S = phi * (q.ko - q.kw);
    } else {
        r.Lo[0] = r.ro / mo;
        r.Lo[1] = r.ro_p / mo;
        r.Lo[2] = r.ro_T / mo - r.ro * mo_T / (mo * mo);
        r.Lo[3] = 0.0;
        r.kT = kTs;
        r.kT_S = 0.0;
        r.rw = r.rw_p = r.rw_T = 0.0;
        r.Lw[0] = r.Lw[1] = r.Lw[2] = r.Lw[3] = 0.0;
        r.mw = 1.0;
    }
    return r;
}

// Flux through one face from the '+' cell P to the '-' cell M and its derivatives w.r.t. both
// states.  gam = g*Delta_h/2 on the gravity axis, else 0; Ga = |e|/Delta_h.
// GRADED (tp_set_spacing): the two cells have widths of their own, so the harmonic mean of kT weighs each side by
// its half distance over the face area: Ga carries c_P = d_P/|e| and cM carries c_M = d_M/|e|; gam = g (d_P + d_M)/2 and TK come
// from the caller as before.  The false branch is the uniform code.
// SATFN (tp_set_saturation_functions): water is driven by p_w = p - p_c(S) of either side, and its Phi depends on
// both saturations through p_c and through rho_w(p_w, T): dPhi/dS+ = -pc_S+ - gam rw_S+, dPhi/dS- = +pc_S- - gam rw_S-.
template <int NPH, bool SCHUR, bool GRADED = false, bool SATFN = false>
__device__ __forceinline__ void face_flux(const Props<NPH> &P, const Props<NPH> &M, double TK, double gam,
                                          double Ga, const DevPrm &q, double *f, double (*dP)[NPH + 1],
                                          double (*dM)[NPH + 1], double &sP, double &sM, double cM = 0.0) {
    constexpr int B = NPH + 1;
#pragma unroll
    for (int r = 0; r < B; ++r) {
        f[r] = 0.0;
#pragma unroll
        for (int c = 0; c < B; ++c) { dP[r][c] = 0.0; dM[r][c] = 0.0; }
    }
    sP = 0.0; sM = 0.0;
    auto phase = [&](double ce, double c0, bool to2, double rP, double rP_p, double rP_T, double rM,
                     double rM_p, double rM_T, const double *LP, const double *LM) {
        double Phi, dsP = 0.0, dsM = 0.0;               // dsP, dsM: dPhi/dS of either side
        if constexpr (SATFN) {
            if (!to2) {                                 // (two phases: water is the phase that has no row of its own)
                Phi = (P.p - P.pc) - (M.p - M.pc) - gam * (rP + rM);
                dsP = -P.pc_S - gam * P.rw_S;
                dsM = M.pc_S - gam * M.rw_S;
            } else Phi = P.p - M.p - gam * (rP + rM);
        } else Phi = P.p - M.p - gam * (rP + rM);
        const bool up = Phi > 0.0;                      // gt(flow, 0): strict, ties -> '-' side
        const double L = up ? LP[0] : LM[0];
        const double Tu = up ? P.T : M.T;
        const double F = TK * L * Phi;
        const double dPhiP[3] = {1.0 - gam * rP_p, -gam * rP_T, dsP};
        const double dPhiM[3] = {-1.0 - gam * rM_p, -gam * rM_T, dsM};
        f[0] += q.w0 * c0 * F;
        f[1] += ce * Tu * F;
        if (to2) f[B - 1] += q.w2 * F;
#pragma unroll
        for (int c = 0; c < B; ++c) {
            const double dFP = TK * (L * dPhiP[c] + (up ? LP[c + 1] : 0.0) * Phi);
            const double dFM = TK * (L * dPhiM[c] + (up ? 0.0 : LM[c + 1]) * Phi);
            dP[0][c] += q.w0 * c0 * dFP;
            dM[0][c] += q.w0 * c0 * dFM;
            dP[1][c] += ce * Tu * dFP;
            dM[1][c] += ce * Tu * dFM;
            if (to2) { dP[B - 1][c] += q.w2 * dFP; dM[B - 1][c] += q.w2 * dFM; }
        }
        const double adv = ce * F;
        if (up) dP[1][1] += adv; else dM[1][1] += adv;
        if (SCHUR) { if (up) sP += adv; else sM += adv; }
    };
    if (NPH == 2) {
        phase(q.c_v_w, q.c_v_w, false, P.rw, P.rw_p, P.rw_T, M.rw, M.rw_p, M.rw_T, P.Lw, M.Lw);
        phase(q.c_v_o, q.c_v_o, true, P.ro, P.ro_p, P.ro_T, M.ro, M.ro_p, M.ro_T, P.Lo, M.Lo);
    } else {
        phase(q.c_v_o, 1.0, false, P.ro, P.ro_p, P.ro_T, M.ro, M.ro_p, M.ro_T, P.Lo, M.Lo);
    }
    if (GRADED) {
        // conduction through two half cells in series: H = k_P k_M / D, D = c_P k_M + c_M k_P
        const double cP = Ga;
        const double D = cP * M.kT + cM * P.kT;
        const double H = D > 0.0 ? P.kT * M.kT / D : 0.0;
        const double dT = P.T - M.T;
        f[1] += H * dT;
        dP[1][1] += H;
        dM[1][1] -= H;
        if (SCHUR) { sP += H; sM -= H; }
        if (NPH == 2) {
            const double dHP = D > 0.0 ? cP * M.kT * M.kT / (D * D) : 0.0;
            const double dHM = D > 0.0 ? cM * P.kT * P.kT / (D * D) : 0.0;
            dP[1][2] += dT * dHP * P.kT_S;
            dM[1][2] += dT * dHM * M.kT_S;
        }
        return;
    }
    // conduction with harmonic kT (singlephase.py:103,125)
    const double s2 = P.kT + M.kT;
    const double Hk = s2 > 0.0 ? 2.0 * P.kT * M.kT / s2 : 0.0;
    const double dT = P.T - M.T;
    f[1] += Hk * Ga * dT;
    dP[1][1] += Hk * Ga;
    dM[1][1] -= Hk * Ga;
    if (SCHUR) { sP += Hk * Ga; sM -= Hk * Ga; }
    if (NPH == 2) {
        const double dHP = s2 > 0.0 ? 2.0 * M.kT * M.kT / (s2 * s2) : 0.0;
        const double dHM = s2 > 0.0 ? 2.0 * P.kT * P.kT / (s2 * s2) : 0.0;
        dP[1][2] += Ga * dT * dHP * P.kT_S;
        dM[1][2] += Ga * dT * dHM * M.kT_S;
    }
}

struct AsmArgs {
    GridDev g;
    DevPrm q;
    const double *u, *phi, *kTs, *TK[3], *acc_old;
    double Vdt;          // |E|/dt
    double gam[3];       // g*h_a/2 on the gravity axis, else 0
    double Ga[3];        // |e_a|/h_a
    double *R, *J, *Sm;
};

// Per-axis cell widths (tp_set_spacing): what the graded instantiations take on top of AsmArgs, whose Vdt, gam and Ga they do not
// read.  hs[a][i]: width of the cells of index i along internal axis a (a few KB: hs[0] is indexed by the lane, hs[1] and hs[2]
// are nearly wave-uniform; all of it stays in cache beside the 616 B per cell of the assembly).
struct Spacing {
    const double *hs[3];
    double inv_dt;       // 1/dt: the accumulation takes |E_c|/dt per cell
    double g4;           // g/4: gam_f = g (h_P + h_M)/4 on the gravity axis
    int gaxis;
};
struct AsmArgsG {
    AsmArgs a;
    Spacing sp;
};
// Saturation functions (tp_set_saturation_functions): what the SATFN instantiations take beside the arguments of their twin
template <class A> struct WithSat {
    A a;
    DevSat sat;
};
template <bool GRADED, bool SATFN = false> struct AsmSel { using type = AsmArgs; };
template <> struct AsmSel<true, false> { using type = AsmArgsG; };
template <> struct AsmSel<false, true> { using type = WithSat<AsmArgs>; };
template <> struct AsmSel<true, true> { using type = WithSat<AsmArgsG>; };
__device__ __forceinline__ const AsmArgs &asm_base(const AsmArgs &a) { return a; }
__device__ __forceinline__ const AsmArgs &asm_base(const AsmArgsG &a) { return a.a; }
// the twin's arguments inside a SATFN instantiation's (themselves otherwise), and the curves (none otherwise)
template <class A> __device__ __forceinline__ A &sat_inner(A &a) { return a; }
template <class A> __device__ __forceinline__ A &sat_inner(WithSat<A> &w) { return w.a; }
template <class A> __device__ __forceinline__ const DevSat *sat_of(const A &) { return nullptr; }
template <class A> __device__ __forceinline__ const DevSat *sat_of(const WithSat<A> &w) { return &w.sat; }

// Geometry of one graded cell: its widths, its volume and 1/|e_a| of its faces.  The area of a face along a is the product of the
// other two widths, so both cells of a face form the same c_P, c_M and gam from the same numbers: the face's flux has the same
// bits in both rows.
struct CellGeom {
    double h[3], V, invA[3];
};
__device__ __forceinline__ CellGeom cell_geom(const Spacing &sp, int i0, int i1, int i2) {
    CellGeom m;
    m.h[0] = sp.hs[0][i0]; m.h[1] = sp.hs[1][i1]; m.h[2] = sp.hs[2][i2];
    m.V = m.h[0] * m.h[1] * m.h[2];
    m.invA[0] = 1.0 / (m.h[1] * m.h[2]);
    m.invA[1] = 1.0 / (m.h[0] * m.h[2]);
    m.invA[2] = 1.0 / (m.h[0] * m.h[1]);
    return m;
}

template <int NPH, bool JAC, bool SCHUR, bool GRADED = false, bool SATFN = false>
__global__ __launch_bounds__(256) void k_assemble(typename AsmSel<GRADED, SATFN>::type aa_) {
    constexpr int B = NPH + 1;
    auto &aa = sat_inner(aa_);
    const DevSat *sat = sat_of(aa_);
    const AsmArgs &a = asm_base(aa);
    const long tid = xcd_tid();
    const GridDev &g = a.g;
    if (tid >= g.nown) return;
    const long c = g.np + tid;
    const int i2 = (int)(tid / g.np);
    const int rem = (int)(tid - (long)i2 * g.np);
    const int i1 = rem / g.n0;
    const int i0 = rem - i1 * g.n0;
    const long nt = g.ntot;
    const DevPrm &q = a.q;

    const double *up_ = a.u, *uT_ = a.u + nt, *uS_ = a.u + 2 * nt;
    const Props<NPH> me = eval_props<NPH, SATFN>(up_[c], uT_[c], NPH == 2 ? uS_[c] : 0.0, a.phi[c], a.kTs[c], q, sat);

    double R[B], Jd[B][B];
    double sd = 0.0;
    // graded: |E_c|/dt of this cell takes the place of the box's one number in the thread's copy of the arguments
    CellGeom cg;
    if constexpr (GRADED) {
        cg = cell_geom(aa.sp, i0, i1, g.off2 + i2);
        aa.a.Vdt = cg.V * aa.sp.inv_dt;
    }
    // ---- accumulation (singlephase.py:120,123 ; twophase.py:162-176) -----------------------------
    {
        const double phi = a.phi[c];
        const double rock = (1.0 - phi) * q.rho_r * q.c_r;
        if (NPH == 2) {
            const double S = me.S, T = me.T;
            const double Mw = phi * me.rw * (1.0 - S), Mo = phi * me.ro * S;
            double dMw[3] = {phi * me.rw_p * (1.0 - S), phi * me.rw_T * (1.0 - S), -phi * me.rw};
            if constexpr (SATFN) dMw[2] += phi * me.rw_S * (1.0 - S);      // rho_w(p - p_c(S), T) follows S
            const double dMo[3] = {phi * me.ro_p * S, phi * me.ro_T * S, phi * me.ro};
            const double e0 = q.c_v_w * Mw + q.c_v_o * Mo;
            R[0] = q.w0 * (e0 - a.acc_old[c]) * a.Vdt;
            R[1] = (e0 * T + rock * T - a.acc_old[nt + c]) * a.Vdt;
            R[2] = q.w2 * (Mo - a.acc_old[2 * nt + c]) * a.Vdt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double de0 = q.c_v_w * dMw[k] + q.c_v_o * dMo[k];
                Jd[0][k] = q.w0 * de0 * a.Vdt;
                Jd[1][k] = de0 * T * a.Vdt;
                Jd[2][k] = q.w2 * dMo[k] * a.Vdt;
            }
            Jd[1][1] += (e0 + rock) * a.Vdt;
            if (SCHUR) sd = (phi * q.c_v_o * S * me.ro + phi * q.c_v_w * (1.0 - S) * me.rw + rock) * a.Vdt;
        } else {
            const double T = me.T;
            const double Mo = phi * me.ro;
            const double dMo[2] = {phi * me.ro_p, phi * me.ro_T};
            R[0] = q.w0 * (Mo - a.acc_old[c]) * a.Vdt;
            R[1] = (q.c_v_o * Mo * T + rock * T - a.acc_old[nt + c]) * a.Vdt;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                Jd[0][k] = q.w0 * dMo[k] * a.Vdt;
                Jd[1][k] = q.c_v_o * dMo[k] * T * a.Vdt;
            }
            Jd[1][1] += (q.c_v_o * Mo + rock) * a.Vdt;
            if (SCHUR) sd = (phi * q.c_v_o * me.ro + rock) * a.Vdt;
        }
    }
    // ---- faces -----------------------------------------------------------------------------------
    const long stride[3] = {1, (long)g.n0, g.np};
    const int idx[3] = {i0, i1, g.off2 + i2};
    const int ext[3] = {g.n0, g.n1, g.gn2};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {          // 0: neighbour at -ax (I am '-'), 1: at +ax (I am '+')
            const int slot = 1 + 2 * ax + dir;
            const bool exists = dir ? (idx[ax] < ext[ax] - 1) : (idx[ax] > 0);
            double f[B], dP[B][B], dM[B][B], sP = 0.0, sM = 0.0;
            if (exists) {
                const long nb = dir ? c + stride[ax] : c - stride[ax];
                const Props<NPH> ot =
                    eval_props<NPH, SATFN>(up_[nb], uT_[nb], NPH == 2 ? uS_[nb] : 0.0, a.phi[nb], a.kTs[nb], q, sat);
                // graded: gam and the half distances over the area, c_me and c_nb, of this face
                double gam = 0.0, c_me = 0.0, c_nb = 0.0;
                if constexpr (GRADED) {
                    const double hn = aa.sp.hs[ax][dir ? idx[ax] + 1 : idx[ax] - 1];
                    gam = ax == aa.sp.gaxis ? aa.sp.g4 * (dir ? cg.h[ax] + hn : hn + cg.h[ax]) : 0.0;
                    c_me = 0.5 * cg.h[ax] * cg.invA[ax];
                    c_nb = 0.5 * hn * cg.invA[ax];
                }
                if (dir) {
                    if constexpr (GRADED)
                        face_flux<NPH, SCHUR, true, SATFN>(me, ot, a.TK[ax][c], gam, c_me, q, f, dP, dM, sP, sM, c_nb);
                    else
                        face_flux<NPH, SCHUR, false, SATFN>(me, ot, a.TK[ax][c], a.gam[ax], a.Ga[ax], q, f, dP, dM, sP, sM);
#pragma unroll
                    for (int r = 0; r < B; ++r) {
                        R[r] += f[r];
#pragma unroll
                        for (int k = 0; k < B; ++k) Jd[r][k] += dP[r][k];
                    }
                    if (SCHUR) sd += sP;
                } else {
                    if constexpr (GRADED)
                        face_flux<NPH, SCHUR, true, SATFN>(ot, me, a.TK[ax][nb], gam, c_nb, q, f, dP, dM, sP, sM, c_me);
                    else
                        face_flux<NPH, SCHUR, false, SATFN>(ot, me, a.TK[ax][nb], a.gam[ax], a.Ga[ax], q, f, dP, dM, sP, sM);
#pragma unroll
                    for (int r = 0; r < B; ++r) {
                        R[r] -= f[r];
#pragma unroll
                        for (int k = 0; k < B; ++k) Jd[r][k] -= dM[r][k];
                    }
                    if (SCHUR) sd -= sM;
                }
            }
            if (JAC) {
#pragma unroll
                for (int r = 0; r < B; ++r)
#pragma unroll
                    for (int k = 0; k < B; ++k) {
                        double v = 0.0;
                        if (exists) v = dir ? dM[r][k] : -dP[r][k];
                        a.J[((long)(slot * B + r) * B + k) * nt + c] = v;
                    }
            }
            if (SCHUR) a.Sm[(long)slot * nt + c] = exists ? (dir ? sM : -sP) : 0.0;
        }
    }
#pragma unroll
    for (int r = 0; r < B; ++r) a.R[(long)r * nt + c] = R[r];
    if (JAC) {
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int k = 0; k < B; ++k) a.J[((long)(r)*B + k) * nt + c] = Jd[r][k];
    }
    if (SCHUR) a.Sm[c] = sd;
}

// ---- LDS-tiled variant (north_star: "LDS staging of per-face neighbour blocks"; TP_ASM_LDS=1) ----------------------
// A workgroup of 256 threads owns a 16 x 4 x 4 tile of cells.  Phase 1 evaluates the closures ONCE per cell of the tile and
// of its six face halos (544 evaluations for 256 cells: 2.1 per cell instead of the 7 of k_assemble) into an LDS image,
// structure-of-arrays [value][slot of the 18 x 6 x 6 box]; phase 2 is k_assemble's cell body with every Props read from the
// LDS.  Same functions on the same inputs: results are bitwise those of k_assemble (tests/test_gpu_assembly_edges.py).  For that
// the image holds the oil density as its two factors, not as their product: rho_o goes straight into the sum rho+ + rho- of the
// driving force, and under -ffp-contract=fast k_assemble, which inlines eval_props, contracts product and sum into one fma; a
// product rounded into the image first gave another last bit in a few entries.  Measured on C4.
constexpr int ATX = 16, ATY = 4, ATZ = 4, ABX = ATX + 2, ABY = ATY + 2, ABZ = ATZ + 2, ANS = ABX * ABY * ABZ;
template <int NPH> struct PropsLds {
    static constexpr int NV = NPH == 2 ? 18 : 8;
    static __device__ __forceinline__ void put(double *l, int s, const Props<NPH> &r) {
        int v = 0;
        auto w = [&](double x) { l[(v++) * ANS + s] = x; };
        w(r.p); w(r.T); w(r.rf1); w(r.rf2); w(r.Lo[0]); w(r.Lo[1]); w(r.Lo[2]); w(r.kT);
        if (NPH == 2) { w(r.S); w(r.Lo[3]); w(r.rw); w(r.rw_p); w(r.rw_T); w(r.Lw[0]); w(r.Lw[1]); w(r.Lw[2]); w(r.Lw[3]); w(r.kT_S); }
    }
    static __device__ __forceinline__ Props<NPH> get(const double *l, int s) {
        Props<NPH> r;
        int v = 0;
        auto rd = [&]() { return l[(v++) * ANS + s]; };
        r.p = rd(); r.T = rd(); r.rf1 = rd(); r.rf2 = rd(); oil_rho_from(r.rf1, r.rf2, r.ro, r.ro_p, r.ro_T); r.Lo[0] = rd(); r.Lo[1] = rd(); r.Lo[2] = rd(); r.kT = rd();
        if (NPH == 2) {
            r.S = rd(); r.Lo[3] = rd(); r.rw = rd(); r.rw_p = rd(); r.rw_T = rd();
            r.Lw[0] = rd(); r.Lw[1] = rd(); r.Lw[2] = rd(); r.Lw[3] = rd(); r.kT_S = rd();
        } else {
            r.S = 0.0; r.Lo[3] = 0.0; r.kT_S = 0.0; r.rw = r.rw_p = r.rw_T = 0.0;
            r.Lw[0] = r.Lw[1] = r.Lw[2] = r.Lw[3] = 0.0;
        }
        r.mo = r.mw = 1.0;          // (not used by the fluxes)
        return r;
    }
};

template <int NPH, bool JAC, bool SCHUR>
__global__ __launch_bounds__(256) void k_assemble_lds(AsmArgs a) {
    constexpr int B = NPH + 1;
    extern __shared__ double lds[];
    const GridDev &g = a.g;
    const long nt = g.ntot;
    const DevPrm &q = a.q;
    const int X0 = blockIdx.x * ATX, Y0 = blockIdx.y * ATY, Z0 = blockIdx.z * ATZ;
    const double *up_ = a.u, *uT_ = a.u + nt, *uS_ = a.u + 2 * nt;
    // ---- phase 1: closures of the tile and its face halos, once each --------------------------------------------------
    for (int s = threadIdx.x; s < ANS; s += 256) {
        const int bx = s % ABX, by = (s / ABX) % ABY, bz = s / (ABX * ABY);
        const int nh = (bx == 0 || bx == ABX - 1) + (by == 0 || by == ABY - 1) + (bz == 0 || bz == ABZ - 1);
        const int i0 = X0 + bx - 1, i1 = Y0 + by - 1, i2 = Z0 + bz - 1;
        const int gz = g.off2 + i2;
        if (nh > 1 || i0 < 0 || i0 >= g.n0 || i1 < 0 || i1 >= g.n1 || i2 < -1 || i2 > g.n2 || gz < 0 || gz >= g.gn2) continue;
        const long cc = g.np + (long)i0 + (long)g.n0 * i1 + g.np * i2;
        PropsLds<NPH>::put(lds, s, eval_props<NPH>(up_[cc], uT_[cc], NPH == 2 ? uS_[cc] : 0.0, a.phi[cc], a.kTs[cc], q));
    }
    __syncthreads();
    // ---- phase 2: one thread per cell of the tile (k_assemble's body; Props from the LDS image) ------------------------
    const int lx = threadIdx.x & (ATX - 1), ly = (threadIdx.x / ATX) & (ATY - 1), lz = threadIdx.x / (ATX * ATY);
    const int i0 = X0 + lx, i1 = Y0 + ly, i2 = Z0 + lz;
    if (i0 >= g.n0 || i1 >= g.n1 || i2 >= g.n2) return;
    const long c = g.np + (long)i0 + (long)g.n0 * i1 + g.np * i2;
    const int sme = (lx + 1) + ABX * ((ly + 1) + ABY * (lz + 1));
    const Props<NPH> me = PropsLds<NPH>::get(lds, sme);
    double R[B], Jd[B][B];
    double sd = 0.0;
    {
        const double phi = a.phi[c];
        const double rock = (1.0 - phi) * q.rho_r * q.c_r;
        if (NPH == 2) {
            const double S = me.S, T = me.T;
            const double Mw = phi * me.rw * (1.0 - S), Mo = phi * me.ro * S;
            const double dMw[3] = {phi * me.rw_p * (1.0 - S), phi * me.rw_T * (1.0 - S), -phi * me.rw};
            const double dMo[3] = {phi * me.ro_p * S, phi * me.ro_T * S, phi * me.ro};
            const double e0 = q.c_v_w * Mw + q.c_v_o * Mo;
            R[0] = q.w0 * (e0 - a.acc_old[c]) * a.Vdt;
            R[1] = (e0 * T + rock * T - a.acc_old[nt + c]) * a.Vdt;
            R[2] = q.w2 * (Mo - a.acc_old[2 * nt + c]) * a.Vdt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double de0 = q.c_v_w * dMw[k] + q.c_v_o * dMo[k];
                Jd[0][k] = q.w0 * de0 * a.Vdt;
                Jd[1][k] = de0 * T * a.Vdt;
                Jd[2][k] = q.w2 * dMo[k] * a.Vdt;
            }
            Jd[1][1] += (e0 + rock) * a.Vdt;
            if (SCHUR) sd = (phi * q.c_v_o * S * me.ro + phi * q.c_v_w * (1.0 - S) * me.rw + rock) * a.Vdt;
        } else {
            const double T = me.T;
            const double Mo = phi * me.ro;
            const double dMo[2] = {phi * me.ro_p, phi * me.ro_T};
            R[0] = q.w0 * (Mo - a.acc_old[c]) * a.Vdt;
            R[1] = (q.c_v_o * Mo * T + rock * T - a.acc_old[nt + c]) * a.Vdt;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                Jd[0][k] = q.w0 * dMo[k] * a.Vdt;
                Jd[1][k] = q.c_v_o * dMo[k] * T * a.Vdt;
            }
            Jd[1][1] += (q.c_v_o * Mo + rock) * a.Vdt;
            if (SCHUR) sd = (phi * q.c_v_o * me.ro + rock) * a.Vdt;
        }
    }
    const long stride[3] = {1, (long)g.n0, g.np};
    const int sstride[3] = {1, ABX, ABX * ABY};
    const int idx[3] = {i0, i1, g.off2 + i2};
    const int ext[3] = {g.n0, g.n1, g.gn2};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const int slot = 1 + 2 * ax + dir;
            const bool exists = dir ? (idx[ax] < ext[ax] - 1) : (idx[ax] > 0);
            double f[B], dP[B][B], dM[B][B], sP = 0.0, sM = 0.0;
            if (exists) {
                const long nb = dir ? c + stride[ax] : c - stride[ax];
                const Props<NPH> ot = PropsLds<NPH>::get(lds, dir ? sme + sstride[ax] : sme - sstride[ax]);
                if (dir) {
                    face_flux<NPH, SCHUR>(me, ot, a.TK[ax][c], a.gam[ax], a.Ga[ax], q, f, dP, dM, sP, sM);
#pragma unroll
                    for (int r = 0; r < B; ++r) {
                        R[r] += f[r];
#pragma unroll
                        for (int k = 0; k < B; ++k) Jd[r][k] += dP[r][k];
                    }
                    if (SCHUR) sd += sP;
                } else {
                    face_flux<NPH, SCHUR>(ot, me, a.TK[ax][nb], a.gam[ax], a.Ga[ax], q, f, dP, dM, sP, sM);
#pragma unroll
                    for (int r = 0; r < B; ++r) {
                        R[r] -= f[r];
#pragma unroll
                        for (int k = 0; k < B; ++k) Jd[r][k] -= dM[r][k];
                    }
                    if (SCHUR) sd -= sM;
                }
            }
            if (JAC) {
#pragma unroll
                for (int r = 0; r < B; ++r)
#pragma unroll
                    for (int k = 0; k < B; ++k) {
                        double v = 0.0;
                        if (exists) v = dir ? dM[r][k] : -dP[r][k];
                        a.J[((long)(slot * B + r) * B + k) * nt + c] = v;
                    }
            }
            if (SCHUR) a.Sm[(long)slot * nt + c] = exists ? (dir ? sM : -sP) : 0.0;
        }
    }
#pragma unroll
    for (int r = 0; r < B; ++r) a.R[(long)r * nt + c] = R[r];
    if (JAC) {
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int k = 0; k < B; ++k) a.J[((long)(r)*B + k) * nt + c] = Jd[r][k];
    }
    if (SCHUR) a.Sm[c] = sd;
}

// ---- Dirichlet sides (tp_set_boundary) ---------------------------------------------------------------------
// A boundary face is an interior face whose other cell is a ghost state half a cell away: face_flux, unchanged, between the
// cell and Props evaluated at (p_b, T_b, S_b) with the cell's own phi and static kT.  Orientation as inside: the lower index
// is '+', so on a high side (d = 1) the cell is P and the ghost M, on a low side the ghost is P and the cell M.  Half-cell
// distance: T^K = 2 K_a(c)|E|/h_a^2 (open) or 0 (thermal: conduction only), Ga = 2|e_a|/h_a, gam = g h_a/4 on the gravity axis.
// There is no ghost unknown: only R, the diagonal block of J and the diagonal of S~ gain terms.
//
// One thread per boundary cell, for ALL the set sides that cell lies on (an edge or corner cell has one writer, no atomics),
// launched behind the cell kernel on the same stream: read-modify-write of R, slot 0 of J and Sm[c].  The cell list is sorted,
// so consecutive lanes hold consecutive cells wherever the surface has them: whole planes on the sides of axis 2, runs of n0
// on the sides of axis 1.  On the sides of axis 0 consecutive lanes are n0 cells apart and every access by cell index costs a
// memory transaction per lane; the per-face arrays (ghost values, T^K, flux scratch) stay contiguous there too, because the
// face number follows the same order as the sorted cells.
struct BcArgs {
    AsmArgs a;
    const int *cells;
    int ncells;
    int kind[6];
    const double *val[6], *tk[6];
    double *flux[6];
    long nf[6];
};

__device__ __forceinline__ long bc_face(const GridDev &g, int ax, int i0, int i1, int i2) {
    return ax == 0 ? (long)i1 + (long)g.n1 * i2 : (ax == 1 ? (long)i0 + (long)g.n0 * i2 : (long)i0 + (long)g.n0 * i1);
}

// graded (tp_set_spacing): the same face with both half distances h_a(c)/4, h_a(c) the boundary cell's own width along the side's
// axis: c_P = c_M = h/(4|e|), gam = g h/4; T^K = 2 K|e|/h comes from k_bc_trans_g
struct BcArgsG {
    BcArgs s;
    Spacing sp;
};
template <bool GRADED, bool SATFN = false> struct BcSel { using type = BcArgs; };
template <> struct BcSel<true, false> { using type = BcArgsG; };
template <> struct BcSel<false, true> { using type = WithSat<BcArgs>; };
template <> struct BcSel<true, true> { using type = WithSat<BcArgsG>; };
__device__ __forceinline__ const BcArgs &bc_base(const BcArgs &s) { return s; }
__device__ __forceinline__ const BcArgs &bc_base(const BcArgsG &s) { return s.s; }

// SATFN: the cell and the ghost state (p_b, T_b, S_b) go through the same curves
template <int NPH, bool JAC, bool SCHUR, bool GRADED = false, bool SATFN = false>
__global__ __launch_bounds__(256) void k_assemble_bc(typename BcSel<GRADED, SATFN>::type ss_) {
    constexpr int B = NPH + 1;
    auto &ss = sat_inner(ss_);
    const DevSat *sat = sat_of(ss_);
    const BcArgs &s = bc_base(ss);
    const int t = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (t >= s.ncells) return;
    const AsmArgs &a = s.a;
    const GridDev &g = a.g;
    const DevPrm &q = a.q;
    const long tid = s.cells[t];
    const long c = g.np + tid;
    const int i2 = (int)(tid / g.np);
    const int rem = (int)(tid - (long)i2 * g.np);
    const int i1 = rem / g.n0;
    const int i0 = rem - i1 * g.n0;
    const long nt = g.ntot;
    const double phi = a.phi[c], kTs = a.kTs[c];
    const Props<NPH> me = eval_props<NPH, SATFN>(a.u[c], a.u[nt + c], NPH == 2 ? a.u[2 * nt + c] : 0.0, phi, kTs, q, sat);
    double R[B], Jd[B][B], sd = 0.0;
#pragma unroll
    for (int r = 0; r < B; ++r) {
        R[r] = 0.0;
#pragma unroll
        for (int k = 0; k < B; ++k) Jd[r][k] = 0.0;
    }
#pragma unroll 1
    for (int side = 0; side < 6; ++side) {
        const int ax = side >> 1, dir = side & 1;
        const int ia = ax == 0 ? i0 : (ax == 1 ? i1 : i2);          // (selects, not indexed local arrays: nothing to demote to scratch)
        const int na = ax == 0 ? g.n0 : (ax == 1 ? g.n1 : g.n2);
        if (s.kind[side] == 0 || ia != (dir ? na - 1 : 0)) continue;
        const long nf = s.nf[side];
        const long f_ = bc_face(g, ax, i0, i1, i2);
        const double *v = s.val[side];
        const Props<NPH> gh = eval_props<NPH, SATFN>(v[f_], v[nf + f_], NPH == 2 ? v[2 * nf + f_] : 0.0, phi, kTs, q, sat);
        const double TK = s.tk[side][f_];
        double gam, Ga;
        if constexpr (GRADED) {
            const Spacing &sp = ss.sp;
            const double h0 = sp.hs[0][i0], h1 = sp.hs[1][i1], h2 = sp.hs[2][i2];
            const double h = ax == 0 ? h0 : (ax == 1 ? h1 : h2);
            const double A = ax == 0 ? h1 * h2 : (ax == 1 ? h0 * h2 : h0 * h1);
            gam = ax == sp.gaxis ? sp.g4 * h : 0.0;
            Ga = 0.25 * h / A;                                 // (c_P = c_M: the ghost lies as far from the face as the centre)
        } else {
            gam = 0.5 * a.gam[ax];
            Ga = 2.0 * a.Ga[ax];
        }
        double f[B], dP[B][B], dM[B][B], sP = 0.0, sM = 0.0;
        if (dir) face_flux<NPH, SCHUR, GRADED, SATFN>(me, gh, TK, gam, Ga, q, f, dP, dM, sP, sM, Ga);
        else     face_flux<NPH, SCHUR, GRADED, SATFN>(gh, me, TK, gam, Ga, q, f, dP, dM, sP, sM, Ga);
        const double sg = dir ? 1.0 : -1.0;
#pragma unroll
        for (int r = 0; r < B; ++r) {
            const double fr = sg * f[r];
            R[r] += fr;
            s.flux[side][(long)r * nf + f_] = fr;
            if (JAC) {
#pragma unroll
                for (int k = 0; k < B; ++k) Jd[r][k] += dir ? dP[r][k] : -dM[r][k];
            }
        }
        if (SCHUR) sd += dir ? sP : -sM;
    }
#pragma unroll
    for (int r = 0; r < B; ++r) a.R[(long)r * nt + c] += R[r];
    if (JAC) {
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int k = 0; k < B; ++k) a.J[((long)r * B + k) * nt + c] += Jd[r][k];
    }
    if (SCHUR) a.Sm[c] += sd;
}

// half-cell transmissibility of every face of one side: one thread per face
__global__ void k_bc_trans(GridDev g, const double *K, int side, int open, double geom, long nf, double *tk) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int ax = side >> 1, dir = side & 1;
    const int na = ax == 0 ? g.n1 : g.n0;                 // extent of the faster of the two other axes
    const int lo = (int)(f % na), hi = (int)(f / na);
    int i0, i1, i2;
    if (ax == 0)      { i0 = dir ? g.n0 - 1 : 0; i1 = lo; i2 = hi; }
    else if (ax == 1) { i0 = lo; i1 = dir ? g.n1 - 1 : 0; i2 = hi; }
    else              { i0 = lo; i1 = hi; i2 = dir ? g.n2 - 1 : 0; }
    const long c = g.np + (long)i0 + (long)g.n0 * i1 + g.np * i2;
    tk[f] = open ? 2.0 * K[c] * geom : 0.0;
}

// graded: T^K = K/(2c) with c = h_a(c)/(4|e|), i.e. 2 K |e| / h_a(c) with the cell's own width and face area
__global__ void k_bc_trans_g(GridDev g, const double *K, int side, int open, const double *hs0, const double *hs1,
                             const double *hs2, long nf, double *tk) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int ax = side >> 1, dir = side & 1;
    const int na = ax == 0 ? g.n1 : g.n0;
    const int lo = (int)(f % na), hi = (int)(f / na);
    int i0, i1, i2;
    if (ax == 0)      { i0 = dir ? g.n0 - 1 : 0; i1 = lo; i2 = hi; }
    else if (ax == 1) { i0 = lo; i1 = dir ? g.n1 - 1 : 0; i2 = hi; }
    else              { i0 = lo; i1 = hi; i2 = dir ? g.n2 - 1 : 0; }
    const long c = g.np + (long)i0 + (long)g.n0 * i1 + g.np * i2;
    const double h0 = hs0[i0], h1 = hs1[i1], h2 = hs2[i2];
    const double h = ax == 0 ? h0 : (ax == 1 ? h1 : h2);
    const double A = ax == 0 ? h1 * h2 : (ax == 1 ? h0 * h2 : h0 * h1);
    tk[f] = open ? 2.0 * K[c] * A / h : 0.0;
}

// ---- accumulation of the old state (once per time step) -------------------------------------------
// SATFN: water's density at p_old - p_c(S_old), as the accumulation of the new state takes it
template <int NPH, bool SATFN>
__device__ __forceinline__ void accum_old_cell(const GridDev &g, const DevPrm &q, const double *u, const double *phi_, double *acc,
                                               const DevSat *sat) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= g.nown) return;
    const long c = g.np + tid, nt = g.ntot;
    const double p = u[c], T = u[nt + c];
    const double phi = phi_[c];
    const double rock = (1.0 - phi) * q.rho_r * q.c_r;
    double ro, ro_p, ro_T;
    oil_rho(p, T, q, ro, ro_p, ro_T);
    if (NPH == 2) {
        const double S = u[2 * nt + c];
        double rw, rw_p, rw_T;
        if constexpr (SATFN) water_rho(p - pc_t(Dual1{S, 1.0}, *sat).v, T, rw, rw_p, rw_T);
        else water_rho(p, T, rw, rw_p, rw_T);
        const double Mw = phi * rw * (1.0 - S), Mo = phi * ro * S;
        const double e0 = q.c_v_w * Mw + q.c_v_o * Mo;
        acc[c] = e0;
        acc[nt + c] = e0 * T + rock * T;
        acc[2 * nt + c] = Mo;
    } else {
        const double Mo = phi * ro;
        acc[c] = Mo;
        acc[nt + c] = q.c_v_o * Mo * T + rock * T;
    }
}
template <int NPH>
__global__ void k_accum_old(GridDev g, DevPrm q, const double *u, const double *phi_, double *acc) {
    accum_old_cell<NPH, false>(g, q, u, phi_, acc, nullptr);
}
__global__ void k_accum_old_sat(GridDev g, DevPrm q, const double *u, const double *phi_, double *acc, DevSat sat) {
    accum_old_cell<2, true>(g, q, u, phi_, acc, &sat);
}

// ---- face transmissibilities T^K_f = H(K)|e|/Delta_h (singlephase.py:98-103) -----------------------
__global__ void k_trans(GridDev g, const double *K, int ax, double geom, double *TK) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= g.nown) return;
    const long c = g.np + tid;
    const int i2 = (int)(tid / g.np);
    const int rem = (int)(tid - (long)i2 * g.np);
    const int i1 = rem / g.n0, i0 = rem - i1 * g.n0;
    const long stride = ax == 0 ? 1 : (ax == 1 ? g.n0 : g.np);
    const int idx = ax == 0 ? i0 : (ax == 1 ? i1 : g.off2 + i2);
    const int ext = ax == 0 ? g.n0 : (ax == 1 ? g.n1 : g.gn2);
    double t = 0.0;
    if (idx < ext - 1) {
        const double kp = K[c], km = K[c + stride];
        const double s = kp + km;
        t = s > 0.0 ? 2.0 * kp * km / s * geom : 0.0;
    }
    TK[c] = t;
}

// graded (tp_set_spacing): T^K = K_P K_M / (c_P K_M + c_M K_P), c = (h_a/2)/|e|, |e| the product of the other two widths; 0 where
// the denominator is not positive.  One GPU: idx along axis 2 is the plane itself and the halo plane of TK[2] stays zero.
__global__ void k_trans_g(GridDev g, const double *K, int ax, const double *hs0, const double *hs1, const double *hs2, double *TK) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= g.nown) return;
    const long c = g.np + tid;
    const int i2 = (int)(tid / g.np);
    const int rem = (int)(tid - (long)i2 * g.np);
    const int i1 = rem / g.n0, i0 = rem - i1 * g.n0;
    const long stride = ax == 0 ? 1 : (ax == 1 ? g.n0 : g.np);
    const int idx = ax == 0 ? i0 : (ax == 1 ? i1 : i2);
    const int ext = ax == 0 ? g.n0 : (ax == 1 ? g.n1 : g.n2);
    double t = 0.0;
    if (idx < ext - 1) {
        const double h0 = hs0[i0], h1 = hs1[i1], h2 = hs2[i2];
        const double *hs = ax == 0 ? hs0 : (ax == 1 ? hs1 : hs2);
        const double A = ax == 0 ? h1 * h2 : (ax == 1 ? h0 * h2 : h0 * h1);
        const double cp = 0.5 * hs[idx] / A, cm = 0.5 * hs[idx + 1] / A;
        const double kp = K[c], km = K[c + stride];
        const double d = cp * km + cm * kp;
        t = d > 0.0 ? kp * km / d : 0.0;
    }
    TK[c] = t;
}

// lower halo plane of TK[2]: the face between the last plane of the slab below and my first plane
__global__ void k_trans_halo(GridDev g, const double *K, double geom, double *TK) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.np) return;
    double v = 0.0;
    if (g.off2 > 0) {
        const double kp = K[t], km = K[t + g.np];
        const double s = kp + km;
        v = s > 0.0 ? 2.0 * kp * km / s * geom : 0.0;
    }
    TK[t] = v;
}

// ---- wells / heaters: tiny kernel, one thread per group of entries sharing a cell ------------------
// Rate laws: wellcase.py:171-266; contributions to F: singlephase.py:151-165, twophase.py:212-235;
// to S~: preconditioners.py:102-108,269-276.  Derivatives by forward-mode duals (3 partials).
// SATFN (tp_set_saturation_functions): the producers' total mobility and phase split use kr_a(S_o)/mu_a of the curves; drawdown
// and densities stay at p, injectors inject water only and do not change.
template <int NPH, bool SATFN = false>
__device__ void source_eval(const tp_source &e, const DevPrm &q, Dual3 p, Dual3 T, Dual3 S, Dual3 *out,
                            double *rates, double &schur_diag, const DevSat *sat = nullptr) {
    constexpr int B = NPH + 1;
    for (int r = 0; r < B; ++r) out[r] = Dual3(0.0);
    rates[0] = rates[1] = rates[2] = 0.0;
    schur_diag = 0.0;
    if (e.kind == 2) {                                  // heater: R_E -= U (T_inj - T) wt
        out[1] = (Dual3(q.T_inj) - T) * (q.U * e.wt);
        schur_diag = -q.U * e.wt;
        return;
    }
    const Dual3 mo = oil_mu_t(T, q);
    const Dual3 ro = oil_rho_t(p, T, q);
    const Dual3 ddr = Dual3(e.bhp) - p;
    Dual3 dd;
    if (e.kind == 0) dd = (ddr.v >= 0.0) ? Dual3(0.0) : ddr;   // conditional(ge(bhp-p,0),0,bhp-p)
    else             dd = (ddr.v <= 0.0) ? Dual3(0.0) : ddr;   // conditional(le(bhp-p,0),0,bhp-p)
    auto cap = [&](Dual3 rate) {
        if (fabs(rate.v) - fabs(e.max_rate) >= 0.0) rate = Dual3(e.max_rate);
        if (e.constant_rate) rate = Dual3(e.max_rate);
        return rate;
    };
    if (NPH == 1) {
        const Dual3 rate = cap(dd * (e.WI) / mo);
        rates[0] = rate.v;
        if (e.kind == 0) {
            out[0] = ro * rate * (q.w0 * e.wt);
            out[1] = ro * rate * T * (q.c_v_o * e.wt);
            schur_diag = ro.v * rate.v * q.c_v_o * e.wt;
        } else {
            const Dual3 roi = oil_rho_t(p, Dual3(q.T_inj), q);
            out[0] = roi * rate * (q.w0 * e.wt);
            out[1] = roi * rate * (q.c_v_o * q.T_inj * e.wt);
        }
    } else {
        const Dual3 mw = water_mu_t(T);
        const Dual3 rw = water_rho_t(p, T);
        if (e.kind == 0) {
            Dual3 lam_o, lam_w;
            if constexpr (SATFN) { lam_o = kr_o_t(S, *sat) / mo; lam_w = kr_w_t(S, *sat) / mw; }
            else { lam_o = S / mo; lam_w = (Dual3(1.0) - S) / mw; }
            const Dual3 lam_t = lam_o + lam_w;
            const Dual3 rate = cap(dd * lam_t * e.WI);
            const Dual3 qw = lam_w / lam_t * rate;
            const Dual3 qo = lam_o / lam_t * rate;
            rates[0] = rate.v; rates[1] = qw.v; rates[2] = qo.v;
            out[0] = (rw * qw * q.c_v_w + ro * qo * q.c_v_o) * (q.w0 * e.wt);
            out[2] = ro * qo * (q.w2 * e.wt);
            out[1] = (rw * qw * q.c_v_w + ro * qo * q.c_v_o) * T * e.wt;
            schur_diag = (rw.v * qw.v * q.c_v_w + ro.v * qo.v * q.c_v_o) * e.wt;
        } else {
            const Dual3 rate = cap(dd * e.WI / mw);
            rates[0] = rate.v;
            const Dual3 rwi = water_rho_t(p, Dual3(q.T_inj));
            out[0] = rwi * rate * (q.w0 * q.c_v_w * e.wt);
            out[1] = rwi * rate * (q.c_v_w * q.T_inj * e.wt);
        }
    }
}

template <int NPH, bool SATFN>
__device__ __forceinline__ void sources_group(const GridDev &g, const DevPrm &q, const tp_source *src, const int *start, int ngroups,
                                              const double *u, double *R, double *J, double *Sm, double *rates, int nsrc,
                                              const DevSat *sat) {
    constexpr int B = NPH + 1;
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= ngroups) return;
    const long nt = g.ntot;
    const long c = src[start[gi]].cell;
    Dual3 p(u[c], 0), T(u[nt + c], 1), S(NPH == 2 ? u[2 * nt + c] : 0.0, 2);
    for (int k = start[gi]; k < start[gi + 1]; ++k) {
        Dual3 out[B];
        double rt[3], sd;
        source_eval<NPH, SATFN>(src[k], q, p, T, S, out, rt, sd, sat);
        if (rates) { rates[k] = rt[0]; rates[nsrc + k] = rt[1]; rates[2 * nsrc + k] = rt[2]; }
        if (R)
            for (int r = 0; r < B; ++r) R[(long)r * nt + c] -= out[r].v;
        if (J)
            for (int r = 0; r < B; ++r)
                for (int k2 = 0; k2 < B; ++k2) J[((long)r * B + k2) * nt + c] -= out[r].d[k2];
        if (Sm) Sm[c] -= sd;
    }
}
template <int NPH>
__global__ void k_sources(GridDev g, DevPrm q, const tp_source *src, const int *start, int ngroups,
                          const double *u, double *R, double *J, double *Sm, double *rates, int nsrc) {
    sources_group<NPH, false>(g, q, src, start, ngroups, u, R, J, Sm, rates, nsrc, nullptr);
}
__global__ void k_sources_sat(GridDev g, DevPrm q, const tp_source *src, const int *start, int ngroups,
                              const double *u, double *R, double *J, double *Sm, double *rates, int nsrc, DevSat sat) {
    sources_group<2, true>(g, q, src, start, ngroups, u, R, J, Sm, rates, nsrc, &sat);
}

// ------------------------------------------------------------------------------------------------

void compute_trans(tp_ctx *c) {
    const GridDev &g = c->g;
    if (c->graded) {
        for (int ax = 0; ax < 3; ++ax)
            hipLaunchKernelGGL(k_trans_g, grid_for(g.nown), dim3(256), 0, c->stream, g, c->K[ax].p, ax, c->hs[0].p, c->hs[1].p,
                               c->hs[2].p, c->TK[ax].p);
        // (one slab, off2 == 0: the uniform halo kernel writes the zeros of a box without a slab below)
        hipLaunchKernelGGL(k_trans_halo, grid_for(g.np), dim3(256), 0, c->stream, g, c->K[2].p, 0.0, c->TK[2].p);
        TP_HIP(hipGetLastError());
        return;
    }
    for (int ax = 0; ax < 3; ++ax) {
        const double h = c->grid.h[ax];
        const double geom = c->vol / (h * h);
        hipLaunchKernelGGL(k_trans, grid_for(g.nown), dim3(256), 0, c->stream, g, c->K[ax].p, ax, geom, c->TK[ax].p);
    }
    const double h2 = c->grid.h[2];
    hipLaunchKernelGGL(k_trans_halo, grid_for(g.np), dim3(256), 0, c->stream, g, c->K[2].p, c->vol / (h2 * h2),
                       c->TK[2].p);
    TP_HIP(hipGetLastError());
}

void accum_old(tp_ctx *c) {
    const GridDev &g = c->g;
    if (c->satfn)
        hipLaunchKernelGGL(k_accum_old_sat, grid_for(g.nown), dim3(256), 0, c->stream, g, c->dprm, c->u_old.p, c->phi.p,
                           c->acc_old.p, c->dsat);
    else if (c->nph == 2)
        hipLaunchKernelGGL(k_accum_old<2>, grid_for(g.nown), dim3(256), 0, c->stream, g, c->dprm, c->u_old.p,
                           c->phi.p, c->acc_old.p);
    else
        hipLaunchKernelGGL(k_accum_old<1>, grid_for(g.nown), dim3(256), 0, c->stream, g, c->dprm, c->u_old.p,
                           c->phi.p, c->acc_old.p);
    TP_HIP(hipGetLastError());
    wells_rho(c);                                  // the completed wells' head densities follow the old state (nothing without wells)
}

static AsmArgs asm_args(tp_ctx *c) {
    AsmArgs a;
    a.g = c->g; a.q = c->dprm;
    a.u = c->u.p; a.phi = c->phi.p; a.kTs = c->kTs.p;
    for (int ax = 0; ax < 3; ++ax) {
        a.TK[ax] = c->TK[ax].p;
        const double h = c->grid.h[ax];
        a.gam[ax] = (ax == c->grid.gaxis) ? c->prm.g * h * 0.5 : 0.0;
        a.Ga[ax] = c->vol / (h * h);
    }
    a.acc_old = c->acc_old.p;
    a.Vdt = c->vol / c->dt;
    a.R = c->R.p; a.J = c->J.p; a.Sm = c->Sm.p;
    return a;
}

static Spacing spacing_args(tp_ctx *c) {
    Spacing sp;
    for (int ax = 0; ax < 3; ++ax) sp.hs[ax] = c->hs[ax].p;
    sp.inv_dt = 1.0 / c->dt;
    sp.g4 = 0.25 * c->prm.g;
    sp.gaxis = c->grid.gaxis;
    return sp;
}

// ---- saturation functions: host side (tp_set_saturation_functions) -----------------------------------------------------------
tp_satfn satfn_defaults() {
    tp_satfn d;
    d.relperm = 0; d.capillary = 0;
    d.Sr_o = 0.0; d.Sr_w = 0.0; d.n_o = 2.0; d.n_w = 2.0; d.kro_max = 1.0; d.krw_max = 1.0;
    d.lmbda = 2.0; d.p_ct = 0.0; d.pc_se_min = 0.05;
    return d;
}

void satfn_set(tp_ctx *c, const tp_satfn *sat) {
    TP_REQUIRE(c, "null argument");
    const char *fn = "tp_set_saturation_functions: ";
    bool on = false;
    if (sat) {
        const tp_satfn &t = *sat;
        if (t.relperm < 0 || t.relperm > 1) throw Error(std::string(fn) + "relperm = " + std::to_string(t.relperm) + ": 0 (linear) or 1 (Corey)");
        if (t.capillary < 0 || t.capillary > 2)
            throw Error(std::string(fn) + "capillary = " + std::to_string(t.capillary) + ": 0 (none), 1 (linear) or 2 (Brooks-Corey)");
        const struct { const char *key; double v; } num[] = {{"Sr_o", t.Sr_o}, {"Sr_w", t.Sr_w}, {"n_o", t.n_o}, {"n_w", t.n_w},
            {"kro_max", t.kro_max}, {"krw_max", t.krw_max}, {"lmbda", t.lmbda}, {"p_ct", t.p_ct}, {"pc_se_min", t.pc_se_min}};
        for (const auto &e : num)
            if (!std::isfinite(e.v)) throw Error(std::string(fn) + e.key + " is not a finite number");
        auto bad = [&](const char *key, double v, const char *want) {
            throw Error(std::string(fn) + key + " = " + std::to_string(v) + ": " + want);
        };
        if (t.Sr_o < 0.0) bad("Sr_o", t.Sr_o, "the residual oil saturation, >= 0");
        if (t.Sr_w < 0.0) bad("Sr_w", t.Sr_w, "the connate water saturation, >= 0");
        if (!(t.Sr_o + t.Sr_w < 1.0)) bad("Sr_o + Sr_w", t.Sr_o + t.Sr_w, "the residual saturations must leave a mobile range, < 1");
        if (t.n_o < 1.0) bad("n_o", t.n_o, "a Corey exponent, >= 1");
        if (t.n_w < 1.0) bad("n_w", t.n_w, "a Corey exponent, >= 1");
        if (!(t.kro_max > 0.0)) bad("kro_max", t.kro_max, "an end-point relative permeability, > 0");
        if (!(t.krw_max > 0.0)) bad("krw_max", t.krw_max, "an end-point relative permeability, > 0");
        if (!(t.lmbda > 0.0)) bad("lmbda", t.lmbda, "the Brooks-Corey pore-size index, > 0");
        if (t.p_ct < 0.0) bad("p_ct", t.p_ct, "the capillary entry pressure in MPa, >= 0");
        if (!(t.pc_se_min > 0.0 && t.pc_se_min <= 1.0)) bad("pc_se_min", t.pc_se_min, "the floor of Se_w in the Brooks-Corey p_c, in (0, 1]");
        on = t.relperm != 0 || t.capillary != 0;
        if (on && c->nph != 2)
            throw Error(std::string(fn) + "relperm = " + std::to_string(t.relperm) + ", capillary = " + std::to_string(t.capillary) +
                        " on a single-phase context: saturation functions need a saturation, which only nphase = 2 has");
    }
    TP_HIP(hipStreamSynchronize(c->stream));       // nothing in flight reads what is replaced
    c->satfn = on;
    c->sat_host = on ? *sat : satfn_defaults();
    if (on) {
        const tp_satfn &t = *sat;
        DevSat &d = c->dsat;
        d.Sr_o = t.Sr_o; d.So_max = 1.0 - t.Sr_w; d.D = 1.0 - t.Sr_o - t.Sr_w; d.invD = 1.0 / d.D;
        d.n_o = t.n_o; d.n_w = t.n_w; d.kro_max = t.kro_max; d.krw_max = t.krw_max;
        d.p_ct = t.p_ct; d.inv_lmbda = 1.0 / t.lmbda; d.pc_se_min = t.pc_se_min;
        d.pc_max = t.p_ct * std::pow(t.pc_se_min, -1.0 / t.lmbda);
        d.kr_kind = t.relperm; d.pc_kind = t.capillary;
    }
    // the old state's accumulation holds water's density at the old setting's p_w: recomputed here, before any assembly
    if (c->have_old) accum_old(c);
    c->jac_ready = false;
    c->pc_ready = false;
}

// ---- graded grid: host side (tp_set_spacing) ---------------------------------------------------------------------------------
void spacing_set(tp_ctx *c, const double *h0, long n0, const double *h1, long n1, const double *h2, long n2) {
    TP_REQUIRE(c, "null argument");
    if (c->grid.nranks > 1 || c->dist || c->comm || c->lgroup)
        throw Error("tp_set_spacing: spacing on a context with a communicator or a slab group (nranks = " +
                    std::to_string(c->grid.nranks) + ") is not implemented: graded grids exist on one slab");
    const double *h[3] = {h0, h1, h2};
    const long n[3] = {n0, n1, n2};
    const int ext[3] = {c->g.n0, c->g.n1, c->g.n2};
    const bool clear = !h0 && !h1 && !h2;
    if (!clear) {
        for (int a = 0; a < 3; ++a) {
            if (!h[a]) throw Error("tp_set_spacing: null widths for axis " + std::to_string(a) + ": three arrays, or three nulls for a uniform grid");
            if (n[a] != ext[a])
                throw Error("tp_set_spacing: " + std::to_string(n[a]) + " widths for axis " + std::to_string(a) + " but the grid has " +
                            std::to_string(ext[a]) + " cells along it");
            for (long i = 0; i < n[a]; ++i)
                if (!std::isfinite(h[a][i]) || !(h[a][i] > 0.0))
                    throw Error("tp_set_spacing: width " + std::to_string(i) + " of axis " + std::to_string(a) + " is not a positive finite number");
        }
    }
    TP_HIP(hipStreamSynchronize(c->stream));       // nothing in flight reads what is replaced
    for (int a = 0; a < 3; ++a) {
        if (clear) { c->hs_host[a].clear(); c->hs[a].free(); continue; }
        c->hs_host[a].assign(h[a], h[a] + n[a]);
        c->hs[a].alloc(n[a]);
        copy_sync(c, c->hs[a].p, h[a], sizeof(double) * n[a], hipMemcpyHostToDevice);
    }
    c->graded = !clear;
    c->fields_ready = false;                       // T^K of the interior and of the sides follow the widths: tp_finalize_fields
}

void conduction_strengths(const tp_ctx *c, const GridDev &gam, double sg[3]) {
    const int n[3] = {gam.n0, gam.n1, gam.n2};
    for (int a = 0; a < 3; ++a) {
        if (!c->graded) {
            const double hh = c->grid.h[a];
            sg[a] = n[a] > 1 ? c->vol / (hh * hh) : 0.0;
            continue;
        }
        sg[a] = 0.0;
        if (n[a] <= 1) continue;
        double area = 1.0;                         // mean face area: the product of the other two axes' mean widths
        for (int o = 0; o < 3; ++o) {
            if (o == a) continue;
            double sum = 0.0;
            for (double w : c->hs_host[o]) sum += w;
            area *= sum / (double)c->hs_host[o].size();
        }
        const std::vector<double> &w = c->hs_host[a];
        double inv = 0.0;                          // mean of 1/(d_P + d_M) over the interior faces
        for (size_t i = 0; i + 1 < w.size(); ++i) inv += 1.0 / (0.5 * (w[i] + w[i + 1]));
        sg[a] = area * inv / (double)(w.size() - 1);
    }
}

// ---- Dirichlet sides: host side ------------------------------------------------------------------------------------------
static long bc_side_faces(const GridDev &g, int side) {
    const int ax = side >> 1;
    return ax == 0 ? (long)g.n1 * g.n2 : (ax == 1 ? (long)g.n0 * g.n2 : (long)g.n0 * g.n1);
}

static void bc_trans_side(tp_ctx *c, int side) {
    BcSide &s = c->bc.side[side];
    if (s.kind == 0) return;
    const int ax = side >> 1;
    const double h = c->grid.h[ax];
    if (c->graded)
        hipLaunchKernelGGL(k_bc_trans_g, grid_for(s.nf), dim3(256), 0, c->stream, c->g, c->K[ax].p, side, s.kind == 1 ? 1 : 0,
                           c->hs[0].p, c->hs[1].p, c->hs[2].p, s.nf, s.tk.p);
    else
        hipLaunchKernelGGL(k_bc_trans, grid_for(s.nf), dim3(256), 0, c->stream, c->g, c->K[ax].p, side, s.kind == 1 ? 1 : 0,
                           c->vol / (h * h), s.nf, s.tk.p);
    TP_HIP(hipGetLastError());
}

void bc_trans(tp_ctx *c) {
    for (int side = 0; side < 6; ++side) bc_trans_side(c, side);
}

// the sorted list of the cells that lie on a set side
static void bc_rebuild_cells(tp_ctx *c) {
    const GridDev &g = c->g;
    std::vector<int> cells;
    for (int side = 0; side < 6; ++side) {
        if (c->bc.side[side].kind == 0) continue;
        const int ax = side >> 1, dir = side & 1;
        const int ext[3] = {g.n0, g.n1, g.n2};
        int lo[3] = {0, 0, 0}, hi[3] = {g.n0, g.n1, g.n2};
        lo[ax] = dir ? ext[ax] - 1 : 0;
        hi[ax] = lo[ax] + 1;
        for (int i2 = lo[2]; i2 < hi[2]; ++i2)
            for (int i1 = lo[1]; i1 < hi[1]; ++i1)
                for (int i0 = lo[0]; i0 < hi[0]; ++i0) cells.push_back((int)(i0 + (long)g.n0 * i1 + g.np * i2));
    }
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    c->bc.ncells = (int)cells.size();
    c->bc.cells.free();
    if (!cells.empty()) {
        c->bc.cells.alloc(cells.size());
        copy_sync(c, c->bc.cells.p, cells.data(), sizeof(int) * cells.size(), hipMemcpyHostToDevice);
    }
}

void bc_set(tp_ctx *c, int side, int kind, const double *values, long nfaces) {
    TP_REQUIRE(c, "null argument");
    if (c->grid.nranks > 1 || c->dist)
        throw Error("tp_set_boundary: a boundary with nranks = " + std::to_string(c->grid.nranks) +
                    " is not implemented: Dirichlet sides exist on one slab");
    TP_REQUIRE(c->fields_ready, "tp_set_boundary: fields not finalised (tp_finalize_fields)");
    if (side < 0 || side > 5) throw Error("tp_set_boundary: side = " + std::to_string(side) + ": 2*axis + d in 0..5");
    if (kind < 0 || kind > 2) throw Error("tp_set_boundary: kind = " + std::to_string(kind) + ": 0 (none), 1 (open) or 2 (thermal)");
    TP_HIP(hipStreamSynchronize(c->stream));       // nothing in flight reads what is replaced
    BcSide &s = c->bc.side[side];
    if (kind == 0) {
        const bool was = s.kind != 0;
        s.kind = 0; s.nf = 0;
        s.val.free(); s.tk.free(); s.flux.free();
        if (was) bc_rebuild_cells(c);
        return;
    }
    const long nf = bc_side_faces(c->g, side);
    if (nfaces != nf)
        throw Error("tp_set_boundary: nfaces = " + std::to_string(nfaces) + " but side " + std::to_string(side) + " of this grid has " +
                    std::to_string(nf) + " faces");
    TP_REQUIRE(values, "tp_set_boundary: null values");
    const long nv = (long)c->b * nf;
    for (long i = 0; i < nv; ++i)
        if (!std::isfinite(values[i])) throw Error("tp_set_boundary: non-finite ghost value at entry " + std::to_string(i));
    if (c->nph == 2)
        for (long i = 2 * nf; i < nv; ++i)
            if (values[i] < 0.0 || values[i] > 1.0)
                throw Error("tp_set_boundary: ghost saturation S_b outside [0, 1] at face " + std::to_string(i - 2 * nf));
    const bool was = s.kind != 0;
    if (!was) { s.val.alloc(nv); s.tk.alloc(nf); s.flux.alloc(nv); }
    else TP_HIP(hipMemsetAsync(s.flux.p, 0, sizeof(double) * nv, c->stream));   // (no assembly has seen these values yet)
    s.kind = kind; s.nf = nf;
    copy_sync(c, s.val.p, values, sizeof(double) * nv, hipMemcpyHostToDevice);
    bc_trans_side(c, side);
    TP_HIP(hipStreamSynchronize(c->stream));
    if (!was) bc_rebuild_cells(c);
}

void assemble_bc(tp_ctx *c, bool want_jac, bool want_schur) {
    if (c->bc.ncells == 0) return;
    TP_REQUIRE(c->fields_ready, "fields not finalised (tp_finalize_fields)");
    TP_REQUIRE(c->have_old && c->dt > 0.0, "old state / dt not set");
    BcArgs s;
    s.a = asm_args(c);
    s.cells = c->bc.cells.p;
    s.ncells = c->bc.ncells;
    for (int i = 0; i < 6; ++i) {
        const BcSide &b = c->bc.side[i];
        s.kind[i] = b.kind; s.val[i] = b.val.p; s.tk[i] = b.tk.p; s.flux[i] = b.flux.p; s.nf[i] = b.nf;
    }
    if (want_schur) TP_REQUIRE(c->Sm.p, "S~ storage not allocated");
    const dim3 gr = grid_for(s.ncells), bl(256);
    BcArgsG sg;
    if (c->graded) { sg.s = s; sg.sp = spacing_args(c); }
#define LAUNCH_BC(NPH, JAC, SCH)                                                                                         \
    do {                                                                                                                 \
        if (c->graded) hipLaunchKernelGGL((k_assemble_bc<NPH, JAC, SCH, true>), gr, bl, 0, c->stream, sg);                \
        else hipLaunchKernelGGL((k_assemble_bc<NPH, JAC, SCH>), gr, bl, 0, c->stream, s);                                 \
    } while (0)
#define LAUNCH_BC_SAT(JAC, SCH)                                                                                          \
    do {                                                                                                                 \
        if (c->graded) hipLaunchKernelGGL((k_assemble_bc<2, JAC, SCH, true, true>), gr, bl, 0, c->stream,                 \
                                          WithSat<BcArgsG>{sg, c->dsat});                                                \
        else hipLaunchKernelGGL((k_assemble_bc<2, JAC, SCH, false, true>), gr, bl, 0, c->stream, WithSat<BcArgs>{s, c->dsat}); \
    } while (0)
    if (c->satfn) {
        if (!want_jac) LAUNCH_BC_SAT(false, false);
        else if (want_schur) LAUNCH_BC_SAT(true, true);
        else LAUNCH_BC_SAT(true, false);
    } else if (c->nph == 2) {
        if (!want_jac) LAUNCH_BC(2, false, false);
        else if (want_schur) LAUNCH_BC(2, true, true);
        else LAUNCH_BC(2, true, false);
    } else {
        if (!want_jac) LAUNCH_BC(1, false, false);
        else if (want_schur) LAUNCH_BC(1, true, true);
        else LAUNCH_BC(1, true, false);
    }
#undef LAUNCH_BC
#undef LAUNCH_BC_SAT
    TP_HIP(hipGetLastError());
}

// out[side*b + r]: what the faces of `side` added to equation r of R at the last assembly, summed in face order on the host
void bc_flux(tp_ctx *c, double *out) {
    const int b = c->b;
    for (int i = 0; i < 6 * b; ++i) out[i] = 0.0;
    TP_HIP(hipStreamSynchronize(c->stream));
    std::vector<double> h;
    for (int side = 0; side < 6; ++side) {
        const BcSide &s = c->bc.side[side];
        if (s.kind == 0) continue;
        h.resize((size_t)b * s.nf);
        copy_sync(c, h.data(), s.flux.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost);
        for (int r = 0; r < b; ++r) {
            double acc = 0.0;
            for (long f = 0; f < s.nf; ++f) acc += h[(size_t)r * s.nf + f];
            out[side * b + r] = acc;
        }
    }
}

void assemble(tp_ctx *c, bool want_jac, bool want_schur) {
    TP_REQUIRE(c->fields_ready, "fields not finalised (tp_finalize_fields)");
    TP_REQUIRE(c->have_old && c->dt > 0.0, "old state / dt not set");
    const GridDev &g = c->g;
    const AsmArgs a = asm_args(c);
    if (want_schur) TP_REQUIRE(c->Sm.p, "S~ storage not allocated");
    const dim3 gr = xcd_grid(g.nown), bl(256);
    static const bool lds_tiled = tp_switch_flag(TP_SW_ASM_LDS);
    const dim3 grl((g.n0 + ATX - 1) / ATX, (g.n1 + ATY - 1) / ATY, (g.n2 + ATZ - 1) / ATZ);
    // a context with spacing always launches the plain graded kernel (the LDS-tiled variant has no graded twin)
    AsmArgsG ag;
    if (c->graded) { ag.a = a; ag.sp = spacing_args(c); }
#define LAUNCH(NPH, JAC, SCH)                                                                                            \
    do {                                                                                                                 \
        if (c->graded) hipLaunchKernelGGL((k_assemble<NPH, JAC, SCH, true>), gr, bl, 0, c->stream, ag);                   \
        else if (lds_tiled) {                                                                                            \
            const size_t bytes = (size_t)PropsLds<NPH>::NV * ANS * sizeof(double);                                        \
            TP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_assemble_lds<NPH, JAC, SCH>),                    \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));                         \
            hipLaunchKernelGGL((k_assemble_lds<NPH, JAC, SCH>), grl, bl, bytes, c->stream, a);                            \
        } else hipLaunchKernelGGL((k_assemble<NPH, JAC, SCH>), gr, bl, 0, c->stream, a);                                 \
    } while (0)
    // a context with saturation functions launches the plain kernel too (the LDS image holds no p_c)
#define LAUNCH_SAT(JAC, SCH)                                                                                             \
    do {                                                                                                                 \
        if (c->graded) hipLaunchKernelGGL((k_assemble<2, JAC, SCH, true, true>), gr, bl, 0, c->stream,                    \
                                          WithSat<AsmArgsG>{ag, c->dsat});                                               \
        else hipLaunchKernelGGL((k_assemble<2, JAC, SCH, false, true>), gr, bl, 0, c->stream, WithSat<AsmArgs>{a, c->dsat}); \
    } while (0)
    if (c->satfn) {
        if (!want_jac) LAUNCH_SAT(false, false);
        else if (want_schur) LAUNCH_SAT(true, true);
        else LAUNCH_SAT(true, false);
    } else if (c->nph == 2) {
        if (!want_jac) LAUNCH(2, false, false);
        else if (want_schur) LAUNCH(2, true, true);
        else LAUNCH(2, true, false);
    } else {
        if (!want_jac) LAUNCH(1, false, false);
        else if (want_schur) LAUNCH(1, true, true);
        else LAUNCH(1, true, false);
    }
#undef LAUNCH
#undef LAUNCH_SAT
    if (c->bc.ncells > 0) assemble_bc(c, want_jac, want_jac && want_schur);
    if (c->nsrc_groups > 0) {
        double *J = want_jac ? c->J.p : nullptr;
        double *Sm = (want_jac && want_schur) ? c->Sm.p : nullptr;
        const dim3 g2 = grid_for(c->nsrc_groups, 64);
        if (c->satfn)
            hipLaunchKernelGGL(k_sources_sat, g2, dim3(64), 0, c->stream, g, c->dprm, c->src.p, c->src_start.p,
                               c->nsrc_groups, c->u.p, c->R.p, J, Sm, (double *)nullptr, c->nsrc, c->dsat);
        else if (c->nph == 2)
            hipLaunchKernelGGL(k_sources<2>, g2, dim3(64), 0, c->stream, g, c->dprm, c->src.p, c->src_start.p,
                               c->nsrc_groups, c->u.p, c->R.p, J, Sm, (double *)nullptr, c->nsrc);
        else
            hipLaunchKernelGGL(k_sources<1>, g2, dim3(64), 0, c->stream, g, c->dprm, c->src.p, c->src_start.p,
                               c->nsrc_groups, c->u.p, c->R.p, J, Sm, (double *)nullptr, c->nsrc);
    }
    TP_HIP(hipGetLastError());
    if (c->wells.nw > 0) wells_assemble(c, want_jac, want_schur);
    if (want_jac) c->jac_ready = true;
}

void well_rates(tp_ctx *c) {
    if (c->nsrc_groups == 0) return;
    const dim3 g2 = grid_for(c->nsrc_groups, 64);
    if (c->satfn)
        hipLaunchKernelGGL(k_sources_sat, g2, dim3(64), 0, c->stream, c->g, c->dprm, c->src.p, c->src_start.p,
                           c->nsrc_groups, c->u.p, (double *)nullptr, (double *)nullptr, (double *)nullptr,
                           c->rates.p, c->nsrc, c->dsat);
    else if (c->nph == 2)
        hipLaunchKernelGGL(k_sources<2>, g2, dim3(64), 0, c->stream, c->g, c->dprm, c->src.p, c->src_start.p,
                           c->nsrc_groups, c->u.p, (double *)nullptr, (double *)nullptr, (double *)nullptr,
                           c->rates.p, c->nsrc);
    else
        hipLaunchKernelGGL(k_sources<1>, g2, dim3(64), 0, c->stream, c->g, c->dprm, c->src.p, c->src_start.p,
                           c->nsrc_groups, c->u.p, (double *)nullptr, (double *)nullptr, (double *)nullptr,
                           c->rates.p, c->nsrc);
    TP_HIP(hipGetLastError());
}

}  // namespace tp
