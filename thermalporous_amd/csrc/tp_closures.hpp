// Device closure laws with analytic derivatives -- restates
// /root/reference/thermalporous/physicalparameters.py:37-57 (oil), :69-90 (water) for gfx950.
// Quirks preserved: water_* use 272.15 (not 273.15) as the Celsius offset (:80,:89).
#pragma once
#include "tp_common.hpp"

namespace tp {

// oil_rho = rho_ref * e^(c(10p - p0)) * e^(-e1 (T - T0))            (:37-46)
// (in two halves: r is the PRODUCT of the two factors, and where r goes straight into a sum the compiler contracts that
// product into the sum.  k_assemble_lds keeps the factors in its LDS image and forms r where it is used, like k_assemble.)
__device__ __forceinline__ void oil_rho_factors(double p, double T, const DevPrm &q, double &f1, double &f2) {
    constexpr double c = 5.5e-5, p0 = 1.01325, e1 = 2.5e-4, T0 = 15.5556 + 273.15;
    f1 = q.rho_ref * exp(c * (p * 1e1 - p0));
    f2 = exp(-e1 * (T - T0));
}
__device__ __forceinline__ void oil_rho_from(double f1, double f2, double &r, double &r_p, double &r_T) {
    constexpr double c = 5.5e-5, e1 = 2.5e-4;
    r = f1 * f2;
    r_p = (10.0 * c) * r;
    r_T = (-e1) * r;
}
__device__ __forceinline__ void oil_rho(double p, double T, const DevPrm &q, double &r, double &r_p, double &r_T) {
    double f1, f2;
    oil_rho_factors(p, T, q, f1, f2);
    oil_rho_from(f1, f2, r, r_p, r_T);
}

// oil_mu = 1e-3 * 10^(A1 API + A2) * Tf^(A3 API + A4), Tf = 1.8 (T - 273.15) + 32     (:48-57)
__device__ __forceinline__ void oil_mu(double T, const DevPrm &q, double &mu, double &mu_T) {
    const double Tf = 1.8 * (T - 273.15) + 32.0;
    mu = q.mu_o_coef * pow(Tf, q.mu_o_exp);
    mu_T = mu * q.mu_o_exp * 1.8 / Tf;
}

// water_rho: Trangenstein's modification of Kell's correlation         (:69-82)
__device__ __forceinline__ void water_rho(double p, double T, double &r, double &r_p, double &r_T) {
    constexpr double E0 = 999.83952, E1 = 16.955176, E2 = -7.987e-3, E3 = -46.170461e-6, E4 = 105.56302e-9,
                     E5 = -280.54353e-12, E6 = 16.87985e-3, E7 = 10.2, Cw = 3.98854e-4;
    const double Tc = T - 272.15;
    const double P = E0 + Tc * (E1 + Tc * (E2 + Tc * (E3 + Tc * (E4 + Tc * E5))));
    const double dP = E1 + Tc * (2 * E2 + Tc * (3 * E3 + Tc * (4 * E4 + Tc * 5 * E5)));
    const double den = 1.0 + E6 * Tc;
    const double ex = exp(Cw * (p - E7));
    r = P * ex / den;
    r_p = Cw * r;
    r_T = (dP - P * E6 / den) * ex / den;
}

// water_mu: Grabowski                                                   (:84-90)
__device__ __forceinline__ void water_mu(double T, double &mu, double &mu_T) {
    constexpr double Aw = 2.1850, Bw = 0.04012, Cw = 5.1547e-6;
    const double Tf = 1.8 * (T - 272.15) + 32.0;
    const double den = -1.0 + Bw * Tf + Cw * Tf * Tf;
    mu = 1e-3 * Aw / den;
    mu_T = -mu * (Bw + 2.0 * Cw * Tf) * 1.8 / den;
}

// ---- forward-mode dual number with three partials (p, T, S): used only by the well kernel ----------
struct Dual3 {
    double v;
    double d[3];
    __host__ __device__ Dual3() : v(0.0) { d[0] = d[1] = d[2] = 0.0; }
    __host__ __device__ explicit Dual3(double x) : v(x) { d[0] = d[1] = d[2] = 0.0; }
    __host__ __device__ Dual3(double x, int k) : v(x) { d[0] = d[1] = d[2] = 0.0; d[k] = 1.0; }
};
__host__ __device__ inline Dual3 operator+(const Dual3 &a, const Dual3 &b) {
    Dual3 r; r.v = a.v + b.v; for (int k = 0; k < 3; ++k) r.d[k] = a.d[k] + b.d[k]; return r;
}
__host__ __device__ inline Dual3 operator-(const Dual3 &a, const Dual3 &b) {
    Dual3 r; r.v = a.v - b.v; for (int k = 0; k < 3; ++k) r.d[k] = a.d[k] - b.d[k]; return r;
}
__host__ __device__ inline Dual3 operator*(const Dual3 &a, const Dual3 &b) {
    Dual3 r; r.v = a.v * b.v; for (int k = 0; k < 3; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k]; return r;
}
__host__ __device__ inline Dual3 operator*(const Dual3 &a, double s) {
    Dual3 r; r.v = a.v * s; for (int k = 0; k < 3; ++k) r.d[k] = a.d[k] * s; return r;
}
__host__ __device__ inline Dual3 operator/(const Dual3 &a, const Dual3 &b) {
    Dual3 r; r.v = a.v / b.v;
    for (int k = 0; k < 3; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
    return r;
}
__host__ __device__ inline Dual3 operator/(const Dual3 &a, double s) { return a * (1.0 / s); }

__device__ inline Dual3 oil_rho_t(const Dual3 &p, const Dual3 &T, const DevPrm &q) {
    double r, rp, rT;
    oil_rho(p.v, T.v, q, r, rp, rT);
    Dual3 o; o.v = r;
    for (int k = 0; k < 3; ++k) o.d[k] = rp * p.d[k] + rT * T.d[k];
    return o;
}
__device__ inline Dual3 oil_mu_t(const Dual3 &T, const DevPrm &q) {
    double m, mT;
    oil_mu(T.v, q, m, mT);
    Dual3 o; o.v = m;
    for (int k = 0; k < 3; ++k) o.d[k] = mT * T.d[k];
    return o;
}
__device__ inline Dual3 water_rho_t(const Dual3 &p, const Dual3 &T) {
    double r, rp, rT;
    water_rho(p.v, T.v, r, rp, rT);
    Dual3 o; o.v = r;
    for (int k = 0; k < 3; ++k) o.d[k] = rp * p.d[k] + rT * T.d[k];
    return o;
}
__device__ inline Dual3 water_mu_t(const Dual3 &T) {
    double m, mT;
    water_mu(T.v, m, mT);
    Dual3 o; o.v = m;
    for (int k = 0; k < 3; ++k) o.d[k] = mT * T.d[k];
    return o;
}

// ---- saturation functions (tp_set_saturation_functions) ---------------------------------------------------------
// kr_o, kr_w and p_c of S_o, written once over the number type: Dual1 (value and d/dS) in the cell kernels, whose derivatives
// w.r.t. p and T are carried by hand, Dual3 in the well kernel.  Every clamp decides on the value and gives a constant (slope
// exactly 0) at and beyond either end: the strict gt of the reference's rel_perm_*_B_C and the tie rule of the upwinding.
struct Dual1 {
    double v, d;
};
__device__ __forceinline__ Dual1 sat_const(const Dual1 &, double c) { return Dual1{c, 0.0}; }
__device__ __forceinline__ Dual3 sat_const(const Dual3 &, double c) { return Dual3(c); }
// the number with value v and the derivative dv times that of x: f(x), f'(x) by the chain rule
__device__ __forceinline__ Dual1 sat_chain(const Dual1 &x, double v, double dv) { return Dual1{v, dv * x.d}; }
__device__ __forceinline__ Dual3 sat_chain(const Dual3 &x, double v, double dv) {
    Dual3 r; r.v = v;
    for (int k = 0; k < 3; ++k) r.d[k] = dv * x.d[k];
    return r;
}
// x^n and n x^(n-1) from one pow; the exponents 1 and 2 (the linear and the common Corey curve) take none.  n is uniform over
// the grid, so no wave diverges here.
template <class N> __device__ __forceinline__ N sat_pow(const N &x, double n) {
    if (n == 1.0) return x;
    if (n == 2.0) return sat_chain(x, x.v * x.v, 2.0 * x.v);
    const double pw = pow(x.v, n - 1.0);
    return sat_chain(x, pw * x.v, n * pw);
}
// effective saturations: the value by a true division (correctly rounded, so the ends lie where the definition puts them)
template <class N> __device__ __forceinline__ N sat_se_o(const N &S, const DevSat &s) { return sat_chain(S, (S.v - s.Sr_o) / s.D, s.invD); }
template <class N> __device__ __forceinline__ N sat_se_w(const N &S, const DevSat &s) { return sat_chain(S, (s.So_max - S.v) / s.D, -s.invD); }

template <class N> __device__ __forceinline__ N sat_corey(const N &Se, double n, double kmax) {
    if (!(Se.v > 0.0)) return sat_const(Se, 0.0);
    if (!(Se.v < 1.0)) return sat_const(Se, kmax);
    const N pw = sat_pow(Se, n);
    return sat_chain(pw, kmax * pw.v, kmax);
}
template <class N> __device__ __forceinline__ N kr_o_t(const N &S, const DevSat &s) {
    if (s.kr_kind == 0) return S;                                    // (:92-94)
    return sat_corey(sat_se_o(S, s), s.n_o, s.kro_max);              // (:124-129, with the clamp at Se > 1)
}
template <class N> __device__ __forceinline__ N kr_w_t(const N &S, const DevSat &s) {
    if (s.kr_kind == 0) return sat_chain(S, 1.0 - S.v, -1.0);        // (:96-98)
    return sat_corey(sat_se_w(S, s), s.n_w, s.krw_max);              // (:131-138)
}
// p_c = p_o - p_w >= 0: linear (:147-152) or Brooks-Corey with Se_w floored at pc_se_min (:140-145)
template <class N> __device__ __forceinline__ N pc_t(const N &S, const DevSat &s) {
    if (s.pc_kind == 0) return sat_const(S, 0.0);
    const N Se = sat_se_w(S, s);
    if (!(Se.v < 1.0)) return sat_const(S, s.pc_kind == 1 ? 0.0 : s.p_ct);
    if (s.pc_kind == 1) {
        if (!(Se.v > 0.0)) return sat_const(S, s.p_ct);
        return sat_chain(Se, s.p_ct * (1.0 - Se.v), -s.p_ct);
    }
    if (!(Se.v > s.pc_se_min)) return sat_const(S, s.pc_max);
    const N pw = sat_pow(Se, -s.inv_lmbda);
    return sat_chain(pw, s.p_ct * pw.v, s.p_ct);
}

}  // namespace tp
