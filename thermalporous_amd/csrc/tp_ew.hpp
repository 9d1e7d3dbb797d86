// Eisenstat-Walker forcing terms (tp_options.ksp_ew; snes_ksp_ew): the relative tolerance of the k-th linear
// solve of one Newton solve, chosen from the nonlinear residual norms.  Plain C++: no HIP, no context -- newton() in
// tp_solver.hip and the export tp_ew_next_rtol call the same function.
//
//   ||F_k||  residual norm at the iterate where system k is formed       rho_k  residual norm the Krylov solver returned for it
//   eta_k    tolerance of solve k: it stops at max(eta_k ||F_k||, ksp_atol)
//
//   k == 0:     eta = rtol0
//   version 1:  eta = | ||F_k|| - rho_{k-1} | / ||F_{k-1}|| ;         s = pow(eta_{k-1}, alpha2)
//   version 2:  eta = gamma pow(||F_k|| / ||F_{k-1}||, alpha) ;       s = gamma pow(eta_{k-1}, alpha)
//   k > 0:      if s > threshold: eta = max(eta, s)                   (safeguard: no sudden tightening after a loose solve)
//   always:     eta = min(eta, rtolmax); eta = max(eta, ksp_rtol)     (cap, then floor)
//
// These are PETSc's formulas and defaults (SNESKSPSetParametersEW) with ONE deliberate difference: the configured ksp_rtol stays
// as a floor, where PETSc overwrites it.  The two differ only where the formula asks for more digits than the user ever wanted.
// Written operation by operation as tests/ew_ref.py:next_rtol is: same inputs, same bits (both call libm's pow).
#ifndef TP_EW_HPP
#define TP_EW_HPP

#include <cmath>
#include <stdexcept>
#include <string>
#include "../../include/thermalporous_hip.h"

namespace tp {

// which branches one choice took (flags of ew_next_rtol)
constexpr int EW_FIRST = 1;            // k == 0: rtol0
constexpr int EW_SAFE_TESTED = 2;      // s > threshold: the safeguard was consulted
constexpr int EW_SAFE_RAISED = 4;      // ... and raised eta
constexpr int EW_CAPPED = 8;           // eta cut to rtolmax
constexpr int EW_FLOORED = 16;         // eta raised to ksp_rtol

inline double ew_default_alpha() { return (1.0 + std::sqrt(5.0)) / 2.0; }

inline void ew_require(bool ok, const char *msg) {
    if (!ok) throw std::runtime_error(msg);
}

inline void ew_check_options(const tp_options &o) {
    ew_require(o.ksp_ew != 3, "ksp_ew 3 (snes_ksp_ew_version 3) is not implemented: it needs the line search's predicted and actual reduction");
    ew_require(o.ksp_ew >= 0 && o.ksp_ew <= 2, "ksp_ew must be 0 (off), 1 or 2 (the Eisenstat-Walker version)");
    if (o.ksp_ew == 0) {
        // the ew fields at their defaults (or zeroed, as a C caller that never heard of them leaves them): refused, never ignored
        const double a = ew_default_alpha();
        ew_require(o.ew_rtol0 == 0.0 || o.ew_rtol0 == 0.3, "ew_rtol0 is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        ew_require(o.ew_rtolmax == 0.0 || o.ew_rtolmax == 0.9, "ew_rtolmax is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        ew_require(o.ew_gamma == 0.0 || o.ew_gamma == 1.0, "ew_gamma is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        ew_require(o.ew_alpha == 0.0 || o.ew_alpha == a, "ew_alpha is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        ew_require(o.ew_alpha2 == 0.0 || o.ew_alpha2 == a, "ew_alpha2 is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        ew_require(o.ew_threshold == 0.0 || o.ew_threshold == 0.1, "ew_threshold is set but ksp_ew is 0 (off): the field belongs to Eisenstat-Walker");
        return;
    }
    ew_require(o.ew_rtol0 >= 0.0 && o.ew_rtol0 < 1.0, "ew_rtol0 must lie in [0, 1)");
    ew_require(o.ew_rtolmax >= 0.0 && o.ew_rtolmax < 1.0, "ew_rtolmax must lie in [0, 1)");
    ew_require(o.ew_gamma >= 0.0 && o.ew_gamma <= 1.0, "ew_gamma must lie in [0, 1]");
    ew_require(o.ew_alpha > 1.0 && o.ew_alpha <= 2.0, "ew_alpha must lie in (1, 2]");
    ew_require(o.ew_alpha2 > 1.0 && o.ew_alpha2 <= 2.0, "ew_alpha2 must lie in (1, 2]");
    ew_require(o.ew_threshold > 0.0 && o.ew_threshold < 1.0, "ew_threshold must lie in (0, 1)");
    ew_require(o.ksp_rtol <= o.ew_rtolmax, "ksp_rtol exceeds ew_rtolmax: the floor of the Eisenstat-Walker tolerance would lie above its cap");
}

// eta_k.  fnorm_last, lresid_last, rtol_last are not read for k == 0.  *flags (optional): the EW_* branches taken.
inline double ew_next_rtol(const tp_options &o, int k, double fnorm, double fnorm_last, double lresid_last, double rtol_last,
                           int *flags = nullptr) {
    int fl = 0;
    double eta;
    if (k == 0) {
        eta = o.ew_rtol0;
        fl |= EW_FIRST;
    } else {
        double s;
        if (o.ksp_ew == 1) {
            eta = std::fabs(fnorm - lresid_last) / fnorm_last;
            s = std::pow(rtol_last, o.ew_alpha2);
        } else {
            eta = o.ew_gamma * std::pow(fnorm / fnorm_last, o.ew_alpha);
            s = o.ew_gamma * std::pow(rtol_last, o.ew_alpha);
        }
        if (s > o.ew_threshold) {
            fl |= EW_SAFE_TESTED;
            if (s > eta) { eta = s; fl |= EW_SAFE_RAISED; }
        }
    }
    if (!(eta <= o.ew_rtolmax)) { eta = o.ew_rtolmax; fl |= EW_CAPPED; }       // (also catches a NaN)
    if (eta < o.ksp_rtol) { eta = o.ksp_rtol; fl |= EW_FLOORED; }
    if (flags) *flags = fl;
    return eta;
}

}  // namespace tp
#endif
