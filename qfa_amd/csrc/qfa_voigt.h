// qfa_voigt.h -- the Voigt profile of the absorber rule (include/qfa_hip.h, qfa_absorber_mask_f32: "profile") in float64: the line
// constants of Ly-alpha and Ly-beta and the Tepper-Garcia form of H(a, x) with its small-P series and its far wing.  One definition
// for k_absorber (qfa_absorber.h: catalogued absorbers) and k_dla_profiles (qfa_dla.h: the template table of the DLA scan).
#pragma once
#include <hip/hip_runtime.h>

namespace qfa_voigt {

constexpr double kC = 299792.458;               // km/s
constexpr double kTauCoef = 1.497e-15;
constexpr double kPSeries = 0.0625, kPWing = 750.0;
constexpr double kFourPi = 12.566370614359172, kSqrtPi = 1.7724538509055159;
// lam0 (Angstrom), oscillator strength, damping constant (1/s) of Ly-alpha and Ly-beta
__device__ constexpr double kLam0[2] = {1215.67, 1025.72};
__device__ constexpr double kOsc[2] = {0.4164, 0.07912};
__device__ constexpr double kGamma[2] = {6.265e8, 1.897e8};

// tau of one line at one pixel from 1 / P (wing: a whole wave beyond kPWing, no exp)
__device__ __forceinline__ double h_wing(double ka, double rP) { return ka * rP * (1.0 + 1.5 * rP); }

__device__ __forceinline__ double h_full(double ka, double P, double rP) {
    const double H0 = exp(-P), Q = 1.5 * rP;
    const double full = H0 - ka * rP * (H0 * H0 * (4.0 * P * P + 7.0 * P + 4.0 + Q) - Q - 1.0);
    double g = 2584.0 / 155925.0;
    g = g * P + -884.0 / 14175.0;
    g = g * P + 38.0 / 189.0;
    g = g * P + -169.0 / 315.0;
    g = g * P + 352.0 / 315.0;
    g = g * P + -8.0 / 5.0;
    g = g * P + 14.0 / 15.0;
    g = g * P + 5.0 / 3.0;
    g = g * P + -4.0;
    g = g * P + 2.0;
    const double series = H0 - ka * g;
    const double wing = h_wing(ka, rP);
    return P < kPSeries ? series : (P > kPWing ? wing : full);
}

// the per-line constants: tau coefficient 1.497e-15 10^logNHI f lam0 / b and ka = a / sqrt(pi)
__device__ __forceinline__ double tau_coef(double lognhi, int l, double b_kms) { return kTauCoef * exp10(lognhi) * kOsc[l] * kLam0[l] / b_kms; }
__device__ __forceinline__ double line_ka(int l, double b_kms) { return kGamma[l] * kLam0[l] * 1e-13 / (kFourPi * b_kms) / kSqrtPi; }

}  // namespace qfa_voigt
