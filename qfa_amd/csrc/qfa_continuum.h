// qfa_continuum.h -- what the kernels that form the pixel of a posterior draw share (include/qfa_hip.h: qfa_forest_f32,
// qfa_mock_spectra_f32, qfa_obs_stack_f32, qfa_bal_scan_f32): the continuum c = mu + F h, the ratio r = flux / c, its inverse
// variance iv = c c / den and the decision use = mask && c > cont_min && isfinite(r) && isfinite(iv).
//
//   load4, store4    four values of the pixels p0 .. p0 + 3 of a row of which `n` exist: one float4 when all four exist and the
//                    address is 16-byte aligned, else scalar (a missing pixel loads as 0 and is not stored).  k_forest, k_mock_spectra
//
// What is NOT here yet, and why.  The loaders of F (a row into f[NHM], an image into f[NHM][4]), the fma chain and the pixel rule
// are still written out in k_forest, k_mock_spectra, k_obs_stack and k_bal_scan: routed through one inlined function each, every
// one of those kernels came out with another register allocation or instruction order (same instructions), and a kernel whose code
// moves needs its bits and its speed measured against its parent first.  The rule has one definition only once the three forms of
// den that the kernels compute TODAY are named in it; they agree to rounding and no more:
//   k_obs_stack   den = fma(sigma, sigma, fl(fl(r r) u2)): r r and its product with u2 are rounded (pinned), sigma sigma is fused
//                 into the sum (outside the pin the compiler contracts __fadd_rn(x, __fmul_rn(..)) whatever `fp contract` says)
//   k_forest      den = fma(fl(T T), u2, fl(sigma sigma)): no pin, the u2 product is fused into the sum
//   k_bal_scan    den = fl(sigma sigma), no u2 term.  Against k_obs_stack with unc = NULL it differs on one input class: r r
//                 overflows while r is finite.  There (r r) 0 is NaN, iv is NaN and the pixel drops out; k_bal_scan keeps it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfa_continuum {

__device__ __forceinline__ void load4(const float *__restrict__ src, int n, float v[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? src[k] : 0.f;
    }
}
__device__ __forceinline__ void store4(float *__restrict__ dst, int n, const float v[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4 *>(dst) = float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) dst[k] = v[k];
    }
}

}  // namespace qfa_continuum
