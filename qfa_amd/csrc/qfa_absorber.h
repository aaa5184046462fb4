// qfa_absorber.h -- catalogued absorbers (DLA Voigt profiles) and bad-wavelength intervals on the (N, Npix) rest-frame arrays: mask,
// correct and the catalogue's counts (include/qfa_hip.h, qfa_absorber_mask_f32, states the rule).  Built in qfa_absorber.hip.
//
//   k_absorber   one workgroup of kThreads = 256 per spectrum, grid-stride over the spectra, so the record needs no atomics.  Thread
//                t owns the pixels k = t, t + 256, .. (at most 64 passes: Npix <= 16 384): the lanes of a wave own neighbouring pixels
//                and a wave owns one 64-bit word of the validity bitmap per pass.
//     lines      the spectrum's absorber list is block-uniform.  Per absorber line the constants 1 / (lam0 (1 + z_a)), the tau
//                coefficient 1.497e-15 10^logNHI f lam0 / b and ka = a / sqrt(pi) are derived once per block (one thread per line: a
//                division and an exp10) into an LDS tile of kTileAbs = 16 absorbers (32 lines, 768 bytes).  A spectrum with more
//                absorbers walks its tiles inside every pass, tau staying in the pixel's register; with at most one tile the tile
//                is staged once in front of the passes.
//     profile    per pixel and line: x by one fma, P = x x, one division 1 / P.  The far wing (P > 750: exp(-P) = 0) is taken by a
//                whole wave on one ballot: H = (ka / P) (1 + 1.5 / P), a division and four multiply-adds, no exp -- the value the
//                full form gives there, so the choice of branch changes no bit.  Otherwise exp(-P), the full form and the
//                small-P series, dealt by selects.  One exp(-tau) behind the lines.
//     intervals  observed-frame and rest-frame intervals are block-uniform lists read through uniform (scalar) loads.
//     sums       the S/N sum and the three counts: per thread in order of k, a butterfly over the wave, lane 0 to LDS, the four wave
//                sums in wave order: one fixed tree.  Runs: wave 0 walks the bitmap as k_preprocess does.
//   A spectrum with no absorbers and no intervals is a copy plus the record: 8 bytes read, 8 written per pixel (wav_grid stays in
//   L2), 4 more with trans_out.  LDS: 768 + 2 048 + 4 x 8 + 4 x 3 x 4 bytes, static.  No scratch, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qfa_hip.h"
#include "qfa_voigt.h"

namespace qfa_absorber {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxNpix = 16384;
constexpr int kWords = kMaxNpix / 64;
constexpr int kTileAbs = 16;                    // absorbers per LDS tile
constexpr int kTileLines = 2 * kTileAbs;

using namespace qfa_voigt;                      // the line constants, h_wing and h_full (qfa_voigt.h)

struct Args {
    const float *flux, *error;                  // (N, Npix); may alias the outputs: no __restrict__ on the four
    const double *zqso, *grid;
    const int64_t *abs_off;                     // (N + 1) or NULL
    const double *abs_z, *abs_lognhi;
    const double *obs;                          // (n_obs, 2) or NULL
    const int64_t *rest_off;                    // (N + 1) or NULL
    const double *rest;                         // (., 2)
    float *flux_out, *error_out, *trans_out;    // trans_out may be NULL
    double *rec_f64;                            // (N, 1) snr
    int32_t *rec_i32;                           // (N, 6)
    int64_t N;
    int Npix, n_obs, lyb, correct;
    double t_min, b_kms, snr_lo, snr_hi;
};

__device__ __forceinline__ double wave_sum(double x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = __dadd_rn(x, __shfl(x, lane ^ d));
    return x;
}
__device__ __forceinline__ int wave_isum(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += __shfl(x, lane ^ d);
    return x;
}

__global__ __launch_bounds__(kThreads) void k_absorber(const Args a) {
    __shared__ double s_r[kTileLines], s_c[kTileLines], s_ka[kTileLines];         // 1 / (lam0 (1 + z_a)), tau coefficient, a / sqrt(pi)
    __shared__ unsigned long long s_bits[kWords];
    __shared__ double s_sum[kWaves];
    __shared__ int s_cnt[kWaves][3];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int Npix = a.Npix, nwords = (Npix + 63) >> 6, npass = (Npix + kThreads - 1) / kThreads;
    const int nl = a.lyb ? 2 : 1;                                                 // lines per absorber
    const double cb = kC / a.b_kms;
    for (int64_t s = blockIdx.x; s < a.N; s += gridDim.x) {
        const double zp1 = 1.0 + a.zqso[s];
        const int64_t a0 = a.abs_off ? a.abs_off[s] : 0;
        const int64_t na64 = a.abs_off ? a.abs_off[s + 1] - a0 : 0;
        const int64_t na = na64 > 0 ? na64 : 0;
        const int64_t r0 = a.rest_off ? a.rest_off[s] : 0;
        const int64_t nr64 = a.rest_off ? a.rest_off[s + 1] - r0 : 0;
        const int64_t nr = nr64 > 0 ? nr64 : 0;
        const bool one_tile = na <= kTileAbs;
        const float *fin = a.flux + s * (int64_t)Npix;
        const float *ein = a.error + s * (int64_t)Npix;
        float *fo = a.flux_out + s * (int64_t)Npix;
        float *eo = a.error_out + s * (int64_t)Npix;
        float *to = a.trans_out ? a.trans_out + s * (int64_t)Npix : nullptr;

        double ps = 0.0;
        int cs = 0, cabs = 0, cint = 0;
#pragma unroll 1
        for (int i = 0; i < npass; ++i) {                                         // (block-uniform: the tiles are staged behind barriers)
            const int k = i * kThreads + tid;
            const int kc = k < Npix ? k : Npix - 1;                               // lanes past the end follow the last pixel
            const double g = a.grid[kc];
            const double lam = __dmul_rn(g, zp1);
            double tau = 0.0;
#pragma unroll 1
            for (int64_t t0 = 0; t0 < na; t0 += kTileAbs) {
                const int nt = (int)((na - t0 < kTileAbs ? na - t0 : kTileAbs)) * nl;     // lines of this tile
                if (!one_tile || i == 0) {
                    __syncthreads();                                              // the tile before it is read no more
                    if (tid < nt) {
                        const int j = tid / nl, l = tid - j * nl;
                        const double za = a.abs_z[a0 + t0 + j], lg = a.abs_lognhi[a0 + t0 + j];
                        s_r[tid] = 1.0 / (kLam0[l] * (1.0 + za));
                        s_c[tid] = kTauCoef * exp10(lg) * kOsc[l] * kLam0[l] / a.b_kms;
                        s_ka[tid] = kGamma[l] * kLam0[l] * 1e-13 / (kFourPi * a.b_kms) / kSqrtPi;
                    }
                    __syncthreads();
                }
#pragma unroll 1
                for (int q = 0; q < nt; ++q) {
                    const double x = cb * fma(lam, s_r[q], -1.0);
                    const double P = x * x, rP = 1.0 / P, ka = s_ka[q];
                    const bool far = P > kPWing;
                    double H;
                    if (__ballot(far) == __ballot(true)) H = h_wing(ka, rP);      // (wave-uniform)
                    else H = h_full(ka, P, rP);
                    tau += s_c[q] * H;
                }
            }
            const double T = exp(-tau);
            const float f = k < Npix ? fin[k] : -999.0f, e = k < Npix ? ein[k] : -999.0f;   // (read before this pixel's stores: in place is allowed)
            const bool valid_in = k < Npix && f != -999.0f && e != -999.0f;
            const bool m_abs = !(T >= a.t_min) || !isfinite(T);
            bool m_int = false;
            for (int q = 0; q < a.n_obs; ++q) m_int |= lam >= a.obs[2 * q] && lam < a.obs[2 * q + 1];
            for (int64_t q = 0; q < nr; ++q) m_int |= g >= a.rest[2 * (r0 + q)] && g < a.rest[2 * (r0 + q) + 1];
            const bool keep = valid_in && !m_abs && !m_int;
            const double fd = valid_in ? (double)f : 0.0, ed = valid_in ? (double)e : 1.0;
            const float fc = a.correct ? (float)__ddiv_rn(fd, T) : f;
            const float ec = a.correct ? (float)__ddiv_rn(ed, T) : e;
            const float fw = keep ? fc : -999.0f, ew = keep ? ec : -999.0f;
            if (k < Npix) {
                fo[k] = fw;
                eo[k] = ew;
                if (to) to[k] = (float)T;
            }
            // the record is taken from the output arrays: a kept pixel whose quotient rounds to the sentinel is not valid there
            const bool valid_out = keep && fw != -999.0f && ew != -999.0f;
            if (valid_out && g >= a.snr_lo && g < a.snr_hi) {
                ps = __dadd_rn(ps, __ddiv_rn((double)fw, (double)ew));
                ++cs;
            }
            cabs += (valid_in && m_abs) ? 1 : 0;
            cint += (valid_in && !m_abs && m_int) ? 1 : 0;
            const unsigned long long bits = __ballot(valid_out);
            if (lane == 0) s_bits[i * kWaves + wv] = bits;
        }
        int ln = lane;
        asm volatile("" : "+v"(ln));
        ps = wave_sum(ps, ln);
        cs = wave_isum(cs, ln);
        cabs = wave_isum(cabs, ln);
        cint = wave_isum(cint, ln);
        if (lane == 0) {
            s_sum[wv] = ps;
            s_cnt[wv][0] = cs; s_cnt[wv][1] = cabs; s_cnt[wv][2] = cint;
        }
        __syncthreads();
        if (wv == 0) {                                                            // the runs of the validity bitmap (k_preprocess's walk)
            double ssn = s_sum[0];
            int ns = s_cnt[0][0], nabs = s_cnt[0][1], nint = s_cnt[0][2];
#pragma unroll
            for (int q = 1; q < kWaves; ++q) {
                ssn = __dadd_rn(ssn, s_sum[q]);
                ns += s_cnt[q][0]; nabs += s_cnt[q][1]; nint += s_cnt[q][2];
            }
            int nv = 0, starts = 0, first = kMaxNpix, last = -1;
            for (int wd = lane; wd < nwords; wd += 64) {
                const unsigned long long v = s_bits[wd];                          // (bits of pixels >= Npix are 0)
                const unsigned long long carry = wd > 0 ? s_bits[wd - 1] >> 63 : 0ull;
                const int tail = Npix - wd * 64;
                const unsigned long long exist = tail >= 64 ? ~0ull : ((1ull << tail) - 1ull);
                starts += __popcll(~v & exist & ((v << 1) | carry));
                nv += __popcll(v);
                if (v) {
                    first = min(first, wd * 64 + (int)__ffsll((long long)v) - 1);
                    last = max(last, wd * 64 + 63 - (int)__clzll((long long)v));
                }
            }
            nv = wave_isum(nv, ln);
            starts = wave_isum(starts, ln);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                first = min(first, __shfl(first, ln ^ d));
                last = max(last, __shfl(last, ln ^ d));
            }
            if (lane == 0) {
                const int lead = nv ? first : Npix, trail = nv ? Npix - 1 - last : Npix;
                int32_t *ri = a.rec_i32 + 6 * s;
                a.rec_f64[s] = ns > 0 ? __ddiv_rn(ssn, (double)ns) : __longlong_as_double(0x7ff8000000000000ll);
                ri[0] = nv;
                ri[1] = lead;
                ri[2] = trail;
                ri[3] = starts - ((nv > 0 && trail > 0) ? 1 : 0);                 // the trailing run started behind a valid pixel too
                ri[4] = nabs;
                ri[5] = nint;
            }
        }
        __syncthreads();                                                          // the bitmap, the tile and the wave sums are free again
    }
}

}  // namespace qfa_absorber
