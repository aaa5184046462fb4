// qfa_preprocess.h -- observed-frame spectra onto the common rest-frame grid: rebin, normalise, S/N and the catalogue's run
// counts (include/qfa_hip.h, qfa_preprocess_f32, states the rule).  Built in qfa_preprocess.hip.
//
//   k_preprocess_windows  win[k] = bit 0: norm_lo <= wav_grid[k] < norm_hi | bit 1: snr_lo <= wav_grid[k] < snr_hi, one byte per
//                         output pixel in the workspace: the windows are the same for every spectrum
//   k_preprocess          one workgroup of kThreads = 1024 per spectrum, grid-stride over the spectra.  Thread t owns the output
//                         pixels k = t, t + 1024, .. (at most kPer = 16: Npix <= 16 384), so that the lanes of a wave own
//                         neighbouring pixels: their input pixels are neighbours too and the stores are whole lines.
//     rebin     per owned pixel: binary search on the input edges for the first input pixel whose upper edge lies above the
//               pixel's lower edge, then a walk forward while the input's lower edge lies below the pixel's upper edge; the four
//               float64 sums W, sum c u f, sum c^2 u, coverage in input-pixel order.  Input edges are formed from `wave` where they
//               are needed (two loads, an addition, a halving).  The input is NOT staged in LDS: at the limit a spectrum's
//               wave / flux / ivar / bad are 32 768 x 17 B = 544 KB, more than a CU's LDS, and at survey size (4 600 .. 7 800
//               pixels, 78 .. 133 KB) a staged copy would leave one workgroup per CU no room and would be read about once anyway
//               -- every input pixel overlaps one or two output pixels, and those belong to the same or the neighbouring lane, so
//               the second read hits the line the first one brought into L1 / L2.
//     on chip   until norm is known the unrounded flux_k of the owned pixels stay in REGISTERS (16 float64 = 32 VGPRs; the loop over
//               the owned pixels is a run-time loop whose result is dealt to the array by selects on the uniform index, so the
//               rebin exists once) and ivar_k in LDS (8 Npix bytes, 128 KB at the limit).  Both as float64 are 256 KB at the limit,
//               more than the 160 KB of a CU; both in registers are 64 VGPRs beside the ~105 the rebin needs, more than the 128 a
//               wave has at 16 waves per CU.  Validity goes to a bitmap in LDS by ballot (2 KB).
//     sums      norm's numerator and denominator, the S/N sum and the two counts: per thread in order of k, a butterfly over the
//               wave (xor 1, 2, .. 32), lane 0 to LDS, and every thread adds the 16 wave sums in wave order: one fixed tree.
//     runs      wave 0 walks the bitmap 64 pixels per lane-word: popcounts for n_valid, (not v) & (v << 1 | carry) for the
//               starts of invalid runs behind a valid pixel, ctz / clz for the first and last valid pixel; integer butterflies.
//     write     flux_out, error_out once, float32, -999 where invalid or not ok.
//   LDS: 131 072 (ivar_k) + 2 048 (bitmap) + 16 x 3 x 8 + 16 x 2 x 4 (wave sums) = 133 632 bytes, static: one workgroup per CU, which
//   1 024 threads at more than 64 VGPRs are anyway.  107 VGPRs, no scratch, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qfa_hip.h"

namespace qfa_preprocess {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 16;                        // output pixels a thread owns at most
constexpr int kMaxNpix = kThreads * kPer;       // 16 384
constexpr int kMaxIn = 32768;
constexpr int kWords = kMaxNpix / 64;

struct Args {
    const double *wave;                         // ragged input, concatenated
    const float *flux, *ivar;
    const uint8_t *bad;                         // or NULL
    const int64_t *offsets;                     // (N + 1)
    const double *zqso;                         // (N)
    const double *edges;                        // (Npix + 1) rest-frame output edges
    const uint8_t *win;                         // (Npix) window bits
    float *flux_out, *error_out;                // (N, Npix)
    double *rec_f64;                            // (N, 2) norm, snr
    int32_t *rec_i32;                           // (N, 5) n_valid, n_lead, n_trail, num_mask, ok
    int64_t N;
    int Npix, max_n_in, norm_min_pixels;
    double min_coverage;
};

static __global__ void k_preprocess_windows(const double *__restrict__ grid, int Npix, double norm_lo, double norm_hi,
                                            double snr_lo, double snr_hi, uint8_t *__restrict__ win) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Npix) return;
    const double g = grid[k];
    win[k] = (uint8_t)((g >= norm_lo && g < norm_hi ? 1 : 0) | (g >= snr_lo && g < snr_hi ? 2 : 0));
}

// observed edge j (0 <= j <= n) of a spectrum of n >= 2 pixels: additions, subtractions and halvings only
__device__ __forceinline__ double in_edge(const double *__restrict__ w, int n, int j) {
    if (j == 0) return w[0] - (0.5 * (w[0] + w[1]) - w[0]);
    if (j == n) return w[n - 1] + (w[n - 1] - 0.5 * (w[n - 2] + w[n - 1]));
    return 0.5 * (w[j - 1] + w[j]);
}

// (the partner lanes are formed from `lane` where they are used: hoisted out of the spectrum loop they would hold six registers)
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

__global__ __launch_bounds__(kThreads) void k_preprocess(const Args a) {
    __shared__ double s_ik[kMaxNpix];                                             // ivar_k of the valid pixels (the others are never read)
    __shared__ unsigned long long s_bits[kWords];
    __shared__ double s_sum[kWaves][3];                                           // norm numerator, denominator, S/N sum
    __shared__ int s_cnt[kWaves][2];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int Npix = a.Npix, nwords = (Npix + 63) >> 6;
    for (int64_t s = blockIdx.x; s < a.N; s += gridDim.x) {
        const int64_t off = a.offsets[s];
        const int64_t n64 = a.offsets[s + 1] - off;
        const double zp1 = 1.0 + a.zqso[s];
        // fewer than two pixels, or 1 + z not a positive finite number: the spectrum covers nothing
        const int n = (n64 >= 2 && n64 <= (int64_t)a.max_n_in && zp1 > 0.0 && isfinite(zp1)) ? (int)n64 : 0;
        const double *__restrict__ w = a.wave + off;
        const float *__restrict__ fin = a.flux + off;
        const float *__restrict__ vin = a.ivar + off;
        const uint8_t *__restrict__ bin = a.bad ? a.bad + off : nullptr;
        const double e_last = n ? in_edge(w, n, n) : 0.0;

        double fk[kPer];
        unsigned vmask = 0;
        double pn = 0.0, pd = 0.0, ps = 0.0;
        int cn = 0, cs = 0;
#pragma unroll
        for (int q = 0; q < kPer; ++q) fk[q] = 0.0;
        // (a run-time loop: the body exists once, and its results are dealt to the register arrays by selects on the uniform i)
#pragma unroll 1
        for (int i = 0; i * kThreads + wv * 64 < Npix; ++i) {                     // (wave-uniform: the wave owns a word of the bitmap)
            const int k = i * kThreads + tid;
            bool valid = false;
            double fv = 0.0, iv = 0.0;
            if (k < Npix && n) {
                const double E0 = __dmul_rn(a.edges[k], zp1), E1 = __dmul_rn(a.edges[k + 1], zp1);
                const double width = __dsub_rn(E1, E0);
                double W = 0.0, S1 = 0.0, S2 = 0.0, cov = 0.0;
                if (E0 < e_last) {
                    int lo = 0, hi = n - 1;                                       // first j with edge(j + 1) > E0; edge(n) > E0
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (in_edge(w, n, mid + 1) > E0) hi = mid; else lo = mid + 1;
                    }
                    double el = in_edge(w, n, lo);
                    for (int j = lo; j < n && el < E1; ++j) {
                        const double eh = in_edge(w, n, j + 1);
                        const double ov = __dsub_rn(fmin(eh, E1), fmax(el, E0));  // > 0: eh > E0, el < E1
                        const double c = __ddiv_rn(ov, width);
                        const float u = vin[j], f = fin[j];
                        const bool use = u > 0.f && isfinite(u) && isfinite(f) && !(bin && bin[j]);
                        const double cu = __dmul_rn(c, use ? (double)u : 0.0);
                        W = __dadd_rn(W, cu);
                        S1 = __dadd_rn(S1, __dmul_rn(cu, use ? (double)f : 0.0)); // selects: nothing unusable reaches a sum
                        S2 = __dadd_rn(S2, __dmul_rn(c, cu));
                        cov = __dadd_rn(cov, use ? c : 0.0);
                        el = eh;
                    }
                }
                valid = cov >= a.min_coverage && W > 0.0;
                if (valid) {
                    fv = __ddiv_rn(S1, W);
                    iv = __ddiv_rn(__dmul_rn(W, W), S2);
                    s_ik[k] = iv;
                    const uint8_t wb = a.win[k];
                    if (wb & 1) {
                        pn = __dadd_rn(pn, __dmul_rn(iv, fv));
                        pd = __dadd_rn(pd, iv);
                        ++cn;
                    }
                    if (wb & 2) {
                        ps = __dadd_rn(ps, __dmul_rn(fv, sqrt(iv)));
                        ++cs;
                    }
                    vmask |= 1u << i;
                }
            }
#pragma unroll
            for (int q = 0; q < kPer; ++q) fk[q] = q == i ? fv : fk[q];
            const unsigned long long bits = __ballot(valid);
            if (lane == 0) s_bits[i * kWaves + wv] = bits;
        }
        int ln = lane;
        asm volatile("" : "+v"(ln));
        pn = wave_sum(pn, ln);
        pd = wave_sum(pd, ln);
        ps = wave_sum(ps, ln);
        cn = wave_isum(cn, ln);
        cs = wave_isum(cs, ln);
        if (lane == 0) {
            s_sum[wv][0] = pn; s_sum[wv][1] = pd; s_sum[wv][2] = ps;
            s_cnt[wv][0] = cn; s_cnt[wv][1] = cs;
        }
        __syncthreads();
        double num = s_sum[0][0], den = s_sum[0][1], ssn = s_sum[0][2];
        int nn = s_cnt[0][0], ns = s_cnt[0][1];
#pragma unroll 4                                                                  // (unrolled whole, the 80 LDS values are all in flight at once)
        for (int q = 1; q < kWaves; ++q) {
            num = __dadd_rn(num, s_sum[q][0]);
            den = __dadd_rn(den, s_sum[q][1]);
            ssn = __dadd_rn(ssn, s_sum[q][2]);
            nn += s_cnt[q][0];
            ns += s_cnt[q][1];
        }
        const double norm = __ddiv_rn(num, den);                                  // 0 / 0 = NaN: not ok
        const bool ok = nn >= a.norm_min_pixels && norm > 0.0 && isfinite(norm);

        if (wv == 0) {                                                            // the runs of the validity bitmap
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
                double *rf = a.rec_f64 + 2 * s;
                int32_t *ri = a.rec_i32 + 5 * s;
                rf[0] = norm;
                rf[1] = ns > 0 ? __ddiv_rn(ssn, (double)ns) : __longlong_as_double(0x7ff8000000000000ll);
                ri[0] = nv;
                ri[1] = lead;
                ri[2] = trail;
                ri[3] = starts - ((nv > 0 && trail > 0) ? 1 : 0);                 // the trailing run started behind a valid pixel too
                ri[4] = ok ? 1 : 0;
            }
        }
        float *__restrict__ fo = a.flux_out + s * (int64_t)Npix;
        float *__restrict__ eo = a.error_out + s * (int64_t)Npix;
#pragma unroll 1
        for (int i = 0; i * kThreads + wv * 64 < Npix; ++i) {
            const int k = i * kThreads + tid;
            double fv = 0.0;
#pragma unroll
            for (int q = 0; q < kPer; ++q) fv = q == i ? fk[q] : fv;
            if (k < Npix) {
                const bool v = ok && ((vmask >> i) & 1u);
                fo[k] = v ? (float)__ddiv_rn(fv, norm) : -999.0f;
                eo[k] = v ? (float)__ddiv_rn(1.0, __dmul_rn(sqrt(v ? s_ik[k] : 1.0), norm)) : -999.0f;
            }
        }
        __syncthreads();                                                          // the bitmap and the wave sums are free again
    }
}

}  // namespace qfa_preprocess
