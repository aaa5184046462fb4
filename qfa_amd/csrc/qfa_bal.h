// qfa_bal.h -- the BAL finder: balnicity-type indices of r = flux / continuum in velocity windows of emission lines, their trough
// lists, and the mask made from them (include/qfa_hip.h: qfa_bal_scan_f32, qfa_bal_mask_f32).  Built in qfa_bal.hip.
//
//   k_bal_scan   one wave (a block of 64 threads) per (spectrum, line, group of draws).  The window sits across the lanes in chunks
//                of 64 pixels, window pixel i = 64 chunk + lane; what a later pass reads of another pixel goes through LDS arrays of
//                the window's length (27 bytes per pixel).  Per draw: (A) c, r, use, sigma / c per pixel; (B) the boxcar r~ and
//                `below`; then per index definition (C) the domain flags from vedge, (D) with max_gap > 0 the stretches of unused
//                pixels and which of them are bridged, (E) the first and last pixel of every pixel's run, (F) every pixel's own
//                contribution from its run's edges, (G) the variance weights a_q.  Stretches and runs are found from ballot words:
//                "the last pixel at or below i that is not P" is the highest set bit of ballot(!P) at or below the lane, else the
//                carry of the chunks before; "the first at or above i" the same walked from the last chunk down.  No pixel waits
//                for another: every decision of a pixel is a function of its run's two ends.
//   k_bal_mask   a block per spectrum (grid-stride): the intervals of the reference draw's troughs in LDS, thread per pixel, the
//                count by ballots added in wave order by thread 0
// No atomics.  Every float64 operation is a plain operator or a __d*_rn intrinsic under `fp contract(off)`; a product that an addition
// follows is pinned first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"

namespace qfa_bal {

constexpr int kWave = 64;
constexpr int kMaxWin = QFA_BAL_MAX_WIN;
constexpr int kMaxTroughs = QFA_BAL_MAX_TROUGHS;
constexpr int kLdsPerPixel = 27;              // w 8 | rt 4 | r 4 | sc 4 | first 2 | last 2 | fl 1 | ni 1 | fx 1
constexpr double kC = 299792.458;             // C_KMS of qfa_amd/absorbers.py
constexpr int kMaskThreads = 256;

enum : unsigned char { FL_USED = 1, FL_BELOW = 2 };
enum : unsigned char { FX_DOM = 1, FX_BD = 2, FX_U = 4, FX_BRIDGED = 8 };

struct Args {
    qfa_batch_t bt;                           // row_stride filled in by the host
    const float *F, *mu, *h;                  // (Npix, Nh), (Npix,), (B, S, Nh)
    const double *vedge[QFA_BAL_MAX_LINES];
    int p_lo[QFA_BAL_MAX_LINES], p_hi[QFA_BAL_MAX_LINES];
    qfa_bal_index_t index[QFA_BAL_MAX_INDICES];
    double thr;
    double *value, *var, *troughs;            // (B, S, L, I), (B, S, L, I), (B, S, L, kMaxTroughs, 2)
    int32_t *counts, *line_counts;            // (B, S, L, I, 3), (B, S, L, 2)
    int B, S, Npix, Nh, n_lines, n_indices, smooth, max_gap, trough_index, nsg, spg, nmax;
    float cont_min;
};

__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }

// sum over the wave in a fixed tree (lanes l and l ^ m, m = 32, 16, .., 1): every lane ends with the same bits
// (not qfa_forest::wave_sum: that one adds the lanes l ^ 1, 2, .., 32, and the float64 sums differ in the last bit)
__device__ __forceinline__ double wave_tree_sum(double x) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, kWave);
    return x;
}

// first[i] = 1 + the last j <= i with !P_j (0 if none);  last[i] = -1 + the first j >= i with !P_j (pixels >= n are !P).  P of pixel i
// is (fx[i] & bits) != 0.  One wave; the caller puts barriers around it.
__device__ __forceinline__ void scan_ends(const unsigned char *fx, unsigned char bits, int n, int nchunks, int lane, short *first,
                                          short *last) {
    int carry = -1;
    for (int k = 0; k < nchunks; ++k) {
        const int i = k * kWave + lane;
        const bool P = i < n && (fx[i] & bits) != 0;
        const unsigned long long nb = __ballot(!P);
        const unsigned long long m = nb & (~0ull >> (63 - lane));
        const int prev = m ? k * kWave + 63 - __clzll((long long)m) : carry;
        if (i < n) first[i] = (short)(prev + 1);
        if (nb) carry = k * kWave + 63 - __clzll((long long)nb);
    }
    carry = n;
    for (int k = nchunks - 1; k >= 0; --k) {
        const int i = k * kWave + lane;
        const bool P = i < n && (fx[i] & bits) != 0;
        const unsigned long long nb = __ballot(!P);
        const unsigned long long m = nb & (~0ull << lane);
        const int next = m ? k * kWave + __ffsll((long long)m) - 1 : carry;
        if (i < n) last[i] = (short)(next - 1);
        if (nb) carry = k * kWave + __ffsll((long long)nb) - 1;
    }
}

// grid (B * n_lines * nsg): block x = (b * n_lines + line) * nsg + sg; the draws [sg spg, min(S, (sg + 1) spg)).  NHM >= Nh.
template <int NHM>
__global__ __launch_bounds__(kWave) void k_bal_scan(const Args a) {
#pragma clang fp contract(off)
    extern __shared__ double s_dyn[];
    const int nmax = a.nmax;
    double *s_w = s_dyn;                                                          // contributed width of pixel i under the index at hand
    float *s_rt = reinterpret_cast<float *>(s_w + nmax);                          // r~
    float *s_r = s_rt + nmax;                                                     // r
    float *s_sc = s_r + nmax;                                                     // sigma / c
    short *s_first = reinterpret_cast<short *>(s_sc + nmax);
    short *s_last = s_first + nmax;
    unsigned char *s_fl = reinterpret_cast<unsigned char *>(s_last + nmax);       // FL_*
    unsigned char *s_ni = s_fl + nmax;                                            // used pixels of the box
    unsigned char *s_fx = s_ni + nmax;                                            // FX_* under the index at hand

    const int lane = threadIdx.x;
    const int sg = blockIdx.x % a.nsg;
    const int line = (blockIdx.x / a.nsg) % a.n_lines;
    const int b = blockIdx.x / (a.nsg * a.n_lines);
    const int Nh = a.Nh, S = a.S, L = a.n_lines, NI = a.n_indices;
    const int p_lo = a.p_lo[line], p_hi = a.p_hi[line];
    const int n = p_hi - p_lo, nchunks = (n + kWave - 1) / kWave;
    const double *__restrict__ ve = a.vedge[line];
    const int hw = a.smooth >> 1;
    const double thr = a.thr;
    const bool vecF = (Nh & 3) == 0 && (reinterpret_cast<uintptr_t>(a.F) & 15) == 0;
    const unsigned long long row = batch_row(a.bt, b);
    const unsigned long long base = row * (unsigned long long)a.bt.row_stride;
    const int s0 = sg * a.spg, s1 = min(S, s0 + a.spg);

    for (int s = s0; s < s1; ++s) {
        const float *hr = a.h + ((int64_t)b * S + s) * Nh;
        const size_t o_line = ((size_t)b * S + s) * L + line;
        // (A) the pixel rule in its noise-only form (qfa_continuum.h: den = sigma^2; where it parts from k_obs_stack with unc = NULL)
        int n_used = 0;
        for (int k = 0; k < nchunks; ++k) {
            const int i = k * kWave + lane;
            const bool valid = i < n;
            const int p = valid ? p_hi - 1 - i : p_lo;
            const float fl = a.bt.delta[base + (unsigned)p], sgm = a.bt.error[base + (unsigned)p];
            const bool mk = a.bt.mask ? a.bt.mask[base + (unsigned)p] != 0 : true;
            float f[NHM];
            const float *Fr = a.F + (int64_t)p * Nh;
            if (vecF) {
#pragma unroll
                for (int j = 0; j < NHM; j += 4) {
                    float4 q = {0.f, 0.f, 0.f, 0.f};
                    if (j < Nh) q = *reinterpret_cast<const float4 *>(Fr + j);
                    f[j] = q.x; f[j + 1] = q.y; f[j + 2] = q.z; f[j + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NHM; ++j) f[j] = j < Nh ? Fr[j] : 0.f;
            }
            float c = a.mu[p];
#pragma unroll
            for (int j = 0; j < NHM; ++j) {
                const float hv = j < Nh ? hr[j] : 0.f;                            // wave-uniform
                c = fmaf(f[j], hv, c);
            }
            const float r = __fdiv_rn(fl, c);
            const float s2 = __fmul_rn(sgm, sgm);
            float cc = __fmul_rn(c, c);
            asm volatile("" : "+v"(cc));
            const float iv = __fdiv_rn(cc, s2);
            const bool use = valid && mk && c > a.cont_min && isfinite(r) && isfinite(iv);
            if (valid) {                                                          // selects: nothing under the mask is stored
                s_r[i] = use ? r : 0.f;
                s_sc[i] = use ? __fdiv_rn(sgm, c) : 0.f;
                s_fl[i] = use ? FL_USED : 0;
            }
            n_used += (int)__popcll(__ballot(use));
        }
        __syncthreads();
        // (B) the boxcar over the used pixels of [i - hw, i + hw] clipped to the window, added in order of j; defined where i is used
        for (int k = 0; k < nchunks; ++k) {
            const int i = k * kWave + lane;
            if (i < n && (s_fl[i] & FL_USED)) {
                float sum = 0.f;
                int cnt = 0;
                const int j0 = max(0, i - hw), j1 = min(n - 1, i + hw);
                for (int j = j0; j <= j1; ++j) {
                    if (s_fl[j] & FL_USED) {
                        sum = __fadd_rn(sum, s_r[j]);
                        ++cnt;
                    }
                }
                const float rt = __fdiv_rn(sum, (float)cnt);
                s_rt[i] = rt;
                s_ni[i] = (unsigned char)cnt;
                if ((double)rt < thr) s_fl[i] = FL_USED | FL_BELOW;               // (only this lane writes s_fl[i]; the others read bit 0)
            }
        }
        __syncthreads();
        int n_troughs = 0;
        for (int x = 0; x < NI; ++x) {
            const double v_lo = a.index[x].v_lo, v_hi = a.index[x].v_hi, w_min = a.index[x].w_min;
            const bool after = a.index[x].mode == QFA_BAL_AFTER;
            // (C) the domain
            for (int k = 0; k < nchunks; ++k) {
                const int i = k * kWave + lane;
                if (i < n) {
                    const double cw = dmin(ve[i + 1], v_hi) - dmax(ve[i], v_lo);
                    const unsigned char fl = s_fl[i];
                    unsigned char fx = 0;
                    if (cw > 0.0) fx = FX_DOM | ((fl & FL_BELOW) ? FX_BD : 0) | ((fl & FL_USED) ? 0 : FX_U);
                    s_fx[i] = fx;
                }
            }
            __syncthreads();
            // (D) bridging: a maximal stretch of 1 .. max_gap unused in-domain pixels with a below pixel directly on both sides
            if (a.max_gap > 0) {
                scan_ends(s_fx, FX_U, n, nchunks, lane, s_first, s_last);
                __syncthreads();
                for (int k = 0; k < nchunks; ++k) {
                    const int i = k * kWave + lane;
                    if (i < n && (s_fx[i] & FX_U)) {
                        const int u0 = s_first[i], u1 = s_last[i];
                        const bool br = u1 - u0 + 1 <= a.max_gap && u0 >= 1 && u1 + 1 < n && (s_fx[u0 - 1] & FX_BD) && (s_fx[u1 + 1] & FX_BD);
                        if (br) s_fx[i] = FX_DOM | FX_U | FX_BRIDGED;             // (the pixels read above are not FX_U: nobody writes them)
                    }
                }
                __syncthreads();
            }
            // (E) the runs
            scan_ends(s_fx, FX_BD | FX_BRIDGED, n, nchunks, lane, s_first, s_last);
            __syncthreads();
            // (F) every pixel's contribution from its run's ends
            double acc = 0.0;
            int n_pix = 0, n_runs = 0, n_bridged = 0;
            double *tr = a.troughs + o_line * (kMaxTroughs * 2);
            for (int k = 0; k < nchunks; ++k) {
                const int i = k * kWave + lane;
                const unsigned char fx = i < n ? s_fx[i] : 0;
                const bool member = (fx & (FX_BD | FX_BRIDGED)) != 0;
                double wi = 0.0, e0 = 0.0, e1 = 0.0;
                bool runq = false, isend = false;
                if (member) {
                    const int fi = s_first[i], li = s_last[i];
                    e0 = dmax(ve[fi], v_lo);
                    e1 = dmin(ve[li + 1], v_hi);
                    const double hi_i = dmin(ve[i + 1], v_hi);
                    if (after) {
                        const double st = e0 + w_min;
                        runq = dmin(ve[li + 1], v_hi) - dmax(ve[li], st) > 0.0;
                        if (fx & FX_BD) wi = dmax(0.0, hi_i - dmax(ve[i], st));
                    } else {
                        runq = e1 - e0 >= w_min;
                        if (runq && (fx & FX_BD)) wi = hi_i - dmax(ve[i], v_lo);
                    }
                    isend = i == li;
                }
                const bool contrib = wi > 0.0;
                if (contrib) {
                    const double q = (double)s_rt[i] / thr;
                    const double d = 1.0 - q;
                    double t = d * wi;
                    pin(t);
                    acc = acc + t;
                }
                if (i < n) s_w[i] = wi;
                n_pix += (int)__popcll(__ballot(contrib));
                n_bridged += (int)__popcll(__ballot(runq && (fx & FX_BRIDGED)));
                const unsigned long long ends = __ballot(isend && runq);
                if (x == a.trough_index) {
                    if (isend && runq) {
                        const int rank = n_troughs + (int)__popcll(ends & ((1ull << lane) - 1ull));
                        if (rank < kMaxTroughs) {
                            tr[2 * rank] = e0;
                            tr[2 * rank + 1] = e1;
                        }
                    }
                    n_troughs += (int)__popcll(ends);
                }
                n_runs += (int)__popcll(ends);
            }
            __syncthreads();
            // (G) var = thr^-2 sum_q (sigma_q / c_q)^2 a_q^2, a_q = sum over the used i of [q - hw, q + hw] of w_i / n_i, in order of i
            double vacc = 0.0;
            for (int k = 0; k < nchunks; ++k) {
                const int q = k * kWave + lane;
                if (q < n && (s_fl[q] & FL_USED)) {
                    double aq = 0.0;
                    const int i0 = max(0, q - hw), i1 = min(n - 1, q + hw);
                    for (int i = i0; i <= i1; ++i) {
                        const double wi = s_w[i];
                        if (wi > 0.0) aq = aq + wi / (double)s_ni[i];
                    }
                    if (aq > 0.0) {
                        const double sc = (double)s_sc[q];
                        const double g = sc * sc;
                        const double a2 = aq * aq;
                        double t = g * a2;
                        pin(t);
                        vacc = vacc + t;
                    }
                }
            }
            acc = wave_tree_sum(acc);
            vacc = wave_tree_sum(vacc);
            if (lane == 0) {
                const size_t o = o_line * NI + x;
                a.value[o] = acc;
                a.var[o] = vacc / (thr * thr);
                a.counts[3 * o] = n_pix;
                a.counts[3 * o + 1] = n_runs;
                a.counts[3 * o + 2] = n_bridged;
            }
            __syncthreads();                                                      // s_w, s_fx, s_first, s_last are free again
        }
        {
            double *tr = a.troughs + o_line * (kMaxTroughs * 2);
            const int filled = min(n_troughs, kMaxTroughs);
            if (lane < 2 * kMaxTroughs && (lane >> 1) >= filled) tr[lane] = __longlong_as_double(0x7ff8000000000000ll);
            if (lane == 0) {
                a.line_counts[2 * o_line] = n_used;
                a.line_counts[2 * o_line + 1] = n_troughs;
            }
        }
    }
}

struct MaskArgs {
    const unsigned char *mask_in;             // (B, Npix) or NULL = all true
    const double *wav, *troughs;              // (Npix,), (B, S, L, kMaxTroughs, 2)
    unsigned char *mask_out;
    int32_t *n_masked;
    double lam[QFA_BAL_MAX_LINES];
    double pad;
    int B, S, L, s_ref, Npix, nlam;
};

static __global__ __launch_bounds__(kMaskThreads) void k_bal_mask(const MaskArgs a) {
#pragma clang fp contract(off)
    constexpr int kIv = QFA_BAL_MAX_LINES * kMaxTroughs * QFA_BAL_MAX_LINES;
    __shared__ double s_lo[kIv], s_hi[kIv];
    __shared__ int s_n[kMaskThreads / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nt = a.L * kMaxTroughs, niv = nt * a.nlam;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const double *tr = a.troughs + ((size_t)b * a.S + a.s_ref) * a.L * (kMaxTroughs * 2);
        if ((int)threadIdx.x < niv) {
            const int t = threadIdx.x / a.nlam, l = threadIdx.x - t * a.nlam;
            const double vmin = __dsub_rn(tr[2 * t], a.pad), vmax = __dadd_rn(tr[2 * t + 1], a.pad);
            // lam (1 - v / c) of qfa_amd.absorbers.bal_intervals: a division, a subtraction, a product (NaN for an unfilled slot)
            s_lo[threadIdx.x] = __dmul_rn(a.lam[l], __dsub_rn(1.0, __ddiv_rn(vmax, kC)));
            s_hi[threadIdx.x] = __dmul_rn(a.lam[l], __dsub_rn(1.0, __ddiv_rn(vmin, kC)));
        }
        __syncthreads();
        int cnt = 0;
        for (int p0 = 0; p0 < a.Npix; p0 += kMaskThreads) {
            const int p = p0 + (int)threadIdx.x;
            bool newly = false;
            if (p < a.Npix) {
                const double g = a.wav[p];
                bool inside = false;
                for (int q = 0; q < niv; ++q) inside |= g >= s_lo[q] && g < s_hi[q];
                const bool m = a.mask_in ? a.mask_in[(size_t)b * a.Npix + p] != 0 : true;
                a.mask_out[(size_t)b * a.Npix + p] = (m && !inside) ? 1 : 0;
                newly = m && inside;
            }
            cnt += (int)__popcll(__ballot(newly));
        }
        if (lane == 0) s_n[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < kMaskThreads / 64; ++w) t += s_n[w];
            a.n_masked[b] = t;
        }
        __syncthreads();
    }
}

}  // namespace qfa_bal
