// qfa_obs.h -- the observed-frame residual stack r = flux / continuum in bins of observed wavelength, and the calibration that is
// applied from it (include/qfa_hip.h: qfa_obs_stack_f32, qfa_calibrate_f32).  Built in qfa_obs.hip.
//
//   k_obs_stack      a bin-owner gather.  The coordinate x(p) of a spectrum is monotone in the pixel p (pix_u is non-decreasing and
//                    every step of the rule is monotone), so the pixels of one spectrum in bin k are a contiguous run.  A block owns
//                    a tile of kThreads bins, a chunk of spectra and up to kDraws draws; a thread owns ONE bin.  Per spectrum of the
//                    chunk, in spectrum order: a lower-bound search ON THE FORWARD RULE finds the first pixel that is not before the
//                    bin -- no inverse formula, so no disagreement at an edge --, the thread walks its run while the rule itself says
//                    the pixel is in the bin, forms c, r, iv of every draw and adds the terms in registers, in pixel order.  The
//                    sums leave as the chunk's row of the workspace: every entry of the row is written, nothing is zeroed first.
//                    Consecutive threads read consecutive pixels of flux, error, mask and F.  No bin table anywhere: nbin is bounded
//                    by the row only.
//   k_obs_reduce     thread per entry of the stack: adds the chunks' rows in chunk order; stack (+)= the result
//   k_calibrate      thread per pixel, grid-stride over spectra: the linear interpolation of the table and the two divisions in
//                    float64; the count of the valid pixels left as they were by ballots, added in wave order by the block's thread 0
// No atomics.  Every float64 product and sum is a plain operator under `fp contract(off)`; a product that a subtraction follows is
// pinned first (the backend fuses `a b - c` into an fma whatever the pragma says).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"

namespace qfa_obs {

constexpr int kThreads = 256;                 // bins of a tile (k_obs_stack), pixels of a step (k_calibrate)
constexpr int kDraws = 4;                     // draws a thread carries in registers

struct Args {
    qfa_batch_t bt;                           // row_stride filled in by the host
    const float *F, *mu;                      // (Npix, Nh), (Npix,)
    const float *h;                           // (B, S, Nh)
    const float *unc;                         // (B, Npix) or NULL
    const double *pix_u, *spec_u;             // (Npix,), (B,)
    double *rows;                             // (chunks, S, 4, nbin)
    double u0, inv_du;
    int B, S, Npix, Nh, nbin, p_lo, p_hi, tiles, sgroups, rpc;
    int linear, unit_w;
    float cont_min;
};

// x = (u - u0) inv_du with u = pix_u + spec_u (log) or pix_u spec_u (linear): three roundings
__device__ __forceinline__ double coord(double pu, double su, int linear, double u0, double inv_du) {
#pragma clang fp contract(off)
    double u = linear ? pu * su : pu + su;
    pin(u);
    const double d = u - u0;
    return d * inv_du;
}

// grid (tiles * sgroups * chunks): block x = (chunk * sgroups + sgroup) * tiles + tile.  NHM >= Nh (8, 16 or 32); SC: the draws
// [s0, s0 + SC) of the block, those >= S idle.
template <int NHM, int SC>
__global__ __launch_bounds__(kThreads) void k_obs_stack(const Args a) {
#pragma clang fp contract(off)
    const int tile = blockIdx.x % a.tiles;
    const int sg = (blockIdx.x / a.tiles) % a.sgroups;
    const int chunk = blockIdx.x / (a.tiles * a.sgroups);
    const int Nh = a.Nh, S = a.S, nbin = a.nbin, p_lo = a.p_lo, p_hi = a.p_hi;
    const int s0 = sg * SC;
    const int k0 = tile * kThreads, k = k0 + (int)threadIdx.x;
    const bool own = k < nbin;
    const double klo = (double)k, khi = (double)(k + 1);
    const double t0 = (double)k0, t1 = (double)min(nbin, k0 + kThreads);
    const bool vecF = (Nh & 3) == 0 && (reinterpret_cast<uintptr_t>(a.F) & 15) == 0;
    double a0[SC], a1[SC], a2[SC];
    int cnt[SC];
#pragma unroll
    for (int sl = 0; sl < SC; ++sl) { a0[sl] = 0.0; a1[sl] = 0.0; a2[sl] = 0.0; cnt[sl] = 0; }
    const int b0 = chunk * a.rpc, b1 = min(a.B, b0 + a.rpc);
    for (int b = b0; b < b1; ++b) {
        const double su = a.spec_u[b];                                            // block-uniform
        if (!isfinite(su)) continue;                                              // stacks nothing
        // the spectrum's ends against the tile: x is monotone, rising unless a linear spec_u is negative
        const double xa = coord(a.pix_u[p_lo], su, a.linear, a.u0, a.inv_du);
        const double xb = coord(a.pix_u[p_hi - 1], su, a.linear, a.u0, a.inv_du);
        const bool rising = xa <= xb;
        const double xmin = rising ? xa : xb, xmax = rising ? xb : xa;
        if (!(xmax >= t0 && xmin < t1)) continue;                                 // (a NaN end: nothing to stack either)
        if (!own) continue;
        // first pixel of [p_lo, p_hi) that is not before bin k: before = x < k (rising), x >= k + 1 (falling)
        int lo = p_lo, hi = p_hi;
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            const double x = coord(a.pix_u[mid], su, a.linear, a.u0, a.inv_du);
            const bool before = rising ? x < klo : x >= khi;
            if (before) lo = mid + 1; else hi = mid;
        }
        const unsigned long long row = batch_row(a.bt, b);
        const unsigned long long base = row * (unsigned long long)a.bt.row_stride;
        const float *hb = a.h + ((int64_t)b * S + s0) * Nh;
        for (int p = lo; p < p_hi; ++p) {
            const double x = coord(a.pix_u[p], su, a.linear, a.u0, a.inv_du);
            if (!(x >= klo && x < khi)) break;                                    // the run has ended (floor(x) == k inside it)
            const float fl = a.bt.delta[base + (unsigned)p], sgm = a.bt.error[base + (unsigned)p];
            const bool mk = a.bt.mask ? a.bt.mask[base + (unsigned)p] != 0 : true;
            float u2 = 0.f;
            if (a.unc) {
                const float u = a.unc[(size_t)b * a.Npix + p];
                u2 = __fmul_rn(u, u);
            }
            const float s2 = __fmul_rn(sgm, sgm);
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
            const float m = a.mu[p];
#pragma unroll
            for (int sl = 0; sl < SC; ++sl) {
                if (s0 + sl >= S) break;                                          // (block-uniform)
                const float *hr = hb + sl * Nh;
                float c = m;
#pragma unroll
                for (int j = 0; j < NHM; ++j) {
                    const float hv = j < Nh ? hr[j] : 0.f;                        // block-uniform
                    c = fmaf(f[j], hv, c);
                }
                const float r = __fdiv_rn(fl, c);
                float rr = __fmul_rn(r, r);
                float ru = __fmul_rn(rr, u2);
                float cc = __fmul_rn(c, c);
                asm volatile("" : "+v"(ru), "+v"(cc));                            // (products: not to be fused into what follows)
                const float den = __fadd_rn(ru, s2);
                const float iv = __fdiv_rn(cc, den);
                const bool use = mk && c > a.cont_min && isfinite(r) && isfinite(iv);
                if (use) {                                                        // selects: nothing under the mask reaches a sum
                    const double dr = (double)r;
                    const double w = a.unit_w ? 1.0 : (double)iv;
                    const double wr = w * dr;
                    const double r2 = dr * dr;
                    const double wr2 = w * r2;
                    a0[sl] = a0[sl] + w;
                    a1[sl] = a1[sl] + wr;
                    a2[sl] = a2[sl] + wr2;
                    cnt[sl] += 1;
                }
            }
        }
    }
    if (own) {
        double *dst = a.rows + ((size_t)chunk * S + s0) * 4 * (size_t)nbin + k;
#pragma unroll
        for (int sl = 0; sl < SC; ++sl) {
            if (s0 + sl >= S) break;
            double *d = dst + (size_t)sl * 4 * nbin;
            d[0] = a0[sl];
            d[nbin] = a1[sl];
            d[2 * (size_t)nbin] = a2[sl];
            d[3 * (size_t)nbin] = (double)cnt[sl];
        }
    }
}

// stack[e] (+)= sum over the chunks, in chunk order, of rows[chunk * nent + e]
static __global__ __launch_bounds__(256) void k_obs_reduce(const double *__restrict__ rows, int chunks, size_t nent, int zero,
                                                           double *__restrict__ stack) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nent) return;
    double t = rows[e];
    for (int c = 1; c < chunks; ++c) t = t + rows[(size_t)c * nent + e];
    stack[e] = zero ? t : stack[e] + t;
}

struct CalArgs {
    const float *flux, *error;
    const double *pix_u, *spec_u, *cal;
    float *flux_out, *error_out;
    int32_t *n_uncal;
    double u0, inv_du, c_min;
    int N, Npix, ncal, linear;
};

// grid-stride over spectra, one block per spectrum at a time
static __global__ __launch_bounds__(kThreads) void k_calibrate(const CalArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_n[kThreads / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
        const double su = a.spec_u[n];
        const size_t base = (size_t)n * a.Npix;
        int left = 0;                                                             // (the wave's count, every lane)
        for (int p0 = 0; p0 < a.Npix; p0 += kThreads) {
            const int p = p0 + (int)threadIdx.x;
            bool valid = false;
            if (p < a.Npix) {
                const float fl = a.flux[base + p], er = a.error[base + p];
                valid = fl != -999.0f && er != -999.0f;
                bool done = false;
                float fo = fl, eo = er;
                if (valid) {
                    double xs = coord(a.pix_u[p], su, a.linear, a.u0, a.inv_du);
                    pin(xs);
                    const double x = xs - 0.5;
                    if (x >= 0.0 && x <= (double)(a.ncal - 1)) {                  // (a NaN x fails)
                        const int j = min((int)floor(x), a.ncal - 2);
                        const double fr = x - (double)j;
                        const double c0 = a.cal[j], c1 = a.cal[j + 1];
                        const double dc = c1 - c0;
                        const double c = fma(fr, dc, c0);
                        if (isfinite(c) && c >= a.c_min) {
                            fo = (float)((double)fl / c);
                            eo = (float)((double)er / c);
                            done = true;
                        }
                    }
                }
                a.flux_out[base + p] = fo;
                a.error_out[base + p] = eo;
                valid = valid && !done;
            }
            left += (int)__popcll(__ballot(valid));
        }
        if (lane == 0) s_n[wave] = left;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) t += s_n[w];
            a.n_uncal[n] = t;
        }
        __syncthreads();
    }
}

}  // namespace qfa_obs
