// qfa_forest.h -- Lyman-alpha forest transmission T = flux / continuum and its redshift-binned stack (include/qfa_hip.h,
// qfa_forest_f32).  Built in qfa_forest.hip.
//
//   k_forest_image   F (Npix, Nh) row-major -> image (Nh + 1, pad) of the BLUE pixels: row j = F[:, j], row Nh = mu, rows padded
//                    with zeros to kStrip pixels
//   k_forest         the shape of k_mock_spectra: a lane owns FOUR consecutive blue pixels and keeps their Nh + 1 image values in
//                    registers; a block owns a strip of kStrip pixels and walks a run of spectra.  Flux, error, mask, z and unc of
//                    (b, p) are read once per launch, the bin of every pixel is formed once, and the draws s of the launch are looped
//                    in registers: c, T, iv are formed, stored and stacked, no continuum is ever written.
//   the stack        a wave's 256 pixels of one spectrum fall into the bins [kmin, kmax] (wave-uniform, formed once per spectrum;
//                    a few consecutive bins when z is monotone in p).  Per draw and per bin of that range that holds a used pixel:
//                    a lane adds its own pixels of the bin in pixel order, a butterfly (xor 1, 2, .. 32) adds the lanes -- the
//                    same tree on every run -- and lane 0 alone adds the three sums and the count to the wave's OWN table
//                    [draw][4][nbin] (float64).  LDS form (nbin <= 512): four tables in LDS, added in wave order into the block's
//                    row of the workspace at the end.  Global form (nbin > 512): the table IS the wave's row of the workspace
//                    (zeroed by the host's memset node).  The host cuts S into launches whose tables fit; k_forest_reduce adds the
//                    rows in order into `stack` after every launch.  No atomics.
//   k_forest_reduce  one thread per (entry, eighth of the rows): float64 sums over consecutive rows, the eight partial sums added in
//                    order; stack (+)= the result
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_continuum.h"

namespace qfa_forest {

using namespace qfa_continuum;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStrip = 4 * kThreads;
constexpr int kReduceGroups = 8;              // k_forest_reduce: 32 entries x 8 row ranges per block

struct Args {
    qfa_batch_t bt;                           // row_stride filled in by the host
    const float *img;                         // (Nh + 1, pad)
    const float *h;                           // (B, S, Nh)
    const float *unc;                         // (B, Npix) or NULL
    float *trans, *ivar;                      // (B, S, Nb) or NULL
    double *rows;                             // partial sums: one row per block (LDS form) or per wave (global form); NULL = no stack
    int pad, B, S, s0, Sc, ScMax, Npix, Nb, Nh, strips, rpb, nbin, p_lo, p_hi;
    float z0, inv_dz, cont_min;
    int unit_w, factored;
};

static __global__ void k_forest_image(const float *__restrict__ F, const float *__restrict__ mu, int Nb, int Nh, int pad,
                                      float *__restrict__ img) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)(Nh + 1) * pad) return;
    const int j = (int)(i / pad), p = (int)(i % pad);
    float v = 0.f;
    if (p < Nb) v = j < Nh ? F[(int64_t)p * Nh + j] : mu[p];
    img[i] = v;
}

// (not qfa_bal::wave_tree_sum: that one adds the lanes l ^ 32, 16, .., 1, and the float64 sums differ in the last bit)
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = __dadd_rn(x, __shfl_xor(x, d));
    return x;
}

// grid (strips * chunks), block x = chunk * strips + strip.  NHM >= Nh (8, 16 or 32): the columns [Nh, NHM) of the image registers
// and of the latent row are zeros.  LDS: the waves' tables live in dynamic LDS (kWaves * ScMax * 4 * nbin doubles).
template <int NHM, bool LDS>
__global__ __launch_bounds__(kThreads) void k_forest(const Args a) {
    extern __shared__ double lds_tab[];
    const int strip = blockIdx.x % a.strips;
    const int chunk = blockIdx.x / a.strips;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nbin = a.nbin, Nh = a.Nh, Nb = a.Nb, S = a.S;
    const bool stack = a.rows != nullptr;
    const int tablen = a.ScMax * 4 * nbin;                                        // doubles of one wave's table
    double *tab = nullptr;
    if (stack) {
        if (LDS) {
            for (int e = threadIdx.x; e < kWaves * tablen; e += kThreads) lds_tab[e] = 0.0;
            __syncthreads();
            tab = lds_tab + wave * tablen;
        } else {
            tab = a.rows + ((size_t)blockIdx.x * kWaves + wave) * (size_t)tablen;   // zeroed before the launch
        }
    }
    const int p0 = strip * kStrip + 4 * (int)threadIdx.x;
    // a wave with no blue pixel has nothing to do (it still meets the block at the barriers of the LDS form)
    if (strip * kStrip + 4 * (int)(threadIdx.x & ~63u) < Nb) {
        const int n = min(4, max(0, Nb - p0));                                    // blue pixels of this lane that exist
        const int b0 = chunk * a.rpb, b1 = min(a.B, b0 + a.rpb);
        float f[NHM][4], m[4], ratio[4];
#pragma unroll
        for (int j = 0; j < NHM; ++j) {
            float4 q = {0.f, 0.f, 0.f, 0.f};
            if (j < Nh) q = *reinterpret_cast<const float4 *>(a.img + (int64_t)j * a.pad + p0);   // p0 + 3 < pad, 16-byte aligned
            f[j][0] = q.x; f[j][1] = q.y; f[j][2] = q.z; f[j][3] = q.w;
        }
        {
            const float4 q = *reinterpret_cast<const float4 *>(a.img + (int64_t)Nh * a.pad + p0);
            m[0] = q.x; m[1] = q.y; m[2] = q.z; m[3] = q.w;
        }
        bool inr[4];                                                              // the pixel exists and is in [p_lo, p_hi)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ratio[k] = (a.factored && k < n) ? a.bt.pix_ratio[p0 + k] : 0.f;
            inr[k] = k < n && p0 + k >= a.p_lo && p0 + k < a.p_hi;
        }
        const float fnbin = (float)nbin;
        for (int b = b0; b < b1; ++b) {
            const unsigned long long row = batch_row(a.bt, b);
            const unsigned long long off = row * (unsigned long long)a.bt.row_stride + (unsigned)p0;
            float fl[4], sg[4], u2[4] = {0.f, 0.f, 0.f, 0.f};
            load4(a.bt.delta + off, n, fl);
            load4(a.bt.error + off, n, sg);
            bool mk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[k] = k < n;
            if (a.bt.mask) {
                const uint8_t *mr = a.bt.mask + off;
#pragma unroll
                for (int k = 0; k < 4; ++k) mk[k] = k < n && mr[k] != 0;
            }
            if (a.unc) {
                float u[4];
                load4(a.unc + (size_t)b * a.Npix + p0, n, u);
#pragma unroll
                for (int k = 0; k < 4; ++k) u2[k] = __fmul_rn(u[k], u[k]);
            }
            float s2[4];
            int kb[4];                                                            // the pixel's bin, or -1: not stacked
            int kmin = nbin, kmax = -1;
            {
                const float zq = a.factored ? a.bt.zq1[row] : 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s2[k] = __fmul_rn(sg[k], sg[k]);
                    kb[k] = -1;
                    if (stack && inr[k]) {
                        const float z = a.factored ? __fmaf_rn(zq, ratio[k], -1.0f) : a.bt.zabs[row * (unsigned long long)Nb + (unsigned)(p0 + k)];
                        const float kf = floorf(__fmul_rn(__fsub_rn(z, a.z0), a.inv_dz));
                        if (kf >= 0.f && kf < fnbin) kb[k] = (int)kf;              // (a NaN fails both)
                    }
                    if (kb[k] >= 0) {
                        kmin = min(kmin, kb[k]);
                        kmax = max(kmax, kb[k]);
                    }
                }
            }
            if (stack) {
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    kmin = min(kmin, __shfl_xor(kmin, d));
                    kmax = max(kmax, __shfl_xor(kmax, d));
                }
                kmin = wave_uniform(kmin);
                kmax = wave_uniform(kmax);
            }
            const float *hr = a.h + ((int64_t)b * S + a.s0) * Nh;
            int64_t o = ((int64_t)b * S + a.s0) * Nb + p0;
            for (int sl = 0; sl < a.Sc; ++sl, hr += Nh, o += Nb) {
                float c[4] = {m[0], m[1], m[2], m[3]};
#pragma unroll
                for (int j = 0; j < NHM; ++j) {
                    const float hv = j < Nh ? hr[j] : 0.f;                        // wave-uniform
#pragma unroll
                    for (int k = 0; k < 4; ++k) c[k] = fmaf(f[j][k], hv, c[k]);
                }
                float Tv[4], iv[4];
                bool use[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float T = __fdiv_rn(fl[k], c[k]);
                    const float den = __fadd_rn(__fmul_rn(__fmul_rn(T, T), u2[k]), s2[k]);
                    const float v = __fdiv_rn(__fmul_rn(c[k], c[k]), den);
                    use[k] = mk[k] && c[k] > a.cont_min && isfinite(T) && isfinite(v);
                    Tv[k] = use[k] ? T : 0.f;                                     // selects: nothing under the mask reaches an output
                    iv[k] = use[k] ? v : 0.f;
                }
                if (a.trans) store4(a.trans + o, n, Tv);
                if (a.ivar) store4(a.ivar + o, n, iv);
                if (stack && kmax >= kmin) {
                    double w[4], wt[4], wtt[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double dT = (double)Tv[k];
                        w[k] = a.unit_w ? 1.0 : (double)iv[k];
                        wt[k] = __dmul_rn(w[k], dT);
                        wtt[k] = __dmul_rn(w[k], __dmul_rn(dT, dT));
                    }
                    double *t = tab + (size_t)sl * 4 * nbin;
                    for (int kk = kmin; kk <= kmax; ++kk) {
                        bool in[4];
                        unsigned cnt = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            in[k] = use[k] && kb[k] == kk;
                            cnt += (unsigned)__popcll(__ballot(in[k]));
                        }
                        if (cnt == 0) continue;                                   // (wave-uniform)
                        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            a0 = __dadd_rn(a0, in[k] ? w[k] : 0.0);
                            a1 = __dadd_rn(a1, in[k] ? wt[k] : 0.0);
                            a2 = __dadd_rn(a2, in[k] ? wtt[k] : 0.0);
                        }
                        a0 = wave_sum(a0);
                        a1 = wave_sum(a1);
                        a2 = wave_sum(a2);
                        if (lane == 0) {                                          // the single writer of this wave's table
                            t[kk] = __dadd_rn(t[kk], a0);
                            t[nbin + kk] = __dadd_rn(t[nbin + kk], a1);
                            t[2 * nbin + kk] = __dadd_rn(t[2 * nbin + kk], a2);
                            t[3 * nbin + kk] = __dadd_rn(t[3 * nbin + kk], (double)cnt);
                        }
                    }
                }
            }
        }
    }
    if (LDS && stack) {
        __syncthreads();
        double *dst = a.rows + (size_t)blockIdx.x * (size_t)tablen;
        for (int e = threadIdx.x; e < tablen; e += kThreads) {
            double v = lds_tab[e];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v = __dadd_rn(v, lds_tab[w * tablen + e]);
            dst[e] = v;
        }
    }
}

// stack[e] (+)= sum over the R rows of rows[r * rowlen + e], e < nent: eight consecutive row ranges, their sums added in order
static __global__ __launch_bounds__(256) void k_forest_reduce(const double *__restrict__ rows, int R, size_t rowlen, int nent,
                                                              int zero, double *__restrict__ stack) {
    __shared__ double part[kReduceGroups][32];
    const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + el;
    const int per = (R + kReduceGroups - 1) / kReduceGroups;
    const int r0 = min(R, g * per), r1 = min(R, r0 + per);
    double acc = 0.0;
    if (e < nent)
        for (int r = r0; r < r1; ++r) acc = __dadd_rn(acc, rows[(size_t)r * rowlen + e]);
    part[g][el] = acc;
    __syncthreads();
    if (g == 0 && e < nent) {
        double t = part[0][el];
#pragma unroll
        for (int q = 1; q < kReduceGroups; ++q) t = __dadd_rn(t, part[q][el]);
        stack[e] = zero ? t : __dadd_rn(stack[e], t);
    }
}

}  // namespace qfa_forest
