// qfa_em.h -- kernels of the closed-form EM update of the factor loadings F (include/qfa_hip.h: qfa_em_stats_f32,
// qfa_em_update_f_f32).
//
// Per batch, with the posterior of the latent h of every spectrum s (the E-step: pass 1 + k_solve, y_s = C_s^-1 b_s,
// E_s = C_s^-1 + y_s y_s^T) and the per-element weights of pass 1 (qfa_common.h: wD = mask / D):
//   S2_i = sum_s wD A^2 E_s       S1_i = sum_s wD A delta y_s       cnt_i = sum_s mask
// and the M-step solves (S2_i + ridge I) f_i = S1_i per pixel.
//
//   k_em_record   [E_s | y_s] of every spectrum from the solve's record: Nh (Nh + 1) / 2 pair columns and Nh columns of y,
//                 each part padded to whole 16-column tiles (zeros)
//   k_em_stats    the hot path: a GEMM whose K dimension is the spectra.  A wave owns 16 pixels, the spectra stream past four
//                 at a time; the weights are formed on the VALU, the contraction is v_mfma_f32_16x16x4_f32 (A operand =
//                 weights of 16 pixels x 4 spectra, B operand = 4 spectra x 16 columns of the record).  Every 256 spectra the
//                 MFMA accumulators are folded into a second set by plain float32 adds and restarted, so that no MFMA chain is
//                 longer than 64 instructions ("Pass 1's accumulation chains").  The grid cuts the batch
//                 into ranges; every (range, pixel) leaves as a row of the slab by plain stores -- no atomics
//   k_em_reduce   slab rows -> stats in range order (float64 partial sums, one rounding), S2 unpacked to the full symmetric
//                 array (both triangles from the same pair column: bit-equal)
//   k_em_nll      sum NLL and the number of spectra (float64, fixed order, one block)
//   k_em_solve_f  one wave per pixel: float64 Cholesky of S2_i + ridge I in LDS, two triangular solves, damping
#pragma once
#include "qfa_common.h"

namespace qfa_em {

__host__ __device__ inline int npairs(int Nh) { return Nh * (Nh + 1) / 2; }
__host__ __device__ inline int pair_tiles(int Nh) { return (npairs(Nh) + 15) / 16; }
__host__ __device__ inline int y_tiles(int Nh) { return (Nh + 15) / 16; }
__host__ __device__ inline int rec_cols(int Nh) { return 16 * (pair_tiles(Nh) + y_tiles(Nh)); }

// ------------------------------------------------------------------------------------------------
// SOL record of k_solve (Cfg<KP>): [y KP][C^-1 pairs, row-major upper triangle of KP, off-diagonals doubled]...
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_em_record(const float *__restrict__ SOL, int nsol, int KP, int sol_ci, int B,
                                                          int Nh, float *__restrict__ REC) {
    const int ncp = rec_cols(Nh), np = npairs(Nh), ypos = 16 * pair_tiles(Nh);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * ncp) return;
    const int s = (int)(i / ncp), c = (int)(i % ncp);
    const float *sol = SOL + (size_t)s * nsol;
    float v = 0.f;
    if (c < np) {
        int a = 0, q = c;
        while (q >= Nh - a) { q -= Nh - a; ++a; }
        const int b = a + q;
        const float ci = sol[sol_ci + pair_index(a, b, KP)];
        v = fmaf(sol[a], sol[b], a == b ? ci : 0.5f * ci);
    } else if (c >= ypos && c < ypos + Nh) {
        v = sol[c - ypos];
    }
    REC[i] = v;
}

// ------------------------------------------------------------------------------------------------
// k_em_stats.  grid = (blocks of 64 pixels, ranges of spectra); 4 waves, wave w owns pixels 64 bx + 16 w ...
// NT column tiles per launch, starting at tile t0 (N_h > 16 runs several column passes); tiles < npt take beta = wD A^2,
// the others gamma' = wD A delta.  ZF: factored-z form (ZS per spectrum, ZP per pixel); HASA: host-supplied A_blue.
// SLAB [range][Npix][ncp], CNT [range][Npix] (written by the pass with t0 = 0).
// ------------------------------------------------------------------------------------------------
constexpr int kFlush = 64;      // MFMA steps (of four spectra) between two folds of the accumulators

template <int NT, bool ZF, bool HASA>
__global__ __launch_bounds__(256) void k_em_stats(qfa_params_t p, qfa_batch_t bt, qfa_tau_t tau, int B, int Npix, int Nb, int Nh,
                                                  int per, int t0, const float4 *__restrict__ ZS,
                                                  const float4 *__restrict__ ZP, const float *__restrict__ REC,
                                                  float *__restrict__ SLAB, float *__restrict__ CNT) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    const int p0 = ((int)blockIdx.x * 4 + w) * 16;
    if (p0 >= Npix) return;                                     // (whole wave; no block-level synchronisation below)
    const int npt = pair_tiles(Nh), ntl = npt + y_tiles(Nh), ncp = 16 * ntl;
    const int range = blockIdx.y;
    const int s_beg = range * per, s_end = min(B, s_beg + per);
    const int px = p0 + lo;
    const bool inb = px < Npix, blue = px < Nb;
    const DevConsts k = load_consts(p, tau);
    const float Psi = inb ? p.Psi[px] : 1.f;
    const float om = blue ? p.omega[px] : 0.f;
    float4 zp = {0.f, 0.f, 0.f, 0.f};
    if (ZF && blue) zp = ZP[px];

    f32x4 acc[NT], tot[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        tot[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float cnt = 0.f;
    int since = 0;
    for (int s4 = s_beg; s4 < s_end; s4 += 4) {
        const int s = s4 + g;
        const bool sv = s < s_end;
        const bool ld = sv && inb;
        float d = 0.f, sg = 1.f, z = 0.f, Ab = 1.f;
        unsigned char m = 0;
        ZFac zs{0.f, 0.f, 0.f};
        if (ld) {
            const unsigned long long row = batch_row(bt, s);
            const unsigned long long off = row * (unsigned long long)bt.row_stride + (unsigned)px;
            m = bt.mask[off];
            d = bt.delta[off];
            sg = bt.error[off];
            if (blue) {
                if (ZF) zs = zfac_load(ZS, s, true);
                else z = bt.zabs[row * (unsigned long long)Nb + (unsigned)px];
                if (HASA) Ab = bt.A_blue[(size_t)s * Nb + px];
            }
        }
        const bool wv = ld && m != 0;
        float A = 1.f, zd = 0.f;
        if (blue) {
            const BlueTerms bl = ZF ? blue_terms_zf(zs, zp.x, zp.y, zp.z, k) : blue_terms(z, k);
            A = HASA ? Ab : bl.A;
            zd = bl.zd;
        }
        const float A2 = A * A;
        const float D = A2 * Psi + om * zd + sg * sg;
        const float wD = wv ? fast_rcp(D) : 0.f;                 // a select: NaN / inf / -999 under the mask give an exact 0
        const float dd = wv ? d : 0.f;
        const float wDA = wD * A;
        const float beta = wDA * A, gam = wDA * dd;
        cnt += wv ? 1.f : 0.f;
        const float *rec = REC + (size_t)(sv ? s : s_beg) * ncp + lo;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int tt = t0 + t;                               // wave-uniform
            if (tt < ntl) {
                const float b = sv ? rec[16 * tt] : 0.f;
                acc[t] = mfma4(tt < npt ? beta : gam, b, acc[t]);
            }
        }
        if (++since == kFlush) {
            since = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                tot[t] += acc[t];
                acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[t] += acc[t];
    // D layout of the MFMA: lane (g, lo), register r = row (pixel) 4 g + r, column lo
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tt = t0 + t;
        if (tt >= ntl) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = p0 + 4 * g + r;
            if (q < Npix) SLAB[((size_t)range * Npix + q) * ncp + 16 * tt + lo] = tot[t][r];
        }
    }
    if (t0 == 0) {
        cnt += __shfl_xor(cnt, 16);
        cnt += __shfl_xor(cnt, 32);
        if (g == 0 && inb) CNT[(size_t)range * Npix + px] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------
// k_em_reduce : stats (+)= the slab rows, ranges in order.  One thread per element of [S2 | S1 | cnt].
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_em_reduce(const float *__restrict__ SLAB, const float *__restrict__ CNT, int R,
                                                          int Npix, int Nh, int zero, float *__restrict__ stats) {
    const int ncp = rec_cols(Nh), ypos = 16 * pair_tiles(Nh);
    const size_t n2 = (size_t)Npix * Nh * Nh, n1 = (size_t)Npix * Nh, n = n2 + n1 + (size_t)Npix;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *src;
    size_t stride;
    if (i < n2) {
        const int q = (int)(i / ((size_t)Nh * Nh)), e = (int)(i % ((size_t)Nh * Nh));
        const int a = e / Nh, b = e % Nh;
        src = SLAB + (size_t)q * ncp + pair_index(a < b ? a : b, a < b ? b : a, Nh);
        stride = (size_t)Npix * ncp;
    } else if (i < n2 + n1) {
        const size_t j = i - n2;
        src = SLAB + (j / Nh) * ncp + ypos + (j % Nh);
        stride = (size_t)Npix * ncp;
    } else {
        src = CNT + (i - n2 - n1);
        stride = (size_t)Npix;
    }
    double a = 0.0;
    for (int r = 0; r < R; ++r) a += (double)src[(size_t)r * stride];
    stats[i] = zero ? (float)a : stats[i] + (float)a;
}

// stats tail (+)= {sum NLL, B, 0, 0}
static __global__ __launch_bounds__(1024) void k_em_nll(const float *__restrict__ nll, int B, int zero, float *__restrict__ tail) {
    __shared__ double sh[16];
    double a = 0.0;
    for (int s = threadIdx.x; s < B; s += 1024) a += (double)nll[s];
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += sh[i];
        if (zero) {
            tail[0] = (float)t; tail[1] = (float)B; tail[2] = 0.f; tail[3] = 0.f;
        } else {
            tail[0] += (float)t; tail[1] += (float)B;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_em_solve_f : F_out_i = F_i + damping ((S2_i + ridge I)^-1 S1_i - F_i).  One wave per pixel, four per block; lane c holds
// row c.  The lower triangle of S2_i goes to LDS (float64, row stride 33), right-looking Cholesky, then L z = S1 and
// L^T x = z with the unknowns in registers and shuffles for the broadcast.  cnt_i = 0 or a pivot that is not > 0: the row
// is copied through and counted.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_em_solve_f(const float *__restrict__ stats, const float *__restrict__ F, int Npix,
                                                           int Nh, double ridge, double damping, float *__restrict__ F_out,
                                                           unsigned *__restrict__ n_skipped) {
    __shared__ double sL[4][32 * 33];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = (int)blockIdx.x * 4 + w;
    if (i >= Npix) return;                                        // (whole wave; waves synchronise with themselves only)
    double *L = sL[w];
    auto wave_lds_sync = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    const float *S2 = stats + (size_t)i * Nh * Nh;
    const float *S1 = stats + (size_t)Npix * Nh * Nh + (size_t)i * Nh;
    const float cnt = stats[(size_t)Npix * Nh * Nh + (size_t)Npix * Nh + i];
    const bool row = lane < Nh;
    const float fold = row ? F[(size_t)i * Nh + lane] : 0.f;
    bool fail = !(cnt > 0.f);
    if (row)
        for (int c = 0; c <= lane; ++c) L[lane * 33 + c] = (double)S2[lane * Nh + c] + (c == lane ? ridge : 0.0);
    wave_lds_sync();
    for (int j = 0; j < Nh; ++j) {
        const double piv = L[j * 33 + j];                         // the same address for every lane: wave-uniform
        if (!(piv > 0.0) || !(piv < 1.0e300)) { fail = true; break; }
        const double dj = sqrt(piv), idj = 1.0 / dj;
        double lij = 0.0;
        if (row && lane > j) lij = L[lane * 33 + j] * idj;
        wave_lds_sync();
        if (row && lane > j) L[lane * 33 + j] = lij;
        if (lane == j) L[j * 33 + j] = dj;
        wave_lds_sync();
        if (row && lane > j)
            for (int c = j + 1; c <= lane; ++c) L[lane * 33 + c] -= lij * L[c * 33 + j];
        wave_lds_sync();
    }
    double x = row ? (double)S1[lane] : 0.0;
    if (!fail) {
        for (int j = 0; j < Nh; ++j) {                            // L z = S1
            const double zj = __shfl(x, j) / L[j * 33 + j];
            if (lane == j) x = zj;
            else if (row && lane > j) x -= L[lane * 33 + j] * zj;
        }
        for (int j = Nh - 1; j >= 0; --j) {                       // L^T x = z
            const double xj = __shfl(x, j) / L[j * 33 + j];
            if (lane == j) x = xj;
            else if (lane < j) x -= L[j * 33 + lane] * xj;
        }
        const double bad = (x == x && x - x == 0.0) ? 0.0 : 1.0;  // a NaN / inf solution: keep the row
        double anybad = bad;
        for (int o = 32; o >= 1; o >>= 1) anybad += __shfl_xor(anybad, o);
        if (anybad != 0.0) fail = true;
    }
    if (row) F_out[(size_t)i * Nh + lane] = fail ? fold : (float)((double)fold + damping * (x - (double)fold));
    if (fail && lane == 0 && n_skipped) atomicAdd(n_skipped, 1u);
}

}  // namespace qfa_em
