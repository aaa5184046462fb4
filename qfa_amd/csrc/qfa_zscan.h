// qfa_zscan.h -- the quasar-redshift finder: the likelihood of every spectrum under the trained model at 2 m + 1 integer pixel
// shifts between data and model (include/qfa_hip.h: qfa_redshift_scan_f32 states the rule).  Built in
// qfa_zscan.hip.  The image of F (k_scan_pf), the pair layout and the float64 Cholesky (chol_quad) are the DLA finder's, qfa_dla.h.
//
//   k_zscan_model   per model pixel q < Npad: {Psi, omega (0 on the red side), mu, blue flag}; pads {1, 0, 0, 0}
//   k_zscan_prep    per spectrum and data pixel p, stored at index p + m of a row of RL = Npad + 2 m records: {x, sigma^2,
//                   exp(-tau(z_p)), zd(z_p)} -- everything that depends on p alone.  sigma^2 = -1 marks a pixel that is masked or
//                   outside the window [m, Npix - m); such a record is {0, -1, 1, 0}, finite whatever the arrays hold there
//   k_zscan         the hot path.  A workgroup owns one spectrum and keeps its records in LDS (or reads them from memory when
//                   they pass 64 KiB); wave w takes the candidate tiles w, w + 4, ..  Lane (lo, g) is candidate s = -m + 16 ct + lo
//                   (clamped to m: the pad candidates repeat the last one and are never read) at model pixel q = 4 j + g: it reads
//                   the record of p = q - s, forms w A^2 and w A delta on the VALU and feeds them as the A operand of
//                   v_mfma_f32_16x16x4_f32 against the PF tiles.  The float32 accumulators hold one block of 16 model pixels (four
//                   MFMAs a tile) and are then added into float64 registers: a float32 chain over the whole spectrum misses the
//                   bar.  sum w delta^2, sum ln D and n are summed per lane in float64 / int
//   k_zscan_close   one wave per (spectrum, candidate): C in float64 in LDS, Cholesky, NLL_s as a double
//   k_zscan_best    one wave per spectrum: llr = (float)(NLL_0 - NLL_s), nll0, the arg-max in the order (value, |s|, s), the parabola
//   No atomics, no scratch.
#pragma once
#include "qfa_common.h"
#include "qfa_dla.h"

namespace qfa_zscan {

using qfa_dla::chol_quad;
using qfa_dla::f_tiles;
using qfa_dla::npairs;
using qfa_dla::pair_tiles;
using qfa_dla::pf_cols;
using qfa_dla::wave_lds_sync;

enum { SC_D3 = 0, SC_LD, SC_N, SC_COLS };                        // the float64 scalars of a candidate

static __global__ __launch_bounds__(256) void k_zscan_model(qfa_params_t p, const float *__restrict__ mu, int Npix, int Npad, int Nb,
                                                            float4 *__restrict__ MQ) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Npad) return;
    float4 v{1.f, 0.f, 0.f, 0.f};
    if (q < Npix) v = float4{p.Psi[q], q < Nb ? p.omega[q] : 0.f, mu[q], q < Nb ? 1.f : 0.f};
    MQ[q] = v;
}

// one thread per (spectrum of the chunk, record index < RL).  REC [spectrum][RL]
static __global__ __launch_bounds__(256) void k_zscan_prep(qfa_params_t p, qfa_batch_t bt, qfa_tau_t tau, const float *__restrict__ ratio,
                                                           int s0, int nspec, int Npix, int RL, int Nb, int m, float4 *__restrict__ REC) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nspec * RL) return;
    const int sl = (int)(i / RL), k = (int)(i % RL) - m, s = s0 + sl;
    float4 rec{0.f, -1.f, 1.f, 0.f};
    if (k >= m && k < Npix - m) {
        const unsigned long long row = batch_row(bt, s);
        const unsigned long long off = row * (unsigned long long)bt.row_stride + (unsigned)k;
        if (bt.mask[off] != 0) {
            const float fl = bt.delta[off], sg = bt.error[off];
            const bool fin = fl - fl == 0.f && sg - sg == 0.f;                     // a non-finite value in a used pixel poisons the spectrum
            rec.x = fin ? fl : __int_as_float(0x7fc00000);
            rec.y = fin ? __fmul_rn(sg, sg) : 1.f;
            if (k < Nb + m) {                                                      // blue under some candidate: q = k + s < Nb for s >= -m
                const DevConsts kc = load_consts(p, tau);
                const BlueTerms bl = blue_terms(__fmaf_rn(bt.zq1[row], ratio[k], -1.0f), kc);
                rec.z = bl.A;
                rec.w = bl.zd;
            }
        }
    }
    REC[i] = rec;
}

// ------------------------------------------------------------------------------------------------
// k_zscan.  grid = spectra of the chunk.  MOM [spectrum][ncp][pc] float64, SC [spectrum][ncp][SC_COLS] float64.
// NTL: tiles of the accumulator array; the shape's ntl = pair_tiles + f_tiles tiles are taken NTL at a time.
// ------------------------------------------------------------------------------------------------
template <int NTL, bool LDS>
__global__ __launch_bounds__(256) void k_zscan(const float4 *__restrict__ REC, const float *__restrict__ PF,
                                               const float4 *__restrict__ MQ, int Npad, int RL, int Nh, int m, int nct,
                                               double *__restrict__ MOM, double *__restrict__ SC) {
    extern __shared__ float4 srec[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    const int sl = blockIdx.x;
    const float4 *grec = REC + (size_t)sl * RL;
    if (LDS) {
        for (int i = threadIdx.x; i < RL; i += 256) srec[i] = grec[i];
        __syncthreads();
    }
    const int npt = pair_tiles(Nh), ntl = npt + f_tiles(Nh), pc = 16 * ntl, ncp = 16 * nct;
    for (int ct = w; ct < nct; ct += 4) {
        const int s = min(-m + 16 * ct + lo, m);
        // the tiles in groups of NTL (one group up to N_h = 16, two of 18 above: 35 tiles of float64 sums do not fit the register file);
        // every group walks the pixels and forms the same operands, and the scalars of the last group stand
#pragma unroll 1
        for (int t0 = 0; t0 < ntl; t0 += NTL) {
            double dacc[NTL][4];
#pragma unroll
            for (int t = 0; t < NTL; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) dacc[t][r] = 0.0;
            double d3 = 0.0, dl = 0.0;
            int cnt = 0;
#pragma unroll 1
            for (int q1 = 0; q1 < Npad; q1 += 16) {                   // a block of 16 model pixels: float32 on the matrix pipe ..
                f32x4 acc[NTL];
#pragma unroll
                for (int t = 0; t < NTL; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int q = q1 + 4 * jj + g, i = q - s + m;     // 0 <= i < Npad + 2 m
                    const float4 r = LDS ? srec[i] : grec[i];
                    const float4 mq = MQ[q];
                    const bool used = r.y >= 0.f;
                    const float A = mq.w != 0.f ? r.z : 1.0f;
                    const float G = __fmaf_rn(__fmul_rn(A, A), mq.x, __fmul_rn(mq.y, r.w));
                    const float D = __fadd_rn(G, used ? r.y : 1.0f);
                    const float wd = used ? fast_rcp(D) : 0.f;
                    const float dp = __fmaf_rn(-A, mq.z, r.x);
                    const float u = __fmul_rn(wd, A), e = __fmul_rn(wd, dp);
                    const float t1 = __fmul_rn(u, A), t2 = __fmul_rn(e, A);
                    d3 += (double)__fmul_rn(e, dp);
                    dl += (double)(used ? fast_log(D) : 0.f);
                    cnt += used ? 1 : 0;
                    const float *pf = PF + (size_t)q * pc + lo;
#pragma unroll
                    for (int tt = 0; tt < NTL; ++tt)
                        if (t0 + tt < ntl) acc[tt] = mfma4(t0 + tt < npt ? t1 : t2, pf[16 * (t0 + tt)], acc[tt]);
                }
#pragma unroll
                for (int tt = 0; tt < NTL; ++tt)                      // .. and float64 across the blocks
                    if (t0 + tt < ntl)
#pragma unroll
                        for (int r = 0; r < 4; ++r) dacc[tt][r] += (double)acc[tt][r];
            }
            // the scalars of candidate lo: the four pixel phases g in order (as lane g = 0 sees it)
            const double a3 = ((d3 + __shfl(d3, lo + 16)) + __shfl(d3, lo + 32)) + __shfl(d3, lo + 48);
            const double al = ((dl + __shfl(dl, lo + 16)) + __shfl(dl, lo + 32)) + __shfl(dl, lo + 48);
            const int an = cnt + __shfl(cnt, lo + 16) + __shfl(cnt, lo + 32) + __shfl(cnt, lo + 48);
            double *mom = MOM + ((size_t)sl * ncp + 16 * ct) * pc;
            // D layout of the MFMA: lane (g, lo), register r = row (candidate) 4 g + r, column lo
#pragma unroll
            for (int tt = 0; tt < NTL; ++tt) {
                if (t0 + tt >= ntl) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) mom[(size_t)(4 * g + r) * pc + 16 * (t0 + tt) + lo] = dacc[tt][r];
            }
            if (g == 0) {
                double *sc = SC + ((size_t)sl * ncp + 16 * ct + lo) * SC_COLS;
                sc[SC_D3] = a3;
                sc[SC_LD] = al;
                sc[SC_N] = (double)an;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_zscan_close: one wave per (spectrum of the chunk, candidate < nc):
//   NLL = (sum w delta^2 - b^T C^-1 b + n log 2 pi + sum ln D + log det C) / 2, float64;  NaN for a pivot that is not positive and finite
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_zscan_close(const double *__restrict__ MOM, const double *__restrict__ SC, int nspec, int nc,
                                                            int ncp, int Nh, double *__restrict__ NLL) {
    __shared__ double sL[4][32 * 33];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t item = (size_t)blockIdx.x * 4 + w;
    if (item >= (size_t)nspec * nc) return;                       // (whole wave; waves synchronise with themselves only)
    const int sl = (int)(item / nc), c = (int)(item % nc);
    double *L = sL[w];
    const int pc = pf_cols(Nh), fpos = 16 * pair_tiles(Nh);
    const double *mom = MOM + ((size_t)sl * ncp + c) * pc;
    const double *sc = SC + ((size_t)sl * ncp + c) * SC_COLS;
    if (lane < Nh)
        for (int a = 0; a <= lane; ++a) L[lane * 33 + a] = mom[pair_index(a, lane, Nh)] + (a == lane ? 1.0 : 0.0);
    wave_lds_sync();
    const double bl = lane < Nh ? mom[fpos + lane] : 0.0;
    double quad, logdet;
    const bool ok = chol_quad(L, lane, Nh, bl, quad, logdet);
    if (lane == 0) {
        const double v = 0.5 * (sc[SC_D3] - quad + sc[SC_N] * 1.8378770664093453 + sc[SC_LD] + logdet);
        NLL[item] = ok ? v : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// ------------------------------------------------------------------------------------------------
// k_zscan_best: one wave per spectrum of the chunk.  The outputs are indexed by the spectrum of the batch (the caller offsets them).
// The best candidate: the largest llr; among equals the lowest |s|, then the lowest s; NaN is never taken; none: s = 0, NaN.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void zbest_merge(float &v, int &i, float v2, int i2, int m) {
    if (i2 < 0) return;
    const int a = abs(i - m), a2 = abs(i2 - m);
    if (i < 0 || v2 > v || (v2 == v && (a2 < a || (a2 == a && i2 < i)))) { v = v2; i = i2; }
}
static __global__ __launch_bounds__(64) void k_zscan_best(const double *__restrict__ NLL, int nc, int m, float *__restrict__ llr,
                                                          float *__restrict__ nll0, int *__restrict__ best_s, float *__restrict__ best_llr,
                                                          double *__restrict__ off, double *__restrict__ sig) {
    const int lane = threadIdx.x, sl = blockIdx.x;
    const double *nl = NLL + (size_t)sl * nc;
    float *row = llr + (size_t)sl * nc;
    const double n0 = nl[m];
    float v = 0.f;
    int i = -1;
    for (int c = lane; c < nc; c += 64) {
        const float x = (float)(n0 - nl[c]);                      // the one rounding; c = m: an exact 0 (NaN for a poisoned spectrum)
        row[c] = x;
        if (x == x) zbest_merge(v, i, x, c, m);
    }
    for (int o = 32; o >= 1; o >>= 1) {                           // a strict total order: both sides of an exchange keep the same one
        const float v2 = __shfl_xor(v, o);
        const int i2 = __shfl_xor(i, o);
        zbest_merge(v, i, v2, i2, m);
    }
    if (lane != 0) return;
    const float fnan = __int_as_float(0x7fc00000);
    const double dnan = __longlong_as_double(0x7ff8000000000000ll);
    nll0[sl] = (float)n0;
    if (best_s) best_s[sl] = i < 0 ? 0 : i - m;
    if (best_llr) best_llr[sl] = i < 0 ? fnan : v;
    double o = dnan, sg = dnan;
    if (i > 0 && i < nc - 1) {
        // the parabola through the three float32 llr values around the best candidate, in float64
        const double ym = (double)(float)(n0 - nl[i - 1]), y0 = (double)v, yp = (double)(float)(n0 - nl[i + 1]);
        const double cv = (ym - y0) + (yp - y0);
        if (cv < 0.0) {
            o = 0.5 * (ym - yp) / cv;
            sg = 1.0 / sqrt(-cv);
        }
    }
    if (off) off[sl] = o;
    if (sig) sig[sl] = sg;
}

}  // namespace qfa_zscan
