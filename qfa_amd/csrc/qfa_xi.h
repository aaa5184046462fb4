// qfa_xi.h -- the pair-weighted line-of-sight correlation function of forest segments and its (lag, z) stack (include/qfa_hip.h,
// qfa_xi_f32).  Built in qfa_p1d.hip; the per-pixel rule and the z-bin of a segment are qfa_segment.h's.
//
//   k_xi         a block of 256 threads owns one segment.  (1) thread j mod 256 forms w_j and x_j = w_j d_j from trans / ivar / z / tbar
//                (the pixel rule and the weight on top of it) and stores them to LDS, zeros behind pixel L - 1; the threads add
//                their used pixels and their (w w) v, a butterfly and the four waves in order make n_used and N0.  delta_F never
//                reaches memory.  (2) a valid segment: thread (t, c) owns the eight lags 8t .. 8t + 7 and the pixels of chunk c,
//                [c Jc, (c + 1) Jc) below L - 8t (pairs of these lags that start further up fall off the segment).  It walks them in
//                steps of four: x[j .. j + 3] as one 16-byte read that the lanes of a chunk share, x[j + 8t .. j + 8t + 11] as three
//                aligned 16-byte reads, 32 products as 18 packed fma (v_pk_fma_f32: a pixel times an aligned pair of what was read;
//                the odd pixels' pairs straddle the lags, which costs two idle halves) into nine accumulator pairs; the same for
//                w: 64 products per eight reads, 18 independent chains.  (3) the chunks' partials meet in LDS and are added in chunk
//                order.  The plan (lag groups per pass, chunks, pixels per chunk) is made on the host from (L, nlag) alone: so is
//                the order of every sum.
//   k_xi_stack   a block owns one chunk of 64 consecutive segments (in order of (b, g)) of one draw: per z-bin the wave ballots the
//                chunk's codes (lane i holds segment i), and thread l adds W_l, A_l and their three products (float64, each rounded
//                once) in segment order from 0; the partial row of (chunk, draw, z-bin) goes to the workspace.
// The stack (S, nz, 2 + 5 nlag) is k_chunk_reduce's (qfa_segment.h) with head = 2 + 5 nlag, n = 0.
// No atomics, and nothing here depends on the grid: k_p1d_band's decomposition (qfa_p1d_band.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_segment.h"

namespace qfa_xi {

constexpr int kThreads = 256;
constexpr int kChunk = qfa_segment::kChunk;     // segments of a reduction chunk (qfa_p1d_band_chunk_segments())
constexpr int kLags = 8;                        // lags of a thread
constexpr int kStep = 4;                        // pixels of a step
constexpr int kPad = 12;                        // zeros behind the segment: the last step reads x[j + 8t + 11], j + 8t <= L - 1
typedef float f32x2 __attribute__((ext_vector_type(2)));

// the tile plan of a segment, a function of (L, nlag) alone
struct Tile {
    int ntp;                                    // lag groups of a pass: a power of two <= 256
    int nc;                                     // pixel chunks = 256 / ntp (1 when the lags need more than one pass)
    int Jc;                                     // pixels of a chunk, a multiple of four
    int Lp;                                     // floats of an LDS array: L rounded up to four, plus kPad
    int Ls;                                     // floats from one LDS array to the next: Lp or Lp + 4, an odd number of 16-byte slots
    int dup;                                    // x and w are held twice (four arrays fit 64 KB): see k_xi
};

__host__ __device__ inline Tile make_tile(int L, int nlag) {
    Tile t;
    const int nt = (nlag + kLags - 1) / kLags;
    t.ntp = 1;
    while (t.ntp < nt && t.ntp < kThreads) t.ntp <<= 1;
    t.nc = kThreads / t.ntp;
    const int per = (L + t.nc - 1) / t.nc;
    t.Jc = (per + 3) & ~3;
    t.Lp = ((L + 3) & ~3) + kPad;
    t.Ls = ((t.Lp >> 2) | 1) << 2;
    t.dup = (size_t)4 * t.Ls * sizeof(float) <= ((size_t)64 << 10) ? 1 : 0;
    return t;
}

struct Args {
    qfa_batch_t bt;                             // redshift only: zabs, or zq1 + pix_ratio; rows
    const float *trans, *ivar;                  // (B, S, Nb)
    const float *tbar;                          // (St, nT)
    float *pairs;                               // (segments of this launch, 2, nlag) or NULL
    float *noise0;                              // (segments of this launch,) or NULL
    int *code;                                  // [S][Bc nseg] z-bin of a valid segment, -1 otherwise; or NULL
    int b0, Bc, S, St, Nb, L, nlag, nseg, p_lo, min_used, nT, nz, factored, unit_w;
    Tile tile;
    float zT0, inv_dzT, z0, inv_dz, sigma2;
};
static_assert(qfa_segment::has_segment_fields<Args>(), "the fields qfa_segment.h reads");

// grid (gx, gy) with gx gy >= segments of the launch; dynamic LDS: (dup ? 4 : 2) Ls floats.
// A thread's three reads of x[j + 8t ..] are 32 bytes apart from its neighbour's: the sixteen lanes that ds_read_b128 serves in one
// cycle would meet on eight 16-byte slots of the 256-byte bank row, two-way.  So x and w are stored twice, the second copy an odd
// number of slots behind the first, and the lanes with bit 3 of t set read the second: their slots are odd, the others' even.
// (Beyond L = 4080 four arrays pass 64 KB: one copy, and the two-way conflict.  The sums and their order are the same.)
__global__ __launch_bounds__(kThreads) void k_xi(const Args a) {
    extern __shared__ __align__(16) float lds[];                                  // [x Ls | its copy Ls | w Ls | its copy Ls]
    __shared__ __align__(16) float red[kThreads * 2 * kLags];                     // [chunk][lag group][W 8 | A 8]
    __shared__ float s_n0[kThreads / 64];
    __shared__ int s_nu[kThreads / 64];
    const int L = a.L, nlag = a.nlag, S = a.S, nseg = a.nseg;
    const int Lp = a.tile.Lp, Ls = a.tile.Ls, dup = a.tile.dup, ntp = a.tile.ntp, nc = a.tile.nc, Jc = a.tile.Jc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nsegs = (int64_t)a.Bc * S * nseg;
    const int64_t q = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (q >= nsegs) return;                                                       // (the whole block)
    float *xs = lds, *ws = lds + (dup ? 2 : 1) * Ls;

    const int g = (int)(q % nseg);
    const int64_t rs = q / nseg;
    const int s = (int)(rs % S), bl = (int)(rs / S);
    // (qfa_segment::locate and code_slot written out, and `used` re-formed from the pixel below: this kernel's code is sensitive to how
    // these reach the compiler -- profiles/segment_refactor_asm.txt -- and in this form it is the code it was before qfa_segment.h)
    const int b = a.b0 + bl;
    const unsigned long long zrow = batch_row(a.bt, b);
    qfa_segment::Segment sg;
    sg.zq = a.factored ? a.bt.zq1[zrow] : 0.f;
    const int pseg = a.p_lo + g * L;                                              // the segment's first pixel
    sg.tr = a.trans + ((int64_t)b * S + s) * a.Nb + pseg;
    sg.iv = a.ivar + ((int64_t)b * S + s) * a.Nb + pseg;
    sg.tb = a.tbar + (int64_t)(a.St == 1 ? 0 : s) * a.nT;
    sg.zr = a.factored ? a.bt.pix_ratio + pseg : a.bt.zabs + zrow * (unsigned long long)a.Nb + (unsigned)pseg;


    // ---- (1) w and x of the segment, once; n_used and N0
    float n0 = 0.f;
    int nused = 0;
    for (int j = tid; j < Lp; j += kThreads) {
        float w = 0.f, x = 0.f;
        if (j < L) {
#pragma clang fp contract(off)
            const qfa_segment::Pixel px = qfa_segment::pixel(a, sg, j);
            const qfa_segment::Contrast c = qfa_segment::contrast(px);
            const bool used = px.ivar > 0.f && px.tbar > 0.f;                     // (qfa_segment::pixel_used, see above)
            const float d = used ? c.d : 0.f;                                     // selects: nothing under the mask reaches an output
            const float v = used ? c.v : 0.f;
            const float wv = __fdiv_rn(1.0f, __fadd_rn(v, a.sigma2));
            w = a.unit_w ? (used ? 1.0f : 0.f) : ((used && __builtin_isfinite(wv)) ? wv : 0.f);
            x = __fmul_rn(w, d);
            n0 = __fmaf_rn(__fmul_rn(w, w), v, n0);
            nused += used ? 1 : 0;
        }
        xs[j] = x;
        ws[j] = w;
        if (dup) {
            xs[Ls + j] = x;
            ws[Ls + j] = w;
        }
    }
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        n0 = __fadd_rn(n0, __shfl_xor(n0, dlt));
        nused += __shfl_xor(nused, dlt);
    }
    if (lane == 0) {
        s_n0[wave] = n0;
        s_nu[wave] = nused;
    }
    __syncthreads();                                                              // x, w and the waves' sums are written
    n0 = __fadd_rn(__fadd_rn(s_n0[0], s_n0[1]), __fadd_rn(s_n0[2], s_n0[3]));
    nused = s_nu[0] + s_nu[1] + s_nu[2] + s_nu[3];
    const bool valid = nused >= a.min_used;
    if (tid == 0) {
        if (a.noise0) a.noise0[q] = valid ? n0 : 0.f;
        if (a.code) a.code[(int64_t)s * ((int64_t)a.Bc * nseg) + (int64_t)bl * nseg + g] = qfa_segment::segment_code(a, sg, valid);
    }
    if (!a.pairs) return;
    float *out = a.pairs + q * 2 * (int64_t)nlag;
    if (!valid) {                                                                 // (block-uniform)
        for (int o = tid; o < 2 * nlag; o += kThreads) out[o] = 0.f;
        return;
    }

    // ---- (2) the pair sums, (3) the chunks in order
    const int nt = (nlag + kLags - 1) / kLags;
    const int tl = tid & (ntp - 1), c = tid / ntp;
    const int copy = (dup && (tl & 8)) ? Ls : 0;
    const float *xr = xs + copy, *wr = ws + copy;
    for (int t0 = 0; t0 < nt; t0 += ntp) {                                        // (one pass unless nlag > 2048)
        const int t = t0 + tl, l0 = kLags * t;
        // e[i] = lags (2i, 2i + 1) from the even pixels of a step, o[i] = lags (2i - 1, 2i) from the odd ones: either way the second
        // operand is an aligned pair (x[j + l0 + 2m], x[j + l0 + 2m + 1]) of what was read.  o[0].x and o[4].y belong to no lag.
        f32x2 eA[4], oA[5], eW[4], oW[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            oA[i] = oW[i] = f32x2{0.f, 0.f};
            if (i < 4) eA[i] = eW[i] = f32x2{0.f, 0.f};
        }
        int jend = (c + 1) * Jc;
        jend = jend < L - l0 ? jend : L - l0;
        if (t >= nt) jend = 0;
        for (int j = c * Jc; j < jend; j += kStep) {                              // (j + l0 <= L - 1: reads end at Lp - 1 at most)
            const f32x4 xa = *reinterpret_cast<const f32x4 *>(xs + j);
            const f32x4 wa = *reinterpret_cast<const f32x4 *>(ws + j);
            f32x2 px[6], pw[6];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const f32x4 xb = *reinterpret_cast<const f32x4 *>(xr + j + l0 + 4 * m);
                const f32x4 wb = *reinterpret_cast<const f32x4 *>(wr + j + l0 + 4 * m);
                px[2 * m] = f32x2{xb[0], xb[1]};
                px[2 * m + 1] = f32x2{xb[2], xb[3]};
                pw[2 * m] = f32x2{wb[0], wb[1]};
                pw[2 * m + 1] = f32x2{wb[2], wb[3]};
            }
#pragma unroll
            for (int k = 0; k < kStep; k += 2) {
                const f32x2 x0 = f32x2{xa[k], xa[k]}, w0 = f32x2{wa[k], wa[k]};
                const f32x2 x1 = f32x2{xa[k + 1], xa[k + 1]}, w1 = f32x2{wa[k + 1], wa[k + 1]};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    eA[i] = __builtin_elementwise_fma(x0, px[i + k / 2], eA[i]);
                    eW[i] = __builtin_elementwise_fma(w0, pw[i + k / 2], eW[i]);
                }
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    oA[i] = __builtin_elementwise_fma(x1, px[i + k / 2], oA[i]);
                    oW[i] = __builtin_elementwise_fma(w1, pw[i + k / 2], oW[i]);
                }
            }
        }
        __syncthreads();                                                          // the pass before has read `red`
        float *rt = red + tid * 2 * kLags;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                             // lag 2i: even then odd pixels; lag 2i + 1 likewise
            rt[2 * i] = __fadd_rn(eW[i][0], oW[i][1]);
            rt[2 * i + 1] = __fadd_rn(eW[i][1], oW[i + 1][0]);
            rt[kLags + 2 * i] = __fadd_rn(eA[i][0], oA[i][1]);
            rt[kLags + 2 * i + 1] = __fadd_rn(eA[i][1], oA[i + 1][0]);
        }
        __syncthreads();
        for (int o = tid; o < 2 * kLags * ntp; o += kThreads) {                   // o = (W | A, lag of this pass)
            const int which = o / (kLags * ntp), ll = o - which * (kLags * ntp);
            const int l = kLags * t0 + ll;
            if (l >= nlag) continue;
            const float *r = red + (ll / kLags) * 2 * kLags + which * kLags + (ll & (kLags - 1));
            float acc = r[0];
            for (int cc = 1; cc < nc; ++cc) acc = __fadd_rn(acc, r[cc * ntp * 2 * kLags]);
            out[which * nlag + l] = acc;
        }
    }
}

struct StackArgs {
    const float *pairs, *noise0;                // (Bc, S, nseg, 2, nlag), (Bc, S, nseg): k_xi's rows of this launch
    const int *code;                            // [S][n]
    double *part;                               // (chunks, S, nz, 2 + 5 nlag)
    int n, S, nseg, nlag, nz;                   // n = Bc nseg segments per draw
};

// grid (chunks of the launch x S)
static __global__ __launch_bounds__(kThreads) void k_xi_stack(const StackArgs a) {
#pragma clang fp contract(off)
    const int nlag = a.nlag, S = a.S, nseg = a.nseg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int chunk = blockIdx.x / S, s = blockIdx.x % S;
    const int e0 = chunk * kChunk;
    const int cnt = a.n - e0 < kChunk ? a.n - e0 : kChunk;                        // (>= 1: the grid has no empty chunk)
    const int cd = lane < cnt ? a.code[(int64_t)s * a.n + e0 + lane] : -1;        // every wave holds the chunk's codes
    const int64_t Wd = 2 + 5 * (int64_t)nlag;
    double *prow = a.part + (int64_t)blockIdx.x * a.nz * Wd;                      // (blockIdx.x = chunk S + s)
    for (int l0 = 0; l0 < nlag; l0 += kThreads) {                                 // (uniform trips: the ballots need every lane)
        const int l = l0 + tid;
        const bool mine = l < nlag;
        for (int kz = 0; kz < a.nz; ++kz) {
            unsigned long long hit = __ballot(cd == kz);
            double sN = 0.0, sW = 0.0, sA = 0.0, sWW = 0.0, sAW = 0.0, sAA = 0.0;
            const double cntz = (double)__popcll(hit);
            while (hit) {                                                         // (wave-uniform) hits in segment order
                const int i = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const int64_t seg = qfa_segment::chunk_segment(e0 + i, s, S, nseg);
                if (mine) {
                    const double W = (double)a.pairs[seg * 2 * nlag + l], A = (double)a.pairs[seg * 2 * nlag + nlag + l];
                    const double ww = W * W, aw = A * W, aa = A * A;
                    sW = sW + W;
                    sA = sA + A;
                    sWW = sWW + ww;
                    sAW = sAW + aw;
                    sAA = sAA + aa;
                }
                if (l == 0) sN = sN + (double)a.noise0[seg];
            }
            double *pr = prow + kz * Wd;
            if (l == 0) {
                pr[0] = cntz;
                pr[1] = sN;
            }
            if (mine) {
                pr[2 + l] = sW;
                pr[2 + nlag + l] = sA;
                pr[2 + 2 * nlag + l] = sWW;
                pr[2 + 3 * nlag + l] = sAW;
                pr[2 + 4 * nlag + l] = sAA;
            }
        }
    }
}

}  // namespace qfa_xi
