// qfa_p1d.h -- the line-of-sight flux power spectrum of forest segments and its (k, z) stack (include/qfa_hip.h, qfa_p1d_f32).
// Built in qfa_p1d.hip.
//
//   k_p1d_twiddle  tw[q] = (cos, sin)(2 pi q / L), q < L: evaluated in float64 on the exact integer q, rounded to float32 once
//   k_p1d          a block owns 16 segments (rows of the product) and kModes consecutive modes.  It walks the L pixels in chunks of
//                  kKC: (1) every thread forms delta_F = T / <T>(z) - 1 and the noise variance of four pixels of one row from trans /
//                  ivar / z / tbar (the pixel rule of qfa_segment.h) and stores the deltas to LDS -- delta_F never reaches memory; pixels past L and rows past the last
//                  segment are zeros; (2) every wave runs v_mfma_f32_16x16x4_f32 over the chunk: A = 16 rows x 4 pixels of deltas
//                  from LDS, B = 4 pixels x 16 modes of cos (one accumulator) and of sin (a second one), the twiddle of (pixel j,
//                  mode m) read from the length-L table in LDS at the exact integer (j m) mod L, carried from one K step to the next
//                  by one add and one conditional subtract.  Re and Im of a mode end in the same lane and register slot of the two
//                  accumulators: |X|^2 / L is formed in registers.  The 16 threads of a row add their noise variances (float64) and
//                  their used pixels by a butterfly; blocks of the first mode group write the noise level and the segment's z-bin code.
//   k_p1d_reduce   one block per (draw, z-bin): every wave scans the codes of the draw's segments 64 at a time, and for each hit, in
//                  segment order, thread m adds P and P P (float64) of its mode.  It starts from what `stack` holds (or 0), so that
//                  the sum does not depend on how the host cuts the batch into launches.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_segment.h"

namespace qfa_p1d {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 16;                       // segments of a block = rows of the MFMA tile
constexpr int kKC = 64;                         // pixels of a chunk: 16 rows x 64 pixels = four per thread
constexpr int kStride = kKC + 4;                // floats of an LDS row of deltas: 16-byte rows for the float4 stores, A reads two-way at worst
constexpr int kTPW = 2;                         // mode tiles of a wave: 2 x (Re, Im) = four independent accumulators
constexpr int kModes = kWaves * kTPW * 16;      // modes of a block

struct Args {
    qfa_batch_t bt;                             // redshift only: zabs, or zq1 + pix_ratio; rows
    const float *trans, *ivar;                  // (B, S, Nb)
    const float *tbar;                          // (St, nT)
    const float2 *tw;                           // (L,)
    float *power;                               // (segments of this launch, M) or NULL
    float *noise;                               // (segments of this launch,) or NULL
    int *code;                                  // [S][Bc nseg] z-bin of a valid segment, -1 otherwise; or NULL
    int b0, Bc, S, St, Nb, L, M, nseg, p_lo, min_used, nT, nz, factored;
    float zT0, inv_dzT, z0, inv_dz;
};
static_assert(qfa_segment::has_segment_fields<Args>(), "the fields qfa_segment.h reads");

static __global__ void k_p1d_twiddle(int L, float2 *__restrict__ tw) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= L) return;
    double s, c;
    sincospi(2.0 * (double)q / (double)L, &s, &c);
    tw[q] = float2{(float)c, (float)s};
}

// grid (ceil(segments / 16), ceil(max(M, 1) / kModes)); dynamic LDS: L float2 + 16 x kStride floats
__global__ __launch_bounds__(kThreads) void k_p1d(const Args a) {
    extern __shared__ __align__(16) float lds[];                                  // [deltas 16 x kStride | table L x 2]
    __shared__ int s_valid[kRows];
    const int L = a.L, M = a.M, S = a.S, nseg = a.nseg;
    float *dl = lds;
    float2 *tw = reinterpret_cast<float2 *>(lds + kRows * kStride);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < L; q += kThreads) tw[q] = a.tw[q];

    // ---- the thread's part in forming the deltas: row prow, pixels pcol .. pcol + 3 of every chunk
    const int prow = tid >> 4, pcol = (tid & 15) * 4;
    const int64_t nsegs = (int64_t)a.Bc * S * nseg;
    const int64_t q = (int64_t)blockIdx.x * kRows + prow;
    const bool rowok = q < nsegs;
    int bl = 0, s = 0, g = 0;
    if (rowok) {
        g = (int)(q % nseg);
        const int64_t rs = q / nseg;
        s = (int)(rs % S);
        bl = (int)(rs / S);
    }
    const qfa_segment::Segment sg = qfa_segment::locate(a, qfa_segment::tbar_row(a, s), bl, s, g, rowok);
    double vsum = 0.0;
    int nused = 0;

    // ---- the thread's part in the product: modes m[t] of its wave's tiles, pixel (lane >> 4) of every K step
    int idx[kTPW], step[kTPW], m[kTPW];
    f32x4 re[kTPW], im[kTPW];
#pragma unroll
    for (int t = 0; t < kTPW; ++t) {
        m[t] = ((blockIdx.y * kWaves + wave) * kTPW + t) * 16 + (lane & 15) + 1;   // (modes past M are computed and dropped)
        idx[t] = ((lane >> 4) * m[t]) % L;
        step[t] = (4 * m[t]) % L;
        re[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        im[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int j0 = 0; j0 < L; j0 += kKC) {
        __syncthreads();                                                          // the table is written; the last chunk is read
        float d4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + pcol + k;
            float d = 0.f;
            if (rowok && j < L) {
                const qfa_segment::Pixel px = qfa_segment::pixel(a, sg, j);
                const qfa_segment::Contrast c = qfa_segment::contrast(px);
                d = px.used ? c.d : 0.f;                                          // selects: nothing under the mask reaches an output
                vsum = __dadd_rn(vsum, px.used ? (double)c.v : 0.0);
                nused += px.used ? 1 : 0;
            }
            d4[k] = d;
        }
        *reinterpret_cast<float4 *>(dl + prow * kStride + pcol) = float4{d4[0], d4[1], d4[2], d4[3]};
        __syncthreads();
        const float *arow = dl + (lane & 15) * kStride + (lane >> 4);
#pragma unroll 4
        for (int kk = 0; kk < kKC; kk += 4) {
            const float av = arow[kk];
#pragma unroll
            for (int t = 0; t < kTPW; ++t) {
                const float2 cs = tw[idx[t]];
                re[t] = mfma4(av, cs.x, re[t]);
                im[t] = mfma4(av, cs.y, im[t]);
                idx[t] += step[t];
                idx[t] -= idx[t] >= L ? L : 0;
            }
        }
    }

    // ---- the row's noise level, its validity and its z-bin: the 16 threads of a row are 16 consecutive lanes
#pragma unroll
    for (int dlt = 1; dlt < 16; dlt <<= 1) {
        vsum = __dadd_rn(vsum, __shfl_xor(vsum, dlt));
        nused += __shfl_xor(nused, dlt);
    }
    const bool valid = rowok && nused >= a.min_used;
    if ((tid & 15) == 0) {
        s_valid[prow] = valid ? 1 : 0;
        if (blockIdx.y == 0 && rowok) {
            if (a.noise) a.noise[q] = valid ? (float)(vsum / (double)L) : 0.f;
            if (a.code) a.code[qfa_segment::code_slot(a.Bc, nseg, bl, s, g)] = qfa_segment::segment_code(a, sg, valid);
        }
    }
    __syncthreads();
    if (a.power) {
        const float fL = (float)L;
#pragma unroll
        for (int t = 0; t < kTPW; ++t) {
            if (m[t] > M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * (lane >> 4) + r;                                // the row of accumulator slot r
                const int64_t qq = (int64_t)blockIdx.x * kRows + i;
                if (qq >= nsegs) continue;
                const float x = re[t][r], y = im[t][r];
                const float P = __fdiv_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), fL);
                a.power[qq * M + (m[t] - 1)] = s_valid[i] ? P : 0.f;
            }
        }
    }
}

// grid (S nz, ceil(max(M, 1) / 256)).  stack (S, nz, 2 + 2M) = [n | sum N | sum P_1..M | sum P^2_1..M]; power / noise / code hold
// the n = Bc nseg segments per draw of one launch of k_p1d.
static __global__ __launch_bounds__(256) void k_p1d_reduce(const int *__restrict__ code, const float *__restrict__ power,
                                                           const float *__restrict__ noise, int Bc, int S, int nseg, int M, int nz,
                                                           int zero, double *__restrict__ stack) {
    const int s = blockIdx.x / nz, kz = blockIdx.x % nz;
    const int lane = threadIdx.x & 63;
    const int mi = blockIdx.y * 256 + threadIdx.x;
    const int n = Bc * nseg;
    const int *cs = code + (int64_t)s * n;
    double *row = stack + ((int64_t)s * nz + kz) * (2 + 2 * (int64_t)M);
    const bool lead = blockIdx.y == 0 && threadIdx.x == 0;
    const bool mine = mi < M;
    double aP = 0.0, aPP = 0.0, aN = 0.0, aC = 0.0;
    if (!zero) {
        if (mine) {
            aP = row[2 + mi];
            aPP = row[2 + M + mi];
        }
        if (lead) {
            aC = row[0];
            aN = row[1];
        }
    }
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane < n ? cs[base + lane] : -1;
        unsigned long long hit = __ballot(c == kz);
        while (hit) {                                                             // (wave-uniform) hits in segment order
            const int e = base + __ffsll((long long)hit) - 1;
            hit &= hit - 1;
            const int64_t seg = qfa_segment::chunk_segment(e, s, S, nseg);
            if (mine) {
                const double p = (double)power[seg * M + mi];
                aP = __dadd_rn(aP, p);
                aPP = __dadd_rn(aPP, __dmul_rn(p, p));
            }
            if (lead) {
                aC = __dadd_rn(aC, 1.0);
                aN = __dadd_rn(aN, (double)noise[seg]);
            }
        }
    }
    if (mine) {
        row[2 + mi] = aP;
        row[2 + M + mi] = aPP;
    }
    if (lead) {
        row[0] = aC;
        row[1] = aN;
    }
}

}  // namespace qfa_p1d
