// qfa_p1d_band.h -- band powers of forest segments and their covariance stack (include/qfa_hip.h, qfa_p1d_band_f32).
// Built in qfa_p1d.hip, behind k_p1d (qfa_p1d.h), whose per-segment rows (power, noise, z-bin code) it reads from the workspace.
//
//   k_p1d_band_prep    one block of 64 threads: thread a counts the modes of band a and lists them in order of m (a counting sort of
//                      the caller's `band` array), so that a band's sum walks its own modes only, whatever the map looks like
//   k_p1d_band         a block owns one chunk of kChunk consecutive segments (in order of (b, g)) of one draw.  (1) thread per
//                      (segment, band): Q_a = sum_m w_m (P_m - s N) in float64 in order of m, to LDS and to `bandpower`; a column of
//                      ones stands next to the bands, so that sum Q_a is the product (a, ones) and has no code of its own.  (2)
//                      chunk_products (qfa_segment.h): every thread owns items of [sum Q_a | sum Q_a Q_b, a <= b]; per z-bin the wave
//                      ballots the chunk's codes (lane i holds segment i) and adds its item's products in segment order from 0; the
//                      partial row [n | items] of (chunk, draw, z-bin) goes to the workspace.  Only the upper triangle is formed: half
//                      the products and half the partials.
// The stack (S, nz, 1 + nband + nband^2) is k_chunk_reduce's (qfa_segment.h) with head = 1 + nband, n = nband.
// No atomics, and nothing here depends on the grid: a chunk is a fixed set of segments, its sum a fixed order of additions.
// Every product and sum is written as a plain operator under `fp contract(off)`: rounded once, never fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_segment.h"

namespace qfa_p1d_band {

constexpr int kChunk = qfa_segment::kChunk;     // segments of a chunk (qfa_p1d_band_chunk_segments()) = lanes of a wave
constexpr int kThreads = qfa_segment::kThreads;
constexpr int kMaxBands = 64;

struct Args {
    const float *power, *noise;                 // (Bc, S, nseg, M), (Bc, S, nseg): k_p1d's rows of this launch
    const int *code;                            // [S][n]
    const int *start, *list;                    // (nband + 1,), (M,): k_p1d_band_prep
    const float *weight;                        // (M,) or NULL
    double *bandpower;                          // rows of this launch's segments, or NULL
    double *part;                               // (chunks, S, nz, 1 + nband + nband (nband + 1) / 2), or NULL
    int n, S, nseg, M, nband, nz, sub;          // n = Bc nseg segments per draw
};

static __global__ __launch_bounds__(kMaxBands) void k_p1d_band_prep(const int *__restrict__ band, int M, int nband,
                                                                    int *__restrict__ start, int *__restrict__ list) {
    __shared__ int cnt[kMaxBands];
    const int a = threadIdx.x;
    int c = 0;
    if (a < nband)
        for (int m = 0; m < M; ++m) c += band[m] == a ? 1 : 0;
    cnt[a] = c;
    __syncthreads();
    if (a >= nband) return;
    int off = 0;
    for (int r = 0; r < a; ++r) off += cnt[r];
    start[a] = off;
    if (a == nband - 1) start[nband] = off + c;
    for (int m = 0; m < M; ++m)
        if (band[m] == a) list[off++] = m;      // (off stays below start[a + 1] <= M: the same count as above)
}

// grid (chunks of the launch x S); dynamic LDS: kChunk x (nband + 1) doubles
static __global__ __launch_bounds__(kThreads) void k_p1d_band(const Args a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) double q[];                                   // [kChunk][nband + 1], the last column ones
    const int nband = a.nband, nb1 = nband + 1, M = a.M, S = a.S, nseg = a.nseg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int chunk = blockIdx.x / S, s = blockIdx.x % S;
    const int e0 = chunk * kChunk;
    const int cnt = a.n - e0 < kChunk ? a.n - e0 : kChunk;                        // (>= 1: the grid has no empty chunk)
    const double sub = (double)a.sub;

    for (int t = tid; t < kChunk * nb1; t += kThreads) {
        const int i = t / nb1, b = t - i * nb1;
        double Q = 0.0;
        if (b == nband) {
            Q = 1.0;
        } else if (i < cnt) {
            const int e = e0 + i;
            const int64_t seg = qfa_segment::chunk_segment(e, s, S, nseg);
            const float *pr = a.power + seg * M;
            const double sN = sub * (double)a.noise[seg];
            const int k1 = a.start[b + 1];
            for (int k = a.start[b]; k < k1; ++k) {
                const int m = a.list[k];
                const double w = a.weight ? (double)a.weight[m] : 1.0;
                const double x = (double)pr[m] - sN;
                const double wx = w * x;
                Q = Q + wx;                                                       // (an invalid segment: P = N = 0, Q stays +0)
            }
            if (a.bandpower) a.bandpower[seg * nband + b] = Q;
        }
        q[t] = Q;
    }
    if (!a.part) return;
    __syncthreads();

    const int cd = lane < cnt ? a.code[(int64_t)s * a.n + e0 + lane] : -1;        // every wave holds the chunk's codes
    qfa_segment::chunk_products<double, 0>(q, nband, a.nz, cd, a.part);
}

}  // namespace qfa_p1d_band
