// qfa_p1d_band.h -- band powers of forest segments and their covariance stack (include/qfa_hip.h, qfa_p1d_band_f32).
// Built in qfa_p1d.hip, behind k_p1d (qfa_p1d.h), whose per-segment rows (power, noise, z-bin code) it reads from the workspace.
//
//   k_p1d_band_prep    one block of 64 threads: thread a counts the modes of band a and lists them in order of m (a counting sort of
//                      the caller's `band` array), so that a band's sum walks its own modes only, whatever the map looks like
//   k_p1d_band         a block owns one chunk of kChunk consecutive segments (in order of (b, g)) of one draw.  (1) thread per
//                      (segment, band): Q_a = sum_m w_m (P_m - s N) in float64 in order of m, to LDS and to `bandpower`; a column of
//                      ones stands next to the bands, so that sum Q_a is the product (a, ones) and has no code of its own.  (2) every
//                      thread owns items of [sum Q_a | sum Q_a Q_b, a <= b]; per z-bin the wave ballots the chunk's codes (lane i holds
//                      segment i) and adds its item's products in segment order from 0; the partial row [n | items] of (chunk, draw,
//                      z-bin) goes to the workspace.  Only the upper triangle is formed: half the products and half the partials.
//   k_p1d_band_reduce  thread per entry of stack (S, nz, 1 + nband + nband^2): adds the partials in chunk order onto what `stack`
//                      holds (or 0); entries (a, b) and (b, a) read the same partials, which makes the stored matrix bit-symmetric.
// No atomics, and nothing here depends on the grid: a chunk is a fixed set of segments, its sum a fixed order of additions.
// Every product and sum is written as a plain operator under `fp contract(off)`: rounded once, never fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfa_p1d_band {

constexpr int kChunk = 64;                      // segments of a chunk = lanes of a wave: one ballot finds a z-bin's segments
constexpr int kThreads = 256;
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
            const int64_t seg = ((int64_t)(e / nseg) * S + s) * nseg + e % nseg;
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
    const int nitems = nband + nband * nb1 / 2;
    const int W = 1 + nitems;
    double *prow = a.part + (int64_t)blockIdx.x * a.nz * (int64_t)W;           // (blockIdx.x = chunk S + s)
    for (int it0 = 0; it0 < nitems; it0 += kThreads) {                            // (uniform trips: the ballots need every lane)
        const int it = it0 + tid;
        const bool mine = it < nitems;
        int ia = nband, ib = nband;
        if (mine) {
            if (it < nband) {
                ia = it;                                                          // sum Q_a = sum Q_a x 1
            } else {
                int rem = it - nband;
                ia = 0;
                while (rem >= nband - ia) {                                       // row ia of the upper triangle holds nband - ia pairs
                    rem -= nband - ia;
                    ++ia;
                }
                ib = ia + rem;
            }
        }
        const double *qa = q + ia, *qb = q + ib;
        for (int kz = 0; kz < a.nz; ++kz) {
            unsigned long long hit = __ballot(cd == kz);
            if (it == 0) prow[(int64_t)kz * W] = (double)__popcll(hit);
            double acc = 0.0;
            while (hit) {                                                         // (wave-uniform) hits in segment order
                const int i = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const double pq = qa[i * nb1] * qb[i * nb1];
                acc = acc + pq;
            }
            if (mine) prow[(int64_t)kz * W + 1 + it] = acc;
        }
    }
}

// grid (S nz, ceil((1 + nband + nband^2) / 256))
static __global__ __launch_bounds__(256) void k_p1d_band_reduce(const double *__restrict__ part, int chunks, int S, int nz, int nband,
                                                                int zero, double *__restrict__ stack) {
#pragma clang fp contract(off)
    const int j = blockIdx.y * 256 + threadIdx.x;
    const int Wf = 1 + nband + nband * nband;
    if (j >= Wf) return;
    const int W = 1 + nband + nband * (nband + 1) / 2;
    int pi = j;                                                                   // n and sum Q_a keep their places
    if (j > nband) {
        int r = (j - 1 - nband) / nband, c = (j - 1 - nband) % nband;
        if (r > c) {
            const int t = r;
            r = c;
            c = t;
        }
        pi = 1 + nband + r * nband - r * (r - 1) / 2 + (c - r);
    }
    double *out = stack + (int64_t)blockIdx.x * Wf + j;                           // blockIdx.x = s nz + kz
    const double *p = part + (int64_t)blockIdx.x * W + pi;
    const int64_t stride = (int64_t)S * nz * W;
    double acc = zero ? 0.0 : *out;
    for (int c = 0; c < chunks; ++c) acc = acc + p[c * stride];
    *out = acc;
}

}  // namespace qfa_p1d_band
