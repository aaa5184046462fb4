// qfa_variance.h -- the variance function of the forest: the moments of delta_F of forest segments in bins of the pipeline's noise
// variance v, and their (v-bin, z) stack (include/qfa_hip.h, qfa_variance_f32).  Built in qfa_p1d.hip; the per-pixel rule, validity
// and the z-bin of a segment are qfa_segment.h's.
//
//   k_var         a block of four waves owns one segment; thread j takes the pixels j, j + 256, ...  and forms `used`, d, v and the
//                 bin code c of v (a shift and a subtraction on the bits of v: no logarithm).  Lane a of a wave keeps the five sums
//                 of bin a in registers (hence nv <= 64).  Per 64 pixels the wave reads the code of its first unserved lane, ballots
//                 the lanes that hold the same code, adds v, d, d^2 and d^4 (float64) of those lanes by a butterfly in which every
//                 other lane holds 0 -- a fixed tree over the lanes -- and lane a adds the four sums and the population count: as
//                 many rounds as there are distinct codes among the 64 pixels (noise varies smoothly along a spectrum: a few).  No
//                 LDS in the rounds, no atomics.  The waves' rows meet in LDS and are added in wave order; the segment's row
//                 [n_used | 5 nv] goes to the workspace, its 5 nv sums to `moments`.  delta_F never reaches memory.
//   k_var_stack   a block owns one chunk of 64 consecutive segments (in order of (b, g)) of one draw: per z-bin the wave ballots the
//                 chunk's codes (lane i holds segment i), and thread l adds entry l of the rows in segment order from 0; the partial
//                 row [n_seg | n_used | 5 nv] of (chunk, draw, z-bin) goes to the workspace.
// The stack (S, nz, 2 + 5 nv) is k_chunk_reduce's (qfa_segment.h) with head = 2 + 5 nv, n = 0.
// The order of every sum is a function of the segment's data and (L, nv): nothing here depends on the grid or on the cut of a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_segment.h"

namespace qfa_variance {

constexpr int kThreads = qfa_segment::kThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = qfa_segment::kChunk;     // segments of a chunk (qfa_p1d_band_chunk_segments()) = lanes of a wave
constexpr int kMaxBins = 64;                    // variance bins = lanes of a wave: lane a sums bin a
constexpr int kSums = 5;                        // [n_a | sum v | sum d | sum d^2 | sum d^4]

struct Args {
    qfa_batch_t bt;                             // redshift only: zabs, or zq1 + pix_ratio; rows
    const float *trans, *ivar;                  // (B, S, Nb)
    const float *tbar;                          // (St, nT)
    double *moments;                            // (B S, nseg, 5, nv) of the whole call, or NULL
    double *rows;                               // (segments of this launch, 1 + 5 nv) = [n_used | sums], or NULL
    int *code;                                  // [S][Bc nseg] z-bin of a valid segment, -1 otherwise; or NULL
    int b0, Bc, S, St, Nb, L, nseg, p_lo, min_used, nT, nz, factored, nv, shift, c0;       // c = (bits(v) >> shift) - c0
    float zT0, inv_dzT, z0, inv_dz, d_max;
};
static_assert(qfa_segment::has_segment_fields<Args>(), "the fields qfa_segment.h reads");

// the sum of x over the wave, every lane: a fixed tree (lanes that are not of the round hold 0, which adds exactly)
__device__ __forceinline__ double wave_sum(double x) {
#pragma clang fp contract(off)
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) x = x + __shfl_xor(x, dlt);
    return x;
}

// grid (gx, gy) with gx gy >= segments of the launch
__global__ __launch_bounds__(kThreads) void k_var(const Args a) {
#pragma clang fp contract(off)
    __shared__ double s_row[kWaves][kSums][kMaxBins];
    __shared__ int s_nu[kWaves];
    const int L = a.L, S = a.S, nseg = a.nseg, nv = a.nv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nsegs = (int64_t)a.Bc * S * nseg;
    const int64_t q = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (q >= nsegs) return;                                                       // (the whole block)
    const int g = (int)(q % nseg);
    const int64_t rs = q / nseg;
    const int s = (int)(rs % S), bl = (int)(rs / S);
    const qfa_segment::Segment sg = qfa_segment::locate(a, qfa_segment::tbar_row(a, s), bl, s, g);

    // ---- (1) the sums of the wave's pixels: lane a holds bin a
    double sn = 0.0, sv = 0.0, sd = 0.0, sd2 = 0.0, sd4 = 0.0;
    int nused = 0;
    for (int j0 = 0; j0 < L; j0 += kThreads) {                                    // (uniform trips: the ballots need every lane)
        const int j = j0 + tid;
        bool used = false;
        int c = -1;
        float d = 0.f, v = 0.f;
        if (j < L) {
            const qfa_segment::Pixel px = qfa_segment::pixel(a, sg, j);
            const qfa_segment::Contrast ct = qfa_segment::contrast(px);
            used = px.used;
            const float du = used ? ct.d : 0.f;                                   // selects: nothing under the mask reaches an output
            const float vu = used ? ct.v : 0.f;
            const int cv = (__float_as_int(vu) >> a.shift) - a.c0;                // (arithmetic shift: a negative v gets a negative code)
            const bool counted = used && cv >= 0 && cv < nv && fabsf(du) <= a.d_max;          // (a NaN d fails the cut)
            c = counted ? cv : -1;
            d = counted ? du : 0.f;
            v = counted ? vu : 0.f;
        }
        nused += __popcll(__ballot(used));
        const double xv = (double)v, xd = (double)d;
        const double xd2 = xd * xd;                                               // (exact: 24 x 24 bits)
        const double xd4 = xd2 * xd2;
        unsigned long long act = __ballot(c >= 0);
        while (act) {                                                             // (wave-uniform) one round per distinct code
            const int src = __ffsll((long long)act) - 1;
            const int ba = __builtin_amdgcn_readlane(c, src);
            const bool in = c == ba;
            const unsigned long long same = __ballot(in);                         // (holds lane src: the loop ends)
            const double tv = wave_sum(in ? xv : 0.0), td = wave_sum(in ? xd : 0.0);
            const double t2 = wave_sum(in ? xd2 : 0.0), t4 = wave_sum(in ? xd4 : 0.0);
            if (lane == ba) {
                sn = sn + (double)__popcll(same);
                sv = sv + tv;
                sd = sd + td;
                sd2 = sd2 + t2;
                sd4 = sd4 + t4;
            }
            act &= ~same;
        }
    }
    s_row[wave][0][lane] = sn;
    s_row[wave][1][lane] = sv;
    s_row[wave][2][lane] = sd;
    s_row[wave][3][lane] = sd2;
    s_row[wave][4][lane] = sd4;
    if (lane == 0) s_nu[wave] = nused;
    __syncthreads();

    // ---- (2) the waves in order
    nused = s_nu[0] + s_nu[1] + s_nu[2] + s_nu[3];
    const bool valid = nused >= a.min_used;
    const int64_t W = 1 + kSums * (int64_t)nv;
    if (tid == 0) {
        if (a.code) a.code[qfa_segment::code_slot(a.Bc, nseg, bl, s, g)] = qfa_segment::segment_code(a, sg, valid);
        if (a.rows) a.rows[q * W] = valid ? (double)nused : 0.0;
    }
    double *mo = a.moments ? a.moments + (sg.row * nseg + g) * (kSums * (int64_t)nv) : nullptr;
    for (int o = tid; o < kSums * nv; o += kThreads) {
        const int k = o / nv, cb = o - k * nv;
        double t = s_row[0][k][cb];
        t = t + s_row[1][k][cb];
        t = t + s_row[2][k][cb];
        t = t + s_row[3][k][cb];
        t = valid ? t : 0.0;                                                      // an invalid segment is exactly 0
        if (a.rows) a.rows[q * W + 1 + o] = t;
        if (mo) mo[o] = t;
    }
}

struct StackArgs {
    const double *rows;                         // (Bc, S, nseg, 1 + 5 nv): k_var's rows of this launch
    const int *code;                            // [S][n]
    double *part;                               // (chunks, S, nz, 2 + 5 nv)
    int n, S, nseg, nv, nz;                     // n = Bc nseg segments per draw
};

// grid (chunks of the launch x S)
static __global__ __launch_bounds__(kThreads) void k_var_stack(const StackArgs a) {
#pragma clang fp contract(off)
    const int S = a.S, nseg = a.nseg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int chunk = blockIdx.x / S, s = blockIdx.x % S;
    const int e0 = chunk * kChunk;
    const int cnt = a.n - e0 < kChunk ? a.n - e0 : kChunk;                        // (>= 1: the grid has no empty chunk)
    const int cd = lane < cnt ? a.code[(int64_t)s * a.n + e0 + lane] : -1;        // every wave holds the chunk's codes
    const int nsum = kSums * a.nv;
    const int64_t W = 1 + (int64_t)nsum, Wd = 2 + (int64_t)nsum;
    double *prow = a.part + (int64_t)blockIdx.x * a.nz * Wd;                      // (blockIdx.x = chunk S + s)
    for (int l0 = 0; l0 < nsum; l0 += kThreads) {                                 // (uniform trips: the ballots need every lane)
        const int l = l0 + tid;
        const bool mine = l < nsum;
        for (int kz = 0; kz < a.nz; ++kz) {
            unsigned long long hit = __ballot(cd == kz);
            const double cntz = (double)__popcll(hit);
            double acc = 0.0, sN = 0.0;
            while (hit) {                                                         // (wave-uniform) hits in segment order
                const int i = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const double *r = a.rows + qfa_segment::chunk_segment(e0 + i, s, S, nseg) * W;
                if (mine) acc = acc + r[1 + l];
                if (l == 0) sN = sN + r[0];
            }
            double *pr = prow + kz * Wd;
            if (l == 0) {
                pr[0] = cntz;
                pr[1] = sN;
            }
            if (mine) pr[2 + l] = acc;
        }
    }
}

}  // namespace qfa_variance
