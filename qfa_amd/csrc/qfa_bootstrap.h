// qfa_bootstrap.h -- the sightline (Poisson) bootstrap of the per-segment rows of the segment statistics (include/qfa_hip.h,
// qfa_segment_codes_f32 / qfa_bootstrap_f64).  k_segment_codes is launched from qfa_p1d.hip (its checks and segment fields are
// qfa_p1d_f32's), k_bootstrap from qfa_bootstrap.hip.
//
//   k_segment_codes  a wave owns one segment: 64 pixels at a time through the pixel rule of qfa_segment.h, n_used by ballots, the code
//                    by segment_code -- the z-bin qfa_p1d_f32 stacks the segment in, or -1.  Nothing of the rule is restated here.
//   k_bootstrap      the product boot[s, :, kz, :] = Wgt (R x n) X (n x (1 + W)) in float64 on the vector pipe, the weight matrix never
//                    stored.  A block is one wave; it owns one (draw, z-bin), kCols columns of [1 | x] and 256 replicates: lane l owns
//                    the four replicates of one Philox call (counter word 0x40000000 | (r >> 2)) and kCols columns of them, 4 x kCols
//                    float64 accumulators in registers.  The wave walks the draw's segments 64 at a time in order of (b, g), ballots the
//                    codes against its z-bin -- lane l fetches the kCols values of segment l when it is a hit, 64 fetches in flight
//                    together -- and, per hit in segment order, reads the hit's values from its lane (v_readlane: wave-uniform),
//                    draws the lane's four weights and issues 4 x kCols fused multiply-adds: w x is never rounded on its own
//                    (for float32 and int32 rows it is exact anyway), the additions are the only roundings.  The accumulators start
//                    from what `boot` holds (or 0): every element is ONE chain of additions in segment order over all the calls that
//                    add into it, which is why the result does not depend on how a batch is cut.  No atomics, no LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_segment.h"

namespace qfa_bootstrap {

constexpr int kCodeThreads = 256;               // k_segment_codes: four waves, a segment each
constexpr int kThreads = 64;                    // k_bootstrap: one wave
constexpr int kCols = 4;                        // columns of [1 | x] of a block of k_bootstrap
constexpr int kQuadsPerBlock = kThreads;        // replicate quads of a block: 256 replicates

struct CodeArgs {
    qfa_batch_t bt;                             // redshift only: zabs, or zq1 + pix_ratio; rows
    const float *trans, *ivar;                  // (B, S, Nb)
    const float *tbar;                          // (St, nT)
    int *codes;                                 // (B S, nseg)
    int b0, Bc, S, St, Nb, L, nseg, p_lo, min_used, nT, nz, factored;
    float zT0, inv_dzT, z0, inv_dz;
};
static_assert(qfa_segment::has_segment_fields<CodeArgs>(), "the fields qfa_segment.h reads");

// grid (ceil(segments / 4)); segment q = (b S + s) nseg + g
static __global__ __launch_bounds__(kCodeThreads) void k_segment_codes(const CodeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (kCodeThreads / 64) + wave;
    if (q >= (int64_t)a.Bc * a.S * a.nseg) return;                                // (the whole wave)
    const int g = (int)(q % a.nseg);
    const int64_t rs = q / a.nseg;
    const int s = (int)(rs % a.S), bl = (int)(rs / a.S);
    const qfa_segment::Segment sg = qfa_segment::locate(a, qfa_segment::tbar_row(a, s), bl, s, g);
    int nused = 0;
    for (int j0 = 0; j0 < a.L; j0 += 64) {
        const int j = j0 + lane;
        const bool used = j < a.L && qfa_segment::pixel(a, sg, j).used;
        nused += __popcll(__ballot(used));
    }
    const int code = qfa_segment::segment_code(a, sg, nused >= a.min_used);
    if (lane == 0) a.codes[q] = code;
}

// Philox4x32-10: the rounds and constants of qfa_sample.h's generator (Random123's philox4x32_10), which that header keeps beside
// kernels of its own translation unit
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Poisson(1) by inversion on a 32-bit word: the number of T_k <= u, T_k = floor(2^32 sum_{i <= k} e^-1 / i!), k = 0 .. 12
__device__ __forceinline__ double poisson1(uint32_t u) {
    constexpr uint32_t T[13] = {0x5e2d58d8u, 0xbc5ab1b1u, 0xeb715e1du, 0xfb239797u, 0xff1025f5u, 0xffd90f3bu, 0xfffa8b71u,
                                0xffff540cu, 0xffffed1fu, 0xfffffe21u, 0xffffffd4u, 0xfffffffcu, 0xffffffffu};
    int w = 0;
#pragma unroll
    for (int k = 0; k < 13; ++k) w += u >= T[k] ? 1 : 0;
    return (double)w;
}

// the value lane `src` (wave-uniform) holds
__device__ __forceinline__ double read_lane(double v, int src) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <typename T>
struct Args {
    const T *rows;                              // (B S, nseg, W)
    const int *codes;                           // (B S, nseg)
    double *boot;                               // (S, R, nz, 1 + W)
    int n, S, nseg, W, nz, R, zero;             // n = B nseg: the segments of a draw
    uint32_t k0, k1;
    int64_t row0;                               // the global row of spectrum 0
};

// grid (S nz ceil((1 + W) / kCols), ceil(R / 256))
template <typename T>
__global__ __launch_bounds__(kThreads) void k_bootstrap(const Args<T> a) {
    const int Wf = a.W + 1;
    const int ntile = (Wf + kCols - 1) / kCols;
    const int tile = blockIdx.x % ntile, skz = blockIdx.x / ntile;
    const int kz = skz % a.nz, s = skz / a.nz;
    const int lane = threadIdx.x;
    const int quad = blockIdx.y * kQuadsPerBlock + lane;                          // replicates 4 quad .. 4 quad + 3
    const int c0 = tile * kCols;
    double acc[4][kCols];
    double *out = a.boot + (((int64_t)s * a.R + 4 * (int64_t)quad) * a.nz + kz) * Wf + c0;
    const int64_t rstride = (int64_t)a.nz * Wf;                                   // from a replicate to the next
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < kCols; ++j) {
            const bool mine = 4 * quad + i < a.R && c0 + j < Wf;
            acc[i][j] = (mine && !a.zero) ? out[i * rstride + j] : 0.0;
        }
    for (int base = 0; base < a.n; base += 64) {
        const int el = base + lane;
        const int c = el < a.n ? a.codes[qfa_segment::chunk_segment(el, s, a.S, a.nseg)] : -1;
        // lane l fetches the columns of entry base + l when it is a hit: the 64 fetches are in flight together, the walk below reads
        // registers (a row whose code is not kz is never read)
        double xl[kCols];
        const T *xr = a.rows + (c == kz ? qfa_segment::chunk_segment(el, s, a.S, a.nseg) * a.W : 0);
#pragma unroll
        for (int j = 0; j < kCols; ++j) {                                         // column 0 of [1 | x] is the one; past 1 + W nothing
            const int col = c0 + j;
            xl[j] = col == 0 ? 1.0 : ((c == kz && col < Wf) ? (double)xr[col - 1] : 0.0);
        }
        unsigned long long hit = __ballot(c == kz);
        while (hit) {                                                             // (wave-uniform) hits in segment order
            const int i0 = __ffsll((long long)hit) - 1;
            hit &= hit - 1;
            double x[kCols];
#pragma unroll
            for (int j = 0; j < kCols; ++j) x[j] = read_lane(xl[j], i0);
            const uint64_t g = (uint64_t)(a.row0 + (base + i0) / a.nseg);
            uint32_t ctr[4] = {0x40000000u | (uint32_t)quad, 0u, (uint32_t)g, (uint32_t)(g >> 32)};
            philox4x32_10(ctr, a.k0, a.k1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double w = poisson1(ctr[i]);
#pragma unroll
                for (int j = 0; j < kCols; ++j) acc[i][j] = __fma_rn(w, x[j], acc[i][j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < kCols; ++j)
            if (4 * quad + i < a.R && c0 + j < Wf) out[i * rstride + j] = acc[i][j];
}

}  // namespace qfa_bootstrap
