// qfa_segment.h -- what the kernels of the four segment statistics share (include/qfa_hip.h: qfa_p1d_f32, qfa_p1d_band_f32, qfa_xi_f32,
// qfa_flux_pdf_f32), so that "the same pixels, the same valid segments, the same z-bin of a segment" has one definition:
//
//   locate                segment (bl, s, g) of a launch -> its rows of trans / ivar / z / tbar
//   pixel, contrast       the per-pixel rule: T, ivar, <T>(z) and `used`; delta_F = T / <T> - 1 and its noise variance
//   segment_code          the z-bin of a valid segment's central pixel, or -1; code_slot: where a launch keeps it
//   chunk_segment         entry e of draw s of a launch -> its segment row
//   tri_unpack, tri_pack  the packed upper triangle of an n x n matrix, both directions
//   chunk_products        step 2 of k_p1d_band and of k_pdf: a chunk's sums [n | sums | products a <= b] per z-bin, by ballots
//   k_chunk_reduce        thread per entry of a stack (S, nz, head + n^2): adds the chunk partials in chunk order onto what `stack`
//                         holds (or 0); entries (a, b) and (b, a) read the same partials, which makes the stored matrix bit-symmetric
// The float32 arithmetic is written with the explicit round-to-nearest intrinsics only: it means the same inside and outside
// `fp contract(off)`.  No atomics, and nothing here depends on the grid: a chunk is a fixed set of segments, its sum a fixed order
// of additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qfa_common.h"

namespace qfa_segment {

constexpr int kChunk = 64;                      // segments of a chunk = lanes of a wave: one ballot finds a z-bin's segments
constexpr int kThreads = 256;                   // threads of a block of the chunk kernels

// The functions below take the kernel's own argument struct `A` (the Args of k_p1d, k_xi and k_pdf), which holds the fields that
// has_segment_fields names, wherever the kernel keeps them: each kernel's argument layout is its own.  The host fills them in one
// place (seg_args, qfa_p1d.hip).
template <typename A>
constexpr bool has_segment_fields() {
    using std::is_same_v;
    return is_same_v<decltype(A::bt), qfa_batch_t> &&                             // redshift only: zabs, or zq1 + pix_ratio; rows
           is_same_v<decltype(A::trans), const float *> && is_same_v<decltype(A::ivar), const float *> &&        // (B, S, Nb)
           is_same_v<decltype(A::tbar), const float *> &&                                                           // (St, nT)
           is_same_v<decltype(A::b0), int> && is_same_v<decltype(A::Bc), int> && is_same_v<decltype(A::S), int> &&
           is_same_v<decltype(A::St), int> && is_same_v<decltype(A::Nb), int> && is_same_v<decltype(A::L), int> &&
           is_same_v<decltype(A::nseg), int> && is_same_v<decltype(A::p_lo), int> && is_same_v<decltype(A::min_used), int> &&
           is_same_v<decltype(A::nT), int> && is_same_v<decltype(A::nz), int> && is_same_v<decltype(A::factored), int> &&
           is_same_v<decltype(A::zT0), float> && is_same_v<decltype(A::inv_dzT), float> && is_same_v<decltype(A::z0), float> &&
           is_same_v<decltype(A::inv_dz), float>;
}

struct Segment {
    const float *tr, *iv, *zr, *tb;             // the segment's pixels of trans, ivar and z (or pix_ratio); the draw's row of tbar
    float zq;                                   // zq1 of the spectrum (factored form)
    int64_t row;                                // b S + s
};

// the row of tbar that draw s is divided by
template <typename A>
__device__ __forceinline__ const float *tbar_row(const A &a, int s) {
    return a.tbar + (int64_t)(a.St == 1 ? 0 : s) * a.nT;
}

// segment g of draw s of spectrum b0 + bl, `tb` = tbar_row(a, s) (a kernel whose blocks own one draw forms it once); `ok` false (a
// row past the last segment): pointers that are never read through
template <typename A>
__device__ __forceinline__ Segment locate(const A &a, const float *tb, int bl, int s, int g, bool ok = true) {
    Segment sg;
    const int b = a.b0 + bl;
    const unsigned long long zrow = ok ? batch_row(a.bt, b) : 0ull;
    sg.zq = (ok && a.factored) ? a.bt.zq1[zrow] : 0.f;
    const int pseg = a.p_lo + g * a.L;                                            // the segment's first pixel
    sg.row = (int64_t)b * a.S + s;
    sg.tr = a.trans + sg.row * a.Nb + pseg;
    sg.iv = a.ivar + sg.row * a.Nb + pseg;
    sg.tb = tb;
    sg.zr = a.factored ? a.bt.pix_ratio + pseg : a.bt.zabs + zrow * (unsigned long long)a.Nb + (unsigned)pseg;
    return sg;
}

template <typename A>
__device__ __forceinline__ float redshift(const A &a, const Segment &sg, int j) {
    return a.factored ? __fmaf_rn(sg.zq, sg.zr[j], -1.0f) : sg.zr[j];
}

// a pixel is used when it has weight and a mean transmission to divide by (a NaN tbar fails the comparison)
__device__ __forceinline__ bool pixel_used(float ivar, float tbar) { return ivar > 0.f && tbar > 0.f; }

struct Pixel {
    float T, ivar, tbar;
    bool used;
};

template <typename A>
__device__ __forceinline__ Pixel pixel(const A &a, const Segment &sg, int j) {
    const float T = sg.tr[j], w = sg.iv[j];
    const float kf = floorf(__fmul_rn(__fsub_rn(redshift(a, sg, j), a.zT0), a.inv_dzT));
    float tb = 0.f;
    if (kf >= 0.f && kf < (float)a.nT) tb = sg.tb[(int)kf];                       // (a NaN fails both)
    return Pixel{T, w, tb, pixel_used(w, tb)};
}

struct Contrast {
    float d, v;                                 // delta_F and its noise variance; the caller masks both by `used`
};

__device__ __forceinline__ Contrast contrast(const Pixel &p) {
    return Contrast{__fsub_rn(__fdiv_rn(p.T, p.tbar), 1.0f), __fdiv_rn(1.0f, __fmul_rn(p.ivar, __fmul_rn(p.tbar, p.tbar)))};
}

template <typename A>
__device__ __forceinline__ int segment_code(const A &a, const Segment &sg, bool valid) {
    const float kf = floorf(__fmul_rn(__fsub_rn(redshift(a, sg, a.L / 2), a.z0), a.inv_dz));
    const bool in = valid && kf >= 0.f && kf < (float)a.nz;
    return in ? (int)kf : -1;
}

// code [S][Bc nseg] of a launch: the place of segment (bl, s, g)
__device__ __forceinline__ int64_t code_slot(int Bc, int nseg, int bl, int s, int g) {
    return (int64_t)s * ((int64_t)Bc * nseg) + (int64_t)bl * nseg + g;
}

// entry e (in order of (b, g)) of draw s -> its row of the launch's per-segment arrays (Bc, S, nseg)
__device__ __forceinline__ int64_t chunk_segment(int e, int s, int S, int nseg) {
    return ((int64_t)(e / nseg) * S + s) * nseg + e % nseg;
}

// item t of the packed upper triangle -> (ia, ib), ia <= ib: row ia holds n - ia pairs
__device__ __forceinline__ void tri_unpack(int t, int n, int &ia, int &ib) {
    ia = 0;
    while (t >= n - ia) {
        t -= n - ia;
        ++ia;
    }
    ib = ia + t;
}

// entry (r, c) of the full matrix -> its item of the packed upper triangle
__device__ __forceinline__ int tri_pack(int r, int c, int n) { return r <= c ? pair_index(r, c, n) : pair_index(c, r, n); }

// A chunk's LDS rows [kChunk][nw] = [x_0 .. x_{n-1} | EXTRA further columns | 1], nw = n + EXTRA + 1, and the z-bin code `cd` of
// segment `lane` (-1 behind the chunk's last): every thread owns items of [sum of the further columns | sum x_a | sum x_a x_b, a <= b],
// a sum being the product with the column of ones; per z-bin the wave ballots the codes and adds its item's products in segment order
// from 0.  The partial row [n_segments | items] of (block = chunk S + s, z-bin) goes to part (blocks, nz, W), W = 1 + EXTRA + n +
// n (n + 1) / 2.  T = double: each product and sum a plain operator, rounded once, never fused.  Called by the whole block (the
// ballots need every lane).
template <typename T, int EXTRA>
__device__ __forceinline__ void chunk_products(const T *rows, int n, int nz, int cd, T *part) {
#pragma clang fp contract(off)
    const int one = n + EXTRA, nw = one + 1;
    const int nitems = one + n * (n + 1) / 2;
    const int W = 1 + nitems;
    T *prow = part + (int64_t)blockIdx.x * nz * (int64_t)W;
    for (int it0 = 0; it0 < nitems; it0 += kThreads) {                            // (uniform trips)
        const int it = it0 + (int)threadIdx.x;
        const bool mine = it < nitems;
        int ia = one, ib = one;
        if (mine) {
            if (it < EXTRA) ia = n + it;
            else if (it < one) ia = it - EXTRA;
            else tri_unpack(it - EXTRA - n, n, ia, ib);
        }
        const T *qa = rows + ia, *qb = rows + ib;
        for (int kz = 0; kz < nz; ++kz) {
            unsigned long long hit = __ballot(cd == kz);
            if (it == 0) prow[(int64_t)kz * W] = (T)__popcll(hit);
            T acc = 0;
            while (hit) {                                                         // (wave-uniform) hits in segment order
                const int i = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const T pq = qa[i * nw] * qb[i * nw];
                acc = acc + pq;
            }
            if (mine) prow[(int64_t)kz * W + 1 + it] = acc;
        }
    }
}

// grid (S nz, ceil((head + n^2) / 256)); part (chunks, S, nz, head + n (n + 1) / 2).  n = 0: every entry keeps its place.
template <typename T>
static __global__ __launch_bounds__(256) void k_chunk_reduce(const T *__restrict__ part, int chunks, int S, int nz, int head, int n,
                                                             int zero, double *__restrict__ stack) {
#pragma clang fp contract(off)
    const int j = blockIdx.y * 256 + threadIdx.x;
    const int Wf = head + n * n;
    if (j >= Wf) return;
    const int W = head + n * (n + 1) / 2;
    const int pi = j < head ? j : head + tri_pack((j - head) / n, (j - head) % n, n);
    double *out = stack + (int64_t)blockIdx.x * Wf + j;                           // blockIdx.x = s nz + kz
    const T *p = part + (int64_t)blockIdx.x * W + pi;
    const int64_t stride = (int64_t)S * nz * W;
    double acc = zero ? 0.0 : *out;
    for (int c = 0; c < chunks; ++c) acc = acc + (double)p[c * stride];           // (int: below 2^53, exact in any order)
    *out = acc;
}

}  // namespace qfa_segment
