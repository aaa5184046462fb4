// qfa_pdf.h -- the probability distribution of the transmitted flux of forest segments, P(F), and the stack its covariance matrix
// comes from (include/qfa_hip.h, qfa_flux_pdf_f32).  Built in qfa_p1d.hip; `used`, validity and the z-bin of a segment are k_p1d's
// (qfa_p1d.h).
//
//   k_pdf         a block of four waves owns one chunk of kChunk consecutive segments (in order of (b, g)) of one draw and reads
//                 trans / ivar itself.  (1) A wave takes every fourth segment of the chunk and walks it 64 pixels at a time: a lane
//                 forms `used`, `counted` and the bin of its pixel; lane a keeps the count of bin a in a register (hence nt <= 64).
//                 Per 64 pixels the wave reads the bin of its first still-active lane, ballots the lanes that hold the same bin, lane
//                 a adds the population count, the lanes leave: as many rounds as there are distinct bins among the 64 pixels, no
//                 LDS, no atomics.  n_used and n_cnt are population counts of two more ballots.  The segment's row
//                 [h_0 .. h_{nt-1} | n_cnt | 1] goes to LDS (the column of ones makes sum h_a a product like the others) and h to
//                 `hist`.  (2) k_p1d_band's step (2) on integers: every thread owns items of [sum n_cnt | sum h_a | sum h_a h_b,
//                 a <= b]; per z-bin the wave ballots the chunk's codes (lane i holds segment i) and adds its item's products; the
//                 partial row [n | items] of (chunk, draw, z-bin) goes to the workspace as int32 -- a chunk's sums stay below
//                 64 x 4096^2 = 2^30.
//   k_pdf_reduce  thread per entry of stack (S, nz, 2 + nt + nt^2): adds the partials in chunk order, as float64, onto what `stack`
//                 holds (or 0); entries (a, b) and (b, a) read the same partials.
// Every term is an integer: the sums are exact (below 2^53) and do not depend on any order.  No atomics all the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_p1d_band.h"

namespace qfa_pdf {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = qfa_p1d_band::kChunk;    // segments of a chunk (qfa_p1d_band_chunk_segments()) = lanes of a wave
constexpr int kMaxBins = 64;                    // flux bins = lanes of a wave: lane a counts bin a

struct Args {
    qfa_batch_t bt;                             // redshift only: zabs, or zq1 + pix_ratio; rows
    const float *trans, *ivar;                  // (B, S, Nb)
    const float *tbar;                          // (St, nT)
    int *hist;                                  // (B S, nseg, nt) of the whole call, or NULL
    int *part;                                  // (chunks, S, nz, 2 + nt + nt (nt + 1) / 2) of this launch, or NULL
    int b0, Bc, S, St, Nb, L, nseg, p_lo, min_used, nT, nz, factored, nt, relative, clamp;
    float zT0, inv_dzT, z0, inv_dz, t0, inv_dt, ivar_min;
};

// grid (chunks of the launch x S); dynamic LDS: kChunk x (nt + 2) ints
__global__ __launch_bounds__(kThreads) void k_pdf(const Args a) {
    extern __shared__ __align__(16) int hs[];                                     // [kChunk][nt + 2] = [h | n_cnt | 1]
    __shared__ int s_code[kChunk];
    const int L = a.L, S = a.S, Nb = a.Nb, nseg = a.nseg, nt = a.nt, nw = nt + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / S, s = blockIdx.x % S;
    const int n = a.Bc * nseg;                                                    // segments per draw of this launch
    const int e0 = chunk * kChunk;
    const int cnt = n - e0 < kChunk ? n - e0 : kChunk;                            // (>= 1: the grid has no empty chunk)
    const float *tb = a.tbar + (int64_t)(a.St == 1 ? 0 : s) * a.nT;
    const float fnT = (float)a.nT, fnt = (float)nt;

    // ---- (1) the counts of the wave's segments
    for (int i = wave; i < cnt; i += kWaves) {
        const int e = e0 + i;
        const int bl = e / nseg, g = e - bl * nseg;
        const int b = a.b0 + bl;
        const unsigned long long zrow = batch_row(a.bt, b);
        const float zq = a.factored ? a.bt.zq1[zrow] : 0.f;
        const int pseg = a.p_lo + g * L;                                          // the segment's first pixel
        const int64_t row = (int64_t)b * S + s;
        const float *tr = a.trans + row * Nb + pseg;
        const float *iv = a.ivar + row * Nb + pseg;
        const float *zr = a.factored ? a.bt.pix_ratio + pseg : a.bt.zabs + zrow * (unsigned long long)Nb + (unsigned)pseg;
        int h = 0, nused = 0, ncnt = 0;
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            bool used = false, counted = false;
            int bin = -1;
            if (j < L) {
#pragma clang fp contract(off)
                const float T = tr[j], wi = iv[j];
                const float z = a.factored ? __fmaf_rn(zq, zr[j], -1.0f) : zr[j];
                const float kf = floorf(__fmul_rn(__fsub_rn(z, a.zT0), a.inv_dzT));
                float tbv = 0.f;
                if (kf >= 0.f && kf < fnT) tbv = tb[(int)kf];                     // (a NaN fails both)
                used = wi > 0.f && tbv > 0.f;                                     // (a NaN tbar fails the comparison)
                counted = used && wi >= a.ivar_min;
                const float x = a.relative ? __fdiv_rn(T, tbv) : T;
                const float fa = floorf(__fmul_rn(__fsub_rn(x, a.t0), a.inv_dt));
                int k = -1;                                                       // (a NaN fa fails every comparison: no bin)
                if (fa >= 0.f && fa < fnt) k = (int)fa;
                else if (a.clamp && fa < 0.f) k = 0;
                else if (a.clamp && fa >= fnt) k = nt - 1;
                bin = counted ? k : -1;                                           // selects: nothing under the mask reaches an output
            }
            nused += __popcll(__ballot(used));
            ncnt += __popcll(__ballot(counted));
            unsigned long long act = __ballot(bin >= 0);
            while (act) {                                                         // (wave-uniform) one round per distinct bin
                const int src = __ffsll((long long)act) - 1;
                const int ba = __builtin_amdgcn_readlane(bin, src);
                const unsigned long long same = __ballot(bin == ba);              // (holds lane src: the loop ends)
                h += lane == ba ? __popcll(same) : 0;
                act &= ~same;
            }
        }
        const bool valid = nused >= a.min_used;
        h = valid ? h : 0;
        const int jc = L / 2;
        const float zc = a.factored ? __fmaf_rn(zq, zr[jc], -1.0f) : zr[jc];
        const float kf = floorf(__fmul_rn(__fsub_rn(zc, a.z0), a.inv_dz));
        const bool in = valid && kf >= 0.f && kf < (float)a.nz;
        if (a.hist && lane < nt) a.hist[(row * nseg + g) * nt + lane] = h;
        int *hr = hs + i * nw;
        if (lane < nt) hr[lane] = h;
        if (lane == 0) {
            hr[nt] = valid ? ncnt : 0;
            hr[nt + 1] = 1;
            s_code[i] = in ? (int)kf : -1;
        }
    }
    if (!a.part) return;
    __syncthreads();

    // ---- (2) the chunk's sums per z-bin
    const int cd = lane < cnt ? s_code[lane] : -1;                                // every wave holds the chunk's codes
    const int nitems = 1 + nt + nt * (nt + 1) / 2;
    const int W = 1 + nitems;
    int *prow = a.part + (int64_t)blockIdx.x * a.nz * (int64_t)W;              // (blockIdx.x = chunk S + s)
    for (int it0 = 0; it0 < nitems; it0 += kThreads) {                            // (uniform trips: the ballots need every lane)
        const int it = it0 + tid;
        const bool mine = it < nitems;
        int ia = nt + 1, ib = nt + 1;
        if (mine) {
            if (it == 0) {
                ia = nt;                                                          // sum n_cnt = sum n_cnt x 1
            } else if (it <= nt) {
                ia = it - 1;                                                      // sum h_a = sum h_a x 1
            } else {
                int rem = it - 1 - nt;
                ia = 0;
                while (rem >= nt - ia) {                                          // row ia of the upper triangle holds nt - ia pairs
                    rem -= nt - ia;
                    ++ia;
                }
                ib = ia + rem;
            }
        }
        const int *qa = hs + ia, *qb = hs + ib;
        for (int kz = 0; kz < a.nz; ++kz) {
            unsigned long long hit = __ballot(cd == kz);
            if (it == 0) prow[(int64_t)kz * W] = __popcll(hit);
            int acc = 0;
            while (hit) {                                                         // (wave-uniform)
                const int i = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                acc += qa[i * nw] * qb[i * nw];
            }
            if (mine) prow[(int64_t)kz * W + 1 + it] = acc;
        }
    }
}

// grid (S nz, ceil((2 + nt + nt^2) / 256))
static __global__ __launch_bounds__(256) void k_pdf_reduce(const int *__restrict__ part, int chunks, int S, int nz, int nt, int zero,
                                                           double *__restrict__ stack) {
    const int j = blockIdx.y * 256 + threadIdx.x;
    const int Wf = 2 + nt + nt * nt;
    if (j >= Wf) return;
    const int W = 2 + nt + nt * (nt + 1) / 2;
    int pi = j;                                                                   // n, sum n_cnt and sum h_a keep their places
    if (j >= 2 + nt) {
        int r = (j - 2 - nt) / nt, c = (j - 2 - nt) % nt;
        if (r > c) {
            const int t = r;
            r = c;
            c = t;
        }
        pi = 2 + nt + r * nt - r * (r - 1) / 2 + (c - r);
    }
    double *out = stack + (int64_t)blockIdx.x * Wf + j;                           // blockIdx.x = s nz + kz
    const int *p = part + (int64_t)blockIdx.x * W + pi;
    const int64_t stride = (int64_t)S * nz * W;
    double acc = zero ? 0.0 : *out;
    for (int c = 0; c < chunks; ++c) acc += (double)p[c * stride];                // (integers below 2^53: exact in any order)
    *out = acc;
}

}  // namespace qfa_pdf
