// qfa_pdf.h -- the probability distribution of the transmitted flux of forest segments, P(F), and the stack its covariance matrix
// comes from (include/qfa_hip.h, qfa_flux_pdf_f32).  Built in qfa_p1d.hip; `used`, validity and the z-bin of a segment are
// qfa_segment.h's.
//
//   k_pdf         a block of four waves owns one chunk of kChunk consecutive segments (in order of (b, g)) of one draw and reads
//                 trans / ivar itself.  (1) A wave takes every fourth segment of the chunk and walks it 64 pixels at a time: a lane
//                 forms `used`, `counted` and the bin of its pixel; lane a keeps the count of bin a in a register (hence nt <= 64).
//                 Per 64 pixels the wave reads the bin of its first still-active lane, ballots the lanes that hold the same bin, lane
//                 a adds the population count, the lanes leave: as many rounds as there are distinct bins among the 64 pixels, no
//                 LDS, no atomics.  n_used and n_cnt are population counts of two more ballots.  The segment's row
//                 [h_0 .. h_{nt-1} | n_cnt | 1] goes to LDS (the column of ones makes sum h_a a product like the others) and h to
//                 `hist`.  (2) chunk_products (qfa_segment.h) on integers: every thread owns items of [sum n_cnt | sum h_a | sum h_a h_b,
//                 a <= b]; per z-bin the wave ballots the chunk's codes (lane i holds segment i) and adds its item's products; the
//                 partial row [n | items] of (chunk, draw, z-bin) goes to the workspace as int32 -- a chunk's sums stay below
//                 64 x 4096^2 = 2^30.
// The stack (S, nz, 2 + nt + nt^2) is k_chunk_reduce's (qfa_segment.h) on the int32 partials with head = 2 + nt, n = nt.
// Every term is an integer: the sums are exact (below 2^53) and do not depend on any order.  No atomics all the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qfa_common.h"
#include "qfa_segment.h"

namespace qfa_pdf {

constexpr int kThreads = qfa_segment::kThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = qfa_segment::kChunk;     // segments of a chunk (qfa_p1d_band_chunk_segments()) = lanes of a wave
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
static_assert(qfa_segment::has_segment_fields<Args>(), "the fields qfa_segment.h reads");

// grid (chunks of the launch x S); dynamic LDS: kChunk x (nt + 2) ints
__global__ __launch_bounds__(kThreads) void k_pdf(const Args a) {
    extern __shared__ __align__(16) int hs[];                                     // [kChunk][nt + 2] = [h | n_cnt | 1]
    __shared__ int s_code[kChunk];
    const int L = a.L, S = a.S, nseg = a.nseg, nt = a.nt, nw = nt + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / S, s = blockIdx.x % S;
    const int n = a.Bc * nseg;                                                    // segments per draw of this launch
    const int e0 = chunk * kChunk;
    const int cnt = n - e0 < kChunk ? n - e0 : kChunk;                            // (>= 1: the grid has no empty chunk)
    const float *tb = qfa_segment::tbar_row(a, s);
    const float fnt = (float)nt;

    // ---- (1) the counts of the wave's segments
    for (int i = wave; i < cnt; i += kWaves) {
        const int e = e0 + i;
        const int bl = e / nseg, g = e - bl * nseg;
        const qfa_segment::Segment sg = qfa_segment::locate(a, tb, bl, s, g);
        int h = 0, nused = 0, ncnt = 0;
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            bool used = false, counted = false;
            int bin = -1;
            if (j < L) {
#pragma clang fp contract(off)
                const qfa_segment::Pixel px = qfa_segment::pixel(a, sg, j);
                used = px.used;
                counted = used && px.ivar >= a.ivar_min;
                const float x = a.relative ? __fdiv_rn(px.T, px.tbar) : px.T;
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
        const int code = qfa_segment::segment_code(a, sg, valid);
        if (a.hist && lane < nt) a.hist[(sg.row * nseg + g) * nt + lane] = h;
        int *hr = hs + i * nw;
        if (lane < nt) hr[lane] = h;
        if (lane == 0) {
            hr[nt] = valid ? ncnt : 0;
            hr[nt + 1] = 1;
            s_code[i] = code;
        }
    }
    if (!a.part) return;
    __syncthreads();

    // ---- (2) the chunk's sums per z-bin
    const int cd = lane < cnt ? s_code[lane] : -1;                                // every wave holds the chunk's codes
    qfa_segment::chunk_products<int, 1>(hs, nt, a.nz, cd, a.part);
}

}  // namespace qfa_pdf
