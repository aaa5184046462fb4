// qfa_host.h -- host side of the step: workspace layout, launch geometry, kernel sequences.
// Shared by qfa_capi.hip (N_h <= 16; built with -amdgpu-mfma-vgpr-form so that the MFMA accumulators
// stay in VGPRs; pass 1 and stage 3 of pass 2 on the bf16 XDL pipe) and qfa_k32.hip (N_h in 17..32: 280 accumulator registers per lane need the AGPR
// half of the register file, so that translation unit is built without the flag).
// Every function here takes the call as one block (BatchCall, qfa_estep.h) and pass 2 as one more (Pass2Call); the input form and
// KP become template arguments in by_form (qfa_estep.h) and by_kp, and nowhere else; k_solve is launched by launch_solve alone.
#pragma once
#include "qfa_step_kernels.h"
#include "qfa_xdl_kernels.h"
#include "qfa_s12_x.h"
#include "qfa_estep.h"

// One launch of pass 2: the call plus what every form of pass 2 takes
struct Pass2Call : BatchCall {
    const float *SOL;            // the solve's records
    const float4 *ZS;            // per-spectrum factors of the factored-z form, else NULL
    float *accum;                // the packed buffer
    float *rows;                 // rows of the fixed-order reducer and their scalar records (NULL: pass 2 adds to the packed buffer
    double *rowsS;               // with atomics)
    int row_stride;              // floats per row
    Scal64 *sc64;
    int exact;                   // QFA_F_EXACT_GRAD
};

// KP -> compile-time constant: the one place that switches on it.  KPMAX = 16 in the translation units that hold no N_h = 17..32 code.
template <int KPMAX = 32, class Fn>
inline auto by_kp(int KP, Fn &&fn) {
    if (KP == 8) return fn(std::integral_constant<int, 8>{});
    if constexpr (KPMAX == 16) return fn(std::integral_constant<int, 16>{});
    else {
        if (KP == 16) return fn(std::integral_constant<int, 16>{});
        return fn(std::integral_constant<int, 32>{});
    }
}

// pass 2 for N_h <= 16 with every contraction on the XDL pipe (qfa_grads_x.h: KP = 8 or 16, built in qfa_gx.hip)
size_t qfa_gx_image_bytes(int KP, int ntiles32);
void qfa_gx_launch(int KP, const Pass2Call &a, int ntiles32, const WorkPlan &wp, unsigned char *PGX);
// everything a training step derives from the parameters before pass 1, in one launch (N_h <= 16; qfa_gx.hip, k_prep_step)
void qfa_prep_step_launch(int KP, bool pixres, const BatchCall &c, int ntiles32, unsigned char *PFX, unsigned char *P2, float4 *ZS,
                          float *zero, size_t n_zero, unsigned *tick1);

// the pixel-resident form of the all-XDL pass 2 (qfa_grads_t.h, built in qfa_gx.hip; N_h = 9..16): QFA_F_PASS2_PIXRES
struct GtPlan;
size_t qfa_gt_state_bytes(int KP, int B);
int qfa_gt_items(int KP, int B, int Npix, int max_ranges);
int qfa_gt_ranges(int KP, int B, int Npix, int max_ranges);
int qfa_gt_range_groups(int KP, int B, int Npix, int max_ranges);
int qfa_gt_items_bound(int KP, int B, int Npix);
int qfa_gt_ranges_bound(int KP, int B, int Npix);
void qfa_gt_launch(int KP, const Pass2Call &a, int max_ranges, const unsigned char *PGT, const unsigned char *PST);

// posterior writer for N_h <= 16 on the XDL pipe (qfa_predict_x.h, built in qfa_gx.hip)
size_t qfa_px_image_bytes(int KP, int ntiles32);
void qfa_px_launch(int KP, const BatchCall &c, const float *mu, int ntiles32, const WorkPlan &wp, unsigned char *PXI, const float *SOL,
                   float *cont, float *unc);

namespace {

#ifndef QFA_P1_MAX_CHAIN
#define QFA_P1_MAX_CHAIN 32  // longest accumulation chain of pass 1 at N_h = 17..32, in 32-pixel tiles (make_layout_t).  Round 5: 64 -> 32 --
                             // F gradient of 4 096 c5-shape spectra against the float64 oracle 8.2e-5 -> 4.5e-5 (the chain bias of
                             // qfa_xdl_kernels.h: N_h <= 16 has fresh accumulators per tile instead), c5 step 5.32 -> 5.41 ms
                             // (eight partial records per spectrum instead of four: k_sum_segments + 0.08 ms)
#endif

inline int kp_for(int Nh) { return Nh <= 8 ? 8 : (Nh <= 16 ? 16 : 32); }

// Compute units of the current device, queried once per device (launch geometry: resident-workgroup slots of the
// work plans).  256 on MI355X; also the answer when no device is visible (sizing calls in a CPU-only process).
inline int cu_count() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    int n = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        n = 256;
    }
    __atomic_store_n(&cache[dev], n, __ATOMIC_RELAXED);
    return n;
}

// XCDs of the current device (each has its own L2; the hardware deals the workgroups of a launch to them round-robin), queried
// once per device: 8 on MI355X in SPX mode, fewer in the partitioned modes.  k_grads_t maps its work items so that the
// workgroups that walk the same spectra share an XCD (GtPlan).
inline int xcd_count() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 8; }
    int n = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess || n < 1 || n > 64) {
        (void)hipGetLastError();
        n = 8;
    }
    __atomic_store_n(&cache[dev], n, __ATOMIC_RELAXED);
    return n;
}

// Work plan of a pass (WorkPlan, qfa_common.h): the blocks of 64 spectra that fill whole rounds of the 512
// resident-workgroup slots walk the whole pixel axis; the remaining blocks are cut into 1..8 pixel segments.  The
// plan minimises rounds x (tiles per item + prologue), the prologue of an item (operand loads, pipeline fill)
// counted as `pro` tiles; small batches (no full round) get the uniform split that fills the chip -- down to three
// tiles per item while the chip stays at most half full (the step of a small batch is latency-bound).
constexpr int kMaxSeg = 32;

inline WorkPlan plan_work(int B, int ntiles, int pro, int slots, int spb = 64, int max_chain = 0) {
    // slots = CUs x resident workgroups per CU; spb = spectra per block (64; 32 for k_grads_x)
    const int nblk = (B + spb - 1) / spb;
    // max_chain > 0: no item walks more than max_chain tiles (pass 1 at N_h = 17..32: see make_layout_t) -- every block is cut
    // into the same ceil(ntiles / max_chain) segments
    if (max_chain > 0 && ntiles > max_chain) {
        const int nn0 = (ntiles + max_chain - 1) / max_chain, st = (ntiles + nn0 - 1) / nn0;
        return WorkPlan{0, nblk, (ntiles + st - 1) / st, st};
    }
    WorkPlan best{0, nblk, 1, ntiles};
    double best_cost = 1e300;
    for (int full = (nblk / slots) * slots; full >= 0; full -= slots) {       // whole rounds kept unsegmented
        const int rem = nblk - full;
        for (int n = 1; n <= kMaxSeg; ++n) {
            const bool latency_bound = full == 0 && (long long)rem * n <= slots / 2;     // chip at most half full
            if (n > 1 && ntiles / n < (latency_bound ? 3 : 8)) break;  // keep segments >= 8 tiles (3 when latency-bound)
            if (n > 8 && !latency_bound) break;     // more than 8 segments measured slower once the chip is full
            const int st = (ntiles + n - 1) / n;
            const int nn = (ntiles + st - 1) / st;  // no empty segment
            const double rounds_rem = rem ? (double)((long long)rem * nn + slots - 1) / slots : 0.0;
            const double cost = (double)(full / slots) * (ntiles + pro) + (double)(long long)rounds_rem * (st + pro);
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best = WorkPlan{full, rem, rem ? nn : 1, rem ? st : ntiles};
            }
            if (!rem) break;
        }
        if (full == 0) break;
    }
    return best;
}

// deterministic mode: slab = [nblk rows of det_row_stride floats | scalar sums: (max items) x 4 waves x 3 doubles |
//                             float64 partial sums of the reducer: det_chunks x NF]
// A row holds the NF = Npix Nh + 3 Npix + Nb sums of one block of 64 spectra, padded to a multiple of 4 floats (16-byte
// stores), plus 64 floats that lanes outside the arrays write to (every lane of a flushing wave stores: the counted
// wait in k_grads_x needs a constant number of requests per wave).
inline size_t det_rows_floats(int Npix, int Nb, int Nh) { return (size_t)Npix * Nh + 3 * (size_t)Npix + Nb; }
inline size_t det_row_stride(int Npix, int Nb, int Nh) { return (det_rows_floats(Npix, Nb, Nh) + 3) / 4 * 4 + 64; }
inline size_t det_rows(int B) { return (size_t)((B + 63) / 64); }
constexpr int DET_CHUNK_ROWS = QFA_DET_CHUNK_ROWS;   // rows summed by one thread of the reducer's first stage
inline size_t det_chunks(int B) { return (det_rows(B) + DET_CHUNK_ROWS - 1) / DET_CHUNK_ROWS; }
struct DetLayout {
    size_t NF, stride, oS, oPart, bytes;      // offsets in bytes
};
// The region the fixed-order reducer works on: `rows` slab rows | scalar records, 3 doubles per item-wave | float64 partial sums of
// the reducer, `chunks` x NF (the parts start on 16-byte boundaries)
inline DetLayout rows_region(size_t rows, size_t itemwaves, size_t chunks, size_t NF, size_t stride) {
    DetLayout D;
    D.NF = NF;
    D.stride = stride;
    D.oS = (rows * stride * sizeof(float) + 15) / 16 * 16;
    D.oPart = D.oS + (itemwaves * 3 * sizeof(double) + 15) / 16 * 16;
    D.bytes = D.oPart + chunks * NF * sizeof(double);
    return D;
}
// The rows of the pixel-resident pass 2 (k_grads_t) where they live in the workspace (no caller's slab): one slab row per range of
// spectra, 8 waves per item.  make_layout_t sizes Layout::oISLAB from it and plan_step addresses the region by it.  (The reducer's
// chunks are DET_CHUNK_ROWS rows, as launch_reduce_slab cuts them.)
inline DetLayout pixres_rows_layout(size_t rows, size_t itemwaves, int Npix, int Nb, int Nh) {
    DetLayout D = rows_region(rows, itemwaves, (rows + DET_CHUNK_ROWS - 1) / DET_CHUNK_ROWS, det_rows_floats(Npix, Nb, Nh),
                              det_row_stride(Npix, Nb, Nh));
    D.bytes += 24 * sizeof(float);     // the slack this region has always had behind its parts (the workspace sizes are pinned)
    return D;
}

struct Layout {
    int KP, NpixPad, ntiles, Bpad;
    int ntiles32;                                      // pass 1 on the XDL pipe walks 32-pixel tiles (N_h <= 16)
    WorkPlan wp1, wp2;                                 // work items of pass 1 / pass 2
    static constexpr int spb1 = 64;                    // spectra per block of pass 1's plan (four waves of 16: k_moments_x)
    WorkPlan wp2x;                                     // pass 2 on the XDL pipe (k_grads_x: 32-pixel tiles, 1 workgroup per CU)
    WorkPlan wpp;                                      // posterior writer on the XDL pipe (k_predict_x, N_h <= 16)
    size_t oPFT, oPFX, oPGX, oPXI, oMOM, oSOL, oNLL, oNBL, oRED, oBG, oZS, oZP, oPST, oISLAB, total;   // float offsets
    int bg_stride;                                     // beta / gamma hand-over of pass 2 at N_h = 17..32 ([2][Bpad][NpixPad])
};

template <int KP>
Layout make_layout_t(int B, int Npix) {
    using C = Cfg<KP>;
    Layout L;
    L.KP = KP;
    L.NpixPad = round_up(Npix, 16);
    L.ntiles = L.NpixPad / 16;
    L.Bpad = round_up(B, 16);
    L.ntiles32 = (Npix + 31) / 32;
    const int NCU = cu_count();
    L.wp2 = plan_work(B, L.ntiles, 4, NCU * (KP == 8 ? QFA_G8_OCC : (KP > 16 ? 1 : 2)));
    // pass 1 runs on the XDL pipe at every N_h (32-pixel tiles; four waves per workgroup, two workgroups per CU at N_h <= 16 -- an
    // 8-wave workgroup per CU with two phase-shifted groups on one image ring measured 1.44 against 1.31 ms at c3 -- one at N_h > 16)
    // Pass 1 sums C, T, b, b2 of a spectrum over the pixel axis in MFMA accumulators.  The matrix pipe aligns the 32 products
    // of an instruction with the accumulator they are added to and keeps about two bits below the accumulator's last place
    // (tools/ubench/mfma_round.hip: products of 1/16 ulp(C) vanish, of 1/4 ulp survive; the sum itself is rounded to nearest), so
    // the longer the chain, the more of each new product is cut off: the per-spectrum NLL of a launch that walks 250 tiles in one
    // chain is 3.3e-6 (rms) from the float64 oracle, of the same spectra in segmented small-batch launches 7.8e-7
    // (tools/chain_bias.py, c5's shape; 1.8e-6 against 6.3e-7 at c3's 125 tiles), and at N_h = 17..32 the F gradient of
    // 20 000 spectra came out 3.6e-4 from the oracle.  So at N_h = 17..32 no chain is longer than QFA_P1_MAX_CHAIN tiles (the
    // partial records are 4.5 KB per spectrum and segment: 90 MB per segment at c5, against 1.7 ms of pass 1).
    // (N_h <= 16 keeps the work plan's own segmentation: the same bound there was superseded by the fresh accumulators per tile of
    // k_moments_x, profiles/r5_ablation.txt, section 2)
    L.wp1 = KP <= 16 ? plan_work(B, L.ntiles32, 1, 2 * NCU) : plan_work(B, L.ntiles32, 1, NCU, 64, QFA_P1_MAX_CHAIN);
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 63) / 64 * 64; return r; };
    L.oPFT = take((size_t)L.ntiles * C::TILE_PFT);
    L.oPFX = take((size_t)L.ntiles32 * (XCfg<KP>::TILE_B / 4) + 2 * (C::FW + C::PW));      // + the column maxima (pfx_colmax)
    L.oPGX = 0;
    L.wp2x = WorkPlan{0, 0, 1, 0};
    if constexpr (KP == 8 || KP == 16) {
        L.oPGX = take(qfa_gx_image_bytes(KP, L.ntiles32) / 4);
        L.wp2x = plan_work(B, L.ntiles32, 3, NCU, 64);
    } else {                                           // N_h = 17..32: stages 1 and 2 of pass 2 by k_s12_x (qfa_s12_x.h)
        L.oPGX = take((size_t)L.ntiles32 * (S12<KP>::TILE_B / 4));
        L.wp2x = plan_work(B, L.ntiles32, 3, NCU, 64);
    }
    L.oPXI = 0;
    L.wpp = WorkPlan{0, 0, 1, 0};
    if constexpr (KP <= 16) {
        L.oPXI = take(qfa_px_image_bytes(KP, L.ntiles32) / 4);
        L.wpp = plan_work(B, L.ntiles32, 1, 2 * NCU, 64 * (KP == 16 ? QFA_PX_SPW : QFA_PX_SPW8));
    }
    // moment records: segment 0 for every row, segments 1.. for the rows of the segmented blocks only
    L.oMOM = take(((size_t)L.Bpad + (size_t)(L.wp1.nseg - 1) * (L.Bpad - (size_t)L.spb1 * (size_t)L.wp1.full)) * C::NMOM);
    L.oSOL = take((size_t)L.Bpad * C::NSOL);
    L.oNLL = take((size_t)L.Bpad);
    L.oNBL = take((size_t)L.Bpad);
    L.oZS = take(4 * (size_t)L.Bpad);                   // factored-z input form: per-spectrum factors ZS (float4 each)
    L.oZP = take(4 * (size_t)L.NpixPad);                //                        per-pixel factors ZP (blue pixels)
    L.oRED = take(2 * 2 * NRED + 2 + sizeof(Scal64) / 4);   // k_reduce_nll: 2 x NRED doubles + the ticket counter; then the
                                                            // float64 scalar-gradient sums of pass 2 (Scal64)
    L.oPST = 0;                                         // pixel-resident pass 2: the per-group state images (qfa_grads_t.h)
    if constexpr (KP == 8 || KP == 16) L.oPST = take(qfa_gt_state_bytes(KP, B) / 4);
    // pixel-resident pass 2 without a caller's slab: its per-range sums go through rows of the workspace and the fixed-order
    // reducer as well (no atomics: the default accumulation of a large batch is bit-reproducible too).  Sized for N_b = N_pix,
    // N_h = KP
    L.oISLAB = 0;
    if constexpr (KP == 8 || KP == 16)
        L.oISLAB = take(pixres_rows_layout(qfa_gt_ranges_bound(KP, B, Npix), 8 * (size_t)qfa_gt_items_bound(KP, B, Npix), Npix, Npix, KP).bytes / sizeof(float));
    L.oBG = 0;
    L.bg_stride = round_up(Npix, 32);
    if constexpr (KP == 32) L.oBG = take(2 * (size_t)round_up(B, 64) * L.bg_stride);
    L.total = o;
    return L;
}

Layout make_layout(int B, int Npix, int Nh) {
    return by_kp(kp_for(Nh), [&](auto kp) { return make_layout_t<decltype(kp)::value>(B, Npix); });
}

// the batch's pointers: delta, error, mask always; the blue side needs zabs, or the factored form zq1 + pix_ratio
// (then zabs may be NULL), which does not combine with a host-supplied A_blue (include/qfa_hip.h)
// (ABI v3: rows / row_stride -- the resident, indexed input form; not combined with a host-supplied A_blue either)
inline int check_batch(const qfa_batch_t &b, int Npix, int Nb) {
    if (!b.delta || !b.error || !b.mask) return QFA_E_NULL;
    const bool fac = b.zq1 || b.pix_ratio;
    if (fac && !(b.zq1 && b.pix_ratio)) return QFA_E_NULL;
    if (fac && b.A_blue) return QFA_E_NULL;
    if (Nb > 0 && !fac && !b.zabs) return QFA_E_NULL;
    if (b.rows && b.A_blue) return QFA_E_NULL;
    if (b.row_stride != 0 && (b.row_stride < (int64_t)Npix || b.row_stride >= (1LL << 31))) return QFA_E_SIZE;
    if (!b.rows && (long long)64 * b.row_stride >= (1LL << 31)) return QFA_E_SIZE;   // batch order = storage order: 32-bit offsets
                                                                                    // inside a wave's 16 neighbouring rows
    return 0;
}
inline int check_shape(int B, int Npix, int Nb, int Nh) {
    if (B < 1 || Npix < 1 || Nb < 0 || Nb > Npix || Nh < 1 || Nh > 32) return QFA_E_SIZE;
    if ((long long)64 * Npix >= (1LL << 31)) return QFA_E_SIZE;      // 32-bit byte offsets inside a wave's 16 rows
    // the per-pixel counts and the spectrum counts of the packed buffer are float32 sums of ones: exact up to 2^24
    // contributions, so one accumulation (launch, or all-reduced job of launches into one buffer) takes at most
    // 16 777 216 spectra; beyond that the caller finalises more often (the host code here never comes near it)
    if (B > (1 << 24)) return QFA_E_SIZE;
    return 0;
}

// Which form of pass 2 runs at N_h <= 16 (KP = 8 or 16).  Three forms: k_grads (float32-MFMA stage 1), the two-role all-XDL k_grads_x,
// the pixel-resident all-XDL k_grads_t.  Defaults from measurements on MI355X
// (tools/time_pass2.py: pass 1 + solve + pass 2 per call, ms; profiles/r3_ablation_pass2.txt):
//   k_grads never: k_grads_x is as fast or faster at every batch size measured, N_h = 8: 0.072 / 0.083 at 500 spectra x 2000 px,
//     0.104 / 0.117 at 2 000, 0.192 / 0.220 at 8 000, 2.82 / 3.25 at 40 000 x 9243 (the one exception, 10 000 x 2000 --
//     157 blocks on 256 CUs, 0.281 / 0.258 -- goes to k_grads_t); N_h = 16: 2.5 - 2.6 against 3.2 ms at c3;
//   k_grads_t once the batch gives every workgroup a walk long enough to pay for its prologue and epilogue (the figures of ROUND 3 --
//     superseded for N_pix >= 1024 by the round-5 sweep quoted in pass2_form below):
//     N_h = 9..16 from 96 spectra per CU (24 576) on: N_pix = 4000: 0.146 / 0.166 at 1 000 spectra, 0.42 / 0.44 at 8 000,
//       1.43 / 1.35 at 32 000, 4.31 / 3.98 at 100 000 (k_grads_x / k_grads_t); N_pix = 640: 0.161 / 0.183 at 8 000, 1.085 / 0.971 at 100 000;
//     N_h <= 8 (a wave owns two 16-pixel tiles there) from 96 spectra per CU on, and from 36 per CU (9 216) on for N_pix >= 1024:
//       N_pix = 2000: 0.191 / 0.187 at 8 000, 0.278 / 0.215 at 10 000, 0.530 / 0.389 at 24 000, 1.21 / 0.85 at 64 000;
//       N_pix = 9243: 0.635 / 0.672 at 8 000, 1.83 / 1.63 at 24 000, 2.85 / 2.45 at 40 000; N_pix = 640: 0.116 / 0.141 at 8 000,
//       0.274 / 0.260 at 32 000, 0.83 / 0.62 at 100 000 (k_grads_x<8> / k_grads_t<8>).
// QFA_F_PASS2_F32 / QFA_F_PASS2_XDL / QFA_F_PASS2_PIXRES in the call's `flags` force one form (A/B timing and the cross-checks of
// the forms in tests/).
enum class Pass2 { F32, XDL, PIXRES, S12 };       // k_grads | k_grads_x | k_grads_t | k_s12_x + k_grads_s3 (N_h = 17..32)
inline Pass2 pass2_form(int KP, int B, int Npix, unsigned flags) {
    if (KP > 16) return Pass2::S12;
    if (flags & QFA_F_PASS2_F32) return Pass2::F32;
    if (Npix < 16) return Pass2::XDL;                  // (k_grads_t's ragged-tile staging wants N_pix >= 4)
    if (flags & QFA_F_PASS2_PIXRES) return Pass2::PIXRES;
    if (flags & QFA_F_PASS2_XDL) return Pass2::XDL;
    if (B >= 96 * cu_count()) return Pass2::PIXRES;
    // Round 5, after the float16 stages (18 + 35 MFMAs per group instead of 36 + 51) and the reworked walk: the pixel-resident form
    // wins from a few hundred spectra on wherever the pixel axis gives every CU work (tools/pass2_crossover.sh,
    // profiles/r5_pass2_crossover.txt; step k_grads_x / k_grads_t in ms): N_h = 16, N_pix = 4000: 0.102 / 0.096 at 128 spectra,
    // 0.127 / 0.109 at 500, 0.206 / 0.149 at 2 000, 0.51 / 0.30 at 8 000; N_h = 8, N_pix = 2000: 0.080 / 0.088 at 256, 0.086 / 0.085
    // at 500, 0.095 / 0.083 at 1 000, 0.195 / 0.134 at 8 000; N_pix = 9243: 0.106 / 0.102 at 256, 0.182 / 0.148 at 1 000.
    // (Short pixel axes keep the rule of round 3: 96 spectra per CU.)
    if (Npix < 1024) return Pass2::XDL;
    return (KP == 16 ? B >= 128 : B >= 512) ? Pass2::PIXRES : Pass2::XDL;
}

// the tile-major float32 image PFT: k_grads and k_predict_out (N_h <= 16), k_grads_s3 (N_h = 17..32)
template <int KP>
void launch_prep_pft(const BatchCall &c, const float4 *ZP, const Layout &L) {
    dim3 blk(64, 4);
    k_prep_pft<KP><<<(L.NpixPad + 3) / 4, blk, 0, c.st>>>(c.p.F, c.p.Psi, c.p.omega, ZP, c.Npix, c.Nb, c.Nh, L.NpixPad, c.ws + L.oPFT);
}

// the arrival counters of k_reduce_nll and k_solve in the workspace; Scal64 of pass 2 lies behind them (both zeroed by k_solve)
inline unsigned *ws_ticket(const BatchCall &c, const Layout &L) {
    return reinterpret_cast<unsigned *>(reinterpret_cast<double *>(c.ws + L.oRED) + 2 * NRED);
}

// k_solve (KP lanes per spectrum, four waves per block) from the moment records of pass 1.  What it writes:
enum class Solve {
    RECORD,    // the float32 record SOL (the E-step: with exact = 1)
    STATE,     // the operand images k_grads_t streams (N_h <= 16)
    NLLRED,    // SOL, and its last block sums the NLL of a small batch into `scal` (no k_reduce_nll; N_h <= 16)
    PREDICT    // SOL, the log-likelihood `nll`, the posterior mean `hmean` and covariance `hcov`
};
template <int KP>
void launch_solve(Solve kind, const BatchCall &c, const Layout &L, float *nll, int exact, float *scal = nullptr,
                  float *hmean = nullptr, float *hcov = nullptr) {
    constexpr int G = 64 / KP;
    const unsigned nblk = (unsigned)((c.B + 4 * G - 1) / (4 * G));
    float *MOM = c.ws + L.oMOM, *SOL = c.ws + L.oSOL, *NBL = c.ws + L.oNBL;
    unsigned *ticket = ws_ticket(c, L);
    switch (kind) {
        case Solve::RECORD:
            k_solve<KP, false><<<nblk, 256, 0, c.st>>>(MOM, SOL, nll, NBL, c.B, c.Nh, nullptr, nullptr, ticket, nullptr, nullptr, exact);
            break;
        case Solve::STATE:
            if constexpr (KP <= 16)
                k_solve<KP, false, true><<<nblk, 256, 0, c.st>>>(MOM, SOL, nll, NBL, c.B, c.Nh, nullptr, nullptr, ticket,
                                                                 reinterpret_cast<unsigned char *>(c.ws + L.oPST), nullptr, exact);
            break;
        case Solve::NLLRED:
            if constexpr (KP <= 16)
                k_solve<KP, false, false, true><<<nblk, 256, 0, c.st>>>(MOM, SOL, nll, NBL, c.B, c.Nh, nullptr, nullptr, ticket, nullptr, scal, exact);
            break;
        case Solve::PREDICT:
            k_solve<KP, true><<<nblk, 256, 0, c.st>>>(MOM, SOL, nll, nullptr, c.B, c.Nh, hmean, hcov);
            break;
    }
}

// the caller's stage events (bench.py's stamps; entries may be NULL), recorded on the call's stream
struct EventMarks {
    void *const *events;
    hipStream_t st;
    void operator()(int i) const {
        if (events && events[i]) (void)hipEventRecord((hipEvent_t)events[i], st);
    }
};

// MOM[seg 0] += MOM[seg 1..] for the rows of the segmented blocks of pass 1
template <int KP>
void sum_segments(const BatchCall &c, const Layout &L) {
    const WorkPlan &w = L.wp1;
    if (w.rem == 0 || w.nseg <= 1) return;
    float *MOM = c.ws + L.oMOM;
    const size_t row0 = (size_t)w.full * L.spb1;
    const size_t rows = (size_t)L.Bpad - row0;                  // Bpad is a multiple of 16, NMOM of 4
    const size_t n4 = rows * Cfg<KP>::NMOM / 4;
    k_sum_segments<<<(unsigned)((n4 + 255) / 256), 256, 0, c.st>>>(
        reinterpret_cast<float4 *>(MOM + row0 * Cfg<KP>::NMOM),
        reinterpret_cast<const float4 *>(MOM + (size_t)L.Bpad * Cfg<KP>::NMOM), w.nseg, n4);
}

// Factored-z input form (qfa_batch_t::zq1 / pix_ratio; qfa_common.h ZFac): the per-spectrum and per-pixel factor tables
// of this call, or NULL pointers when the batch carries zabs only.
struct ZTables {
    const float4 *ZS, *ZP;
};
inline bool has_zfac(const BatchCall &c) { return c.b.zq1 && c.b.pix_ratio && c.Nb > 0; }
inline ZTables launch_zfac(const BatchCall &c, const Layout &L) {
    if (!has_zfac(c)) return ZTables{nullptr, nullptr};
    float4 *ZS = reinterpret_cast<float4 *>(c.ws + L.oZS), *ZP = reinterpret_cast<float4 *>(c.ws + L.oZP);
    k_zfac_spec<<<(c.B + 255) / 256, 256, 0, c.st>>>(c.b.zq1, c.b.rows, c.p, c.tau, c.B, ZS);
    k_zfac_pix<<<(c.Nb + 255) / 256, 256, 0, c.st>>>(c.b.pix_ratio, c.p, c.tau, c.Nb, ZP);
    return ZTables{ZS, ZP};
}

// pass 1 on the XDL pipe (split-bf16 operands, 32-pixel tiles) at every N_h
template <int KP, bool PREDICT>
void launch_moments(const BatchCall &c, const float *mu, const Layout &L, const ZTables &zt, bool prep = true, bool exact = false) {
    float *MOM = c.ws + L.oMOM;
    unsigned char *PFX = reinterpret_cast<unsigned char *>(c.ws + L.oPFX);
    if (prep) {
        if (XCfg<KP>::F16) {
            unsigned *cm = pfx_colmax<KP>(PFX, L.ntiles32);
            (void)hipMemsetAsync(cm, 0, sizeof(unsigned) * XCfg<KP>::NCOL, c.st);
            k_colmax<KP><<<L.ntiles32, 1024, 0, c.st>>>(c.p.F, c.p.Psi, c.Npix, c.Nh, cm);
        }
        k_prep_pfx<KP><<<L.ntiles32, 256, 0, c.st>>>(c.p.F, c.p.Psi, c.p.omega, PREDICT ? mu : nullptr, zt.ZP, -QFA_LOG2E * c.tau.offset,
                                                     c.Npix, c.Nb, c.Nh, PFX);
    }
    constexpr int NW = 4;                             // (L.spb1 = 16 NW spectra per block)
    // the exact-gradient step's instantiation leaves out the T-side moments where that measured faster (QFA_P1_SKIPT_EXACT_KP)
    constexpr bool SKIP_EX = !PREDICT && KP >= QFA_P1_SKIPT_EXACT_KP;
    by_form(c.b, zt.ZS != nullptr, exact, [&](auto f) {
        using Fm = decltype(f);
        k_moments_x<KP, PREDICT, NW, Fm::zf, SKIP_EX && Fm::exact><<<L.wp1.items(), 64 * NW, 0, c.st>>>(
            c.p, c.b, c.tau, mu, c.B, L.Bpad, c.Npix, c.Nb, L.ntiles32, L.wp1, PFX, zt.ZS, MOM);
    });
}

inline DetLayout det_layout(const Layout &L, int B, int Npix, int Nb, int Nh) {
    size_t items = (size_t)(L.wp2.items() > L.wp2x.items() ? L.wp2.items() : L.wp2x.items());
    if (L.KP == 16 || L.KP == 8) items = std::max(items, 2 * (size_t)qfa_gt_items(L.KP, B, Npix, (int)det_rows(B)));   // (8 waves per item there)
    return rows_region(det_rows(B), 4 * items, det_chunks(B), det_rows_floats(Npix, Nb, Nh), det_row_stride(Npix, Nb, Nh));
}
inline size_t det_slab_bytes(int B, int Npix, int Nb, int Nh) { return det_layout(make_layout(B, Npix, Nh), B, Npix, Nb, Nh).bytes; }

// the fixed-order reduction of `rows` slab rows into the packed buffer: rows in chunks of DET_CHUNK_ROWS (float64 partials,
// rows in order), then the chunks in order
inline void launch_reduce_slab(const float *slab, const DetLayout &D, int rows, int nitemwaves, float *accum, hipStream_t st) {
    const double *slabS = reinterpret_cast<const double *>(reinterpret_cast<const char *>(slab) + D.oS);
    double *part = reinterpret_cast<double *>(const_cast<char *>(reinterpret_cast<const char *>(slab)) + D.oPart);
    const int nch = (rows + DET_CHUNK_ROWS - 1) / DET_CHUNK_ROWS;
    const unsigned gx = (unsigned)((D.NF + 255) / 256);
    k_reduce_slab_rows<<<dim3(gx, (unsigned)nch), 256, 0, st>>>(slab, rows, D.NF, D.stride, part);
    k_reduce_slab_fin<<<gx, 256, 0, st>>>(part, slabS, nch, nitemwaves, D.NF, accum);
}

// What a training step launches, decided once from the shape, the flags and whether the caller brought a slab.
struct StepPlan {
    int err;               // QFA_E_FLAGS: the call asks for a form that does not exist at this N_h
    Pass2 pass2;
    Solve solve;
    bool prep_step;        // the preparations are ONE launch (k_prep_step: both passes on the XDL pipe, N_h <= 16); else memset,
                           // k_zfac_*, k_prep_pft, and k_prep_pfx in front of pass 1
    int nred;              // blocks of k_reduce_nll; 0: the solve summed the NLL itself
    // the fixed-order reducer behind pass 2 (rows == 0: pass 2 adds to the packed buffer itself)
    bool rows_in_ws;       // the rows live in the workspace (Layout::oISLAB), not in a caller's slab
    int max_ranges;        // pixel-resident pass 2: at most that many ranges of spectra (= rows)
    int rows, itemwaves;   // rows written, scalar records written (waves per work item x items)
    DetLayout D;           // of the region the rows live in (all zero without one)
};
inline StepPlan plan_step(const Layout &L, const BatchCall &c, bool slab) {
    const int B = c.B, Npix = c.Npix, Nb = c.Nb, Nh = c.Nh;
    StepPlan P{};
    if (L.KP <= 16 && (c.flags & QFA_F_S3_FAST)) {      // (the three-product form exists at N_h = 17..32 only)
        P.err = QFA_E_FLAGS;
        return P;
    }
    P.pass2 = pass2_form(L.KP, B, Npix, c.flags);
    P.prep_step = P.pass2 == Pass2::XDL || P.pass2 == Pass2::PIXRES;
    // (pixel-resident pass 2: the solve writes the operand images that form streams instead of the float32 record SOL;
    // small batches -- one block of k_reduce_nll -- on the two-role form: the solve's last block sums the NLL itself)
    P.solve = P.pass2 == Pass2::PIXRES ? Solve::STATE : (P.pass2 == Pass2::XDL && B <= 2048 ? Solve::NLLRED : Solve::RECORD);
    P.nred = P.solve == Solve::NLLRED ? 0 : (B <= 2048 ? 1 : (B >= 2048 * NRED ? NRED : (B + 2047) / 2048));   // small batches: one block, no hand-over
    if (slab) P.D = det_layout(L, B, Npix, Nb, Nh);
    if (P.pass2 == Pass2::PIXRES) {
        // the sums of a range leave as one slab row: the caller's slab (deterministic mode), else rows of the workspace
        P.rows_in_ws = !slab;
        P.max_ranges = slab ? (int)det_rows(B) : (1 << 30);
        P.rows = qfa_gt_ranges(L.KP, B, Npix, P.max_ranges);
        P.itemwaves = 8 * qfa_gt_items(L.KP, B, Npix, P.max_ranges);
        if (!slab) P.D = pixres_rows_layout(P.rows, P.itemwaves, Npix, Nb, Nh);
    } else if (slab) {
        P.rows = (int)det_rows(B);
        P.itemwaves = 4 * (P.pass2 == Pass2::F32 ? L.wp2.items() : L.wp2x.items());
    }
    return P;
}

// pass 2 in its float32-MFMA form (QFA_F_PASS2_F32, N_h <= 16): custom tau table / factored z / zabs
template <int KP>
void launch_grads_f32(const Pass2Call &a, const Layout &L, const float *PFT) {
    by_form(a.b, a.ZS != nullptr, a.exact != 0, [&](auto f) {
        using Fm = decltype(f);
        k_grads<KP, Fm::hasa, Fm::zf, Fm::exact><<<L.wp2.items(), 256, 0, a.st>>>(a.p, a.b, a.tau, a.B, a.Npix, a.Nb, a.Nh, L.ntiles, L.wp2, PFT, a.SOL,
                                                                                 a.accum, a.rows, a.rowsS, a.row_stride, a.sc64, a.ZS);
    });
}

// pass 2 at N_h = 17..32: stages 1 and 2 for every (spectrum, pixel) on the XDL pipe, beta / gamma through HBM, then stage 3 per
// 16 columns
template <int KP>
void launch_s12_s3(const Pass2Call &a, const Layout &L, const float4 *ZP, const float *PFT) {
    float *BG = a.ws + L.oBG, *GG = BG + (size_t)round_up(a.B, 64) * L.bg_stride;
    unsigned char *IMG = reinterpret_cast<unsigned char *>(a.ws + L.oPGX);
    k_prep_s12<KP><<<L.ntiles32, 256, 0, a.st>>>(a.p.F, a.p.Psi, a.p.omega, ZP, a.Npix, a.Nb, a.Nh, IMG);
    by_form(a.b, a.ZS != nullptr, a.exact != 0, [&](auto f) {
        using Fm = decltype(f);
        k_s12_x<KP, Fm::hasa, Fm::zf, Fm::exact><<<L.wp2x.items(), 256, 0, a.st>>>(a.p, a.b, a.tau, a.B, a.Npix, a.Nb, a.Nh, L.ntiles32, L.wp2x, IMG, a.SOL,
                                                                                  BG, GG, L.bg_stride, a.accum, a.rows, a.rowsS, a.row_stride,
                                                                                  a.sc64, a.ZS);
    });
    for (int bh = 0; 16 * bh < a.Nh; ++bh) {
        if (a.flags & QFA_F_S3_FAST)
            k_grads_s3<KP, 3><<<L.wp2.items(), 256, 0, a.st>>>(a.B, a.Npix, a.Nh, L.ntiles, L.wp2, bh, PFT, a.SOL, BG, GG, L.bg_stride, a.accum, a.rows, a.row_stride);
        else
            k_grads_s3<KP, 6><<<L.wp2.items(), 256, 0, a.st>>>(a.B, a.Npix, a.Nh, L.ntiles, L.wp2, bh, PFT, a.SOL, BG, GG, L.bg_stride, a.accum, a.rows, a.row_stride);
    }
}

// The training step: plan, preparations, pass 1, solve, NLL sum, pass 2, fixed-order reduction.  The stage events 0..4 stand in
// front of the preparations, pass 1, the segment sum, pass 2, and behind everything.
template <int KP>
int run_nll_grad(const BatchCall &c, float *nll, float *accum, void *const *events, void *slabv) {
    const Layout L = make_layout_t<KP>(c.B, c.Npix);
    const StepPlan P = plan_step(L, c, slabv != nullptr);
    if (P.err == 0) {
        float *ws = c.ws;
        const float *PFT = ws + L.oPFT;
        float *nllbuf = nll ? nll : ws + L.oNLL;
        unsigned char *P2 = reinterpret_cast<unsigned char *>(ws + L.oPGX), *PST = reinterpret_cast<unsigned char *>(ws + L.oPST);
        // the rows of the fixed-order reducer and their scalar records (NULL: pass 2 adds to the packed buffer with atomics)
        float *rows = P.rows_in_ws ? ws + L.oISLAB : reinterpret_cast<float *>(slabv);
        double *rowsS = rows ? reinterpret_cast<double *>(reinterpret_cast<char *>(rows) + P.D.oS) : nullptr;
        const size_t accS = det_rows_floats(c.Npix, c.Nb, c.Nh), n_acc = accS + 8;
        double *red = reinterpret_cast<double *>(ws + L.oRED);
        unsigned *ticket = ws_ticket(c, L);
        Scal64 *sc64 = reinterpret_cast<Scal64 *>(ticket + 2);      // (zeroed by k_solve, like the ticket)
        // QFA_F_EXACT_GRAD: k_solve forms Z = -C^-1, p = y; pass 2 sums the exact tau0 / c0 / beta terms; the buffer's slot 6
        // counts the spectra of such launches (k_reduce_nll, or the solve's last block), and k_finalize* read the mode there
        const int exact = (c.flags & QFA_F_EXACT_GRAD) ? 1 : 0;
        const EventMarks mark{events, c.st};
        mark(0);
        ZTables zt{nullptr, nullptr};
        if (P.prep_step) {
            // ONE launch builds the two images and the per-spectrum factors, zeroes accum and the solve's arrival counter ticket[1]
            float4 *ZS = has_zfac(c) ? reinterpret_cast<float4 *>(ws + L.oZS) : nullptr;
            zt.ZS = ZS;
            qfa_prep_step_launch(KP, P.pass2 == Pass2::PIXRES, c, L.ntiles32, reinterpret_cast<unsigned char *>(ws + L.oPFX), P2, ZS,
                                 (c.flags & QFA_F_ZERO_ACCUM) ? accum : nullptr, n_acc, ticket + 1);
        } else {
            if (c.flags & QFA_F_ZERO_ACCUM) (void)hipMemsetAsync(accum, 0, n_acc * sizeof(float), c.st);
            zt = launch_zfac(c, L);
            launch_prep_pft<KP>(c, zt.ZP, L);
        }
        mark(1);
        launch_moments<KP, false>(c, nullptr, L, zt, !P.prep_step, exact != 0);
        mark(2);
        sum_segments<KP>(c, L);
        launch_solve<KP>(P.solve, c, L, nllbuf, exact, accum + accS);
        if (P.nred) k_reduce_nll<<<P.nred, 256, 0, c.st>>>(nllbuf, ws + L.oNBL, c.B, accum + accS, red, ticket, exact);
        mark(3);
        const Pass2Call a{c, ws + L.oSOL, zt.ZS, accum, rows, rowsS, (int)P.D.stride, sc64, exact};
        switch (P.pass2) {
            case Pass2::F32:
                if constexpr (KP <= 16) launch_grads_f32<KP>(a, L, PFT);
                break;
            case Pass2::XDL: qfa_gx_launch(KP, a, L.ntiles32, L.wp2x, P2); break;
            case Pass2::PIXRES: qfa_gt_launch(KP, a, P.max_ranges, P2, PST); break;
            case Pass2::S12:
                if constexpr (KP > 16) launch_s12_s3<KP>(a, L, zt.ZP, PFT);
                break;
        }
        if (P.rows) launch_reduce_slab(rows, P.D, P.rows, P.itemwaves, accum, c.st);
        mark(4);
    }
    return P.err ? P.err : hip_status(c.st, c.flags);
}

template <int KP>
int run_predict(const BatchCall &c, const float *mu, float *ll, float *hmean, float *hcov, float *cont, float *unc, void *const *events) {
    const Layout L = make_layout_t<KP>(c.B, c.Npix);
    const float *PFT = c.ws + L.oPFT, *SOL = c.ws + L.oSOL;
    const EventMarks mark{events, c.st};
    const bool writer_xdl = !(c.flags & QFA_F_PREDICT_F32);        // (the float32-MFMA writer: A/B timing, cross-check)
    mark(0);
    const ZTables zt = launch_zfac(c, L);
    if (!writer_xdl) launch_prep_pft<KP>(c, nullptr, L);      // (k_predict_out)
    launch_moments<KP, true>(c, mu, L, zt);
    mark(1);
    sum_segments<KP>(c, L);
    launch_solve<KP>(Solve::PREDICT, c, L, ll, 0, nullptr, hmean, hcov);
    mark(2);
    if constexpr (KP > 16) {
        if (writer_xdl) {              // the image of k_s12_x with mu in the place of Psi (qfa_s12_x.h)
            unsigned char *IMG = reinterpret_cast<unsigned char *>(c.ws + L.oPGX);
            k_prep_s12<KP><<<L.ntiles32, 256, 0, c.st>>>(c.p.F, mu, c.p.omega, nullptr, c.Npix, c.Nb, c.Nh, IMG);
            k_predict_x32<KP><<<L.wp2x.items(), 256, 0, c.st>>>(c.B, c.Npix, L.ntiles32, L.wp2x, IMG, SOL, cont, unc);
        }
    }
    if (writer_xdl && KP <= 16)
        qfa_px_launch(KP, c, mu, L.ntiles32, L.wpp, reinterpret_cast<unsigned char *>(c.ws + L.oPXI), SOL, cont, unc);
    else if (!writer_xdl)
        k_predict_out<KP><<<(c.B + 63) / 64, 256, 0, c.st>>>(mu, c.B, c.Npix, L.ntiles, PFT, SOL, cont, unc);
    mark(3);
    return hip_status(c.st, c.flags);
}

// The E-step of the EM update of F (qfa_em.hip): the training step's images + pass 1 + solve with the existing kernels (the
// exact-gradient flavour: pass 1 without the T-side moments where that instantiation exists, the solve's record [y | C^-1' | ..]
// in SOL) -- no pass 2, no continuum writer.  `nll` (B floats, or NULL = the workspace's own row) gets the per-spectrum NLL.
template <int KP>
int run_estep(const BatchCall &c, float *nll, QfaEStep *out) {
    const Layout L = make_layout_t<KP>(c.B, c.Npix);
    float *nllbuf = nll ? nll : c.ws + L.oNLL;
    const ZTables zt = launch_zfac(c, L);
    launch_moments<KP, false>(c, nullptr, L, zt, true, true);
    sum_segments<KP>(c, L);
    launch_solve<KP>(Solve::RECORD, c, L, nllbuf, 1);
    out->SOL = c.ws + L.oSOL;
    out->nsol = Cfg<KP>::NSOL;
    out->KP = KP;
    out->sol_ci = Cfg<KP>::SOL_CI;
    out->ZS = zt.ZS;
    out->ZP = zt.ZP;
    out->nll = nllbuf;
    return hip_status();
}

}  // namespace

// N_h in 17..32 (defined in qfa_k32.hip)
int qfa_k32_nll_grad(const BatchCall &c, float *nll, float *accum, void *const *events, void *slab);
int qfa_k32_predict(const BatchCall &c, const float *mu, float *ll, float *hmean, float *hcov, float *cont, float *unc, void *const *events);
