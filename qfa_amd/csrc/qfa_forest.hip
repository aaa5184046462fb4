// qfa_forest.hip -- C-ABI of the Lyman-alpha forest transmission and its stack (include/qfa_hip.h: qfa_forest_stack_doubles,
// qfa_forest_workspace_bytes, qfa_forest_f32): argument checks, the launch plan and the launches.  Kernels in qfa_forest.h.
#include "qfa_forest.h"
#include "qfa_call.h"

#include <math.h>

namespace {

using namespace qfa_forest;

constexpr int kMaxBins = 4096;
constexpr size_t kLdsTarget = 32768;          // bytes of tables per block the plan aims at (several blocks per CU) ...
constexpr size_t kLdsLimit = 65536;           // ... and the most a block may have: nbin <= 512 at one draw per launch
constexpr int64_t kBlocks = 1024;             // blocks of a large call (four per CU): each owns a row of partial sums
constexpr size_t kGlobalRows = (size_t)64 << 20;   // global form: bytes of rows the plan aims at

// How a call is cut: `Sc` draws per launch, `rpb` spectra per block; workspace = [image (Nh + 1) x pad floats | rows x rowlen
// doubles] from its first 16-byte boundary on.  A function of the shape alone, so that two calls on one shape add in one order.
struct Plan {
    int pad, strips, Sc, rpb;
    bool lds;
    int64_t blocks, rows;
    size_t rowlen, img_floats, bytes;
};

bool shape_ok(int B, int S, int Npix, int Nb, int Nh, int nbin) {
    return B >= 0 && S >= 1 && Npix >= 1 && Nb >= 0 && Nb <= Npix && Nh >= 1 && Nh <= 32 && nbin >= 1 && nbin <= kMaxBins;
}

Plan make_plan(int B, int S, int Nb, int Nh, int nbin) {
    Plan P;
    P.strips = Nb > 0 ? (Nb + kStrip - 1) / kStrip : 1;
    P.pad = P.strips * kStrip;
    const size_t one = (size_t)kWaves * 4 * nbin * sizeof(double);               // tables of a block at one draw
    P.lds = one <= kLdsLimit;
    int64_t sc = P.lds ? (int64_t)(kLdsTarget / one) : 1;
    P.Sc = (int)(sc < 1 ? 1 : (sc > S ? S : sc));
    P.rowlen = (size_t)P.Sc * 4 * nbin;
    int64_t cap = kBlocks;
    if (!P.lds) {
        const int64_t fit = (int64_t)(kGlobalRows / (P.rowlen * sizeof(double))) / kWaves;
        cap = fit < 1 ? 1 : (fit < kBlocks ? fit : kBlocks);
    }
    const int64_t chunks_max = cap / P.strips > 0 ? cap / P.strips : 1;
    const int64_t Bn = B > 0 ? B : 1;
    int64_t rpb = (Bn + chunks_max - 1) / chunks_max;
    const int64_t least = (4 + P.Sc - 1) / P.Sc;                                 // the image loads of a block serve >= 4 rows (b, s)
    if (rpb < least) rpb = least;
    P.rpb = (int)rpb;
    P.blocks = (Bn + rpb - 1) / rpb * P.strips;
    P.rows = P.lds ? P.blocks : P.blocks * kWaves;
    P.img_floats = (size_t)(Nh + 1) * P.pad;
    P.bytes = 16 + P.img_floats * sizeof(float) + (size_t)P.rows * P.rowlen * sizeof(double);
    return P;
}

template <int NHM>
void launch(const Args &a, const Plan &P, hipStream_t st) {
    const unsigned grid = (unsigned)P.blocks;
    if (!a.rows || !P.lds) {
        k_forest<NHM, false><<<grid, kThreads, 0, st>>>(a);
    } else {
        const size_t lds = (size_t)kWaves * a.ScMax * 4 * a.nbin * sizeof(double);
        k_forest<NHM, true><<<grid, kThreads, lds, st>>>(a);
    }
}

}  // namespace

extern "C" {

size_t qfa_forest_stack_doubles(int S, int nbin) {
    if (S < 1 || nbin < 1 || nbin > kMaxBins) return 0;
    return (size_t)S * 4 * nbin;
}

size_t qfa_forest_workspace_bytes(int B, int S, int Npix, int Nb, int Nh, int nbin) {
    if (!shape_ok(B, S, Npix, Nb, Nh, nbin)) return 0;
    return make_plan(B, S, Nb, Nh, nbin).bytes;
}

int qfa_forest_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, const float *unc, int B, int S,
                   int Npix, int Nb, int Nh, const qfa_forest_bins_t *bins, float cont_min, unsigned flags, float *trans,
                   float *ivar, double *stack, void *workspace, size_t workspace_bytes, void *stream) {
    if (!F || !mu || !b || !h || !bins || !workspace || (!trans && !ivar && !stack)) return QFA_E_NULL;
    if (!b->delta || !b->error) return QFA_E_NULL;
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (B < 0 || S < 1 || Npix < 1 || Nb < 0 || Nb > Npix || Nh < 1 || Nh > 32) return QFA_E_SIZE;
    if (Nb > 0 && !fac && !b->zabs) return QFA_E_NULL;
    if (!(bins->dz > 0.f) || !isfinite(bins->dz) || !isfinite(bins->z0) || bins->nbin < 1 || bins->nbin > kMaxBins ||
        bins->p_lo < 0 || bins->p_lo > bins->p_hi || bins->p_hi > Nb)
        return QFA_E_SIZE;
    if (b->row_stride != 0 && b->row_stride < (int64_t)Npix) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_FOREST_UNIT_W)) return QFA_E_FLAGS;
    const int nbin = bins->nbin;
    const Plan P = make_plan(B, S, Nb, Nh, nbin);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0 || Nb == 0) {
        if (stack && zero) {
            hipError_t e = hipMemsetAsync(stack, 0, (size_t)S * 4 * nbin * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    float *img = (float *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    double *rows = (double *)(img + P.img_floats);
    k_forest_image<<<(unsigned)((P.img_floats + 255) / 256), 256, 0, st>>>(F, mu, Nb, Nh, P.pad, img);
    Args a;
    a.bt = norm_batch(*b, Npix);
    a.img = img;
    a.h = h;
    a.unc = unc;
    a.trans = trans;
    a.ivar = ivar;
    a.rows = stack ? rows : nullptr;
    a.pad = P.pad; a.B = B; a.S = S; a.Npix = Npix; a.Nb = Nb; a.Nh = Nh; a.strips = P.strips; a.rpb = P.rpb;
    a.nbin = nbin; a.p_lo = bins->p_lo; a.p_hi = bins->p_hi;
    a.z0 = bins->z0;
    a.inv_dz = 1.0f / bins->dz;
    a.cont_min = cont_min;
    a.unit_w = (flags & QFA_F_FOREST_UNIT_W) ? 1 : 0;
    a.factored = fac ? 1 : 0;
    // without a stack there are no tables: every draw in one launch
    const int step = stack ? P.Sc : S;
    a.ScMax = step;
    for (int s0 = 0; s0 < S; s0 += step) {
        a.s0 = s0;
        a.Sc = S - s0 < step ? S - s0 : step;
        if (stack && !P.lds) {
            hipError_t e = hipMemsetAsync(rows, 0, (size_t)P.rows * P.rowlen * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        by_nhm(Nh, [&](auto nhm) { launch<decltype(nhm)::value>(a, P, st); });
        if (stack) {
            const int nent = a.Sc * 4 * nbin;
            k_forest_reduce<<<(unsigned)((nent + 31) / 32), 256, 0, st>>>(rows, (int)P.rows, P.rowlen, nent, zero,
                                                                           stack + (size_t)s0 * 4 * nbin);
        }
    }
    return hip_status(st, flags);
}

}  // extern "C"
