// qfa_p1d.hip -- C-ABI of the 1D flux power spectrum of forest segments and its (k, z) stack (include/qfa_hip.h:
// qfa_p1d_stack_doubles, qfa_p1d_workspace_bytes, qfa_p1d_f32) and of its band powers and their covariance stack
// (qfa_p1d_band_stack_doubles, qfa_p1d_band_workspace_bytes, qfa_p1d_band_chunk_segments, qfa_p1d_band_f32): argument checks, the
// launch plans and the launches; and of the pair-weighted correlation function of the same segments and its (lag, z) stack
// (qfa_xi_stack_doubles, qfa_xi_workspace_bytes, qfa_xi_f32); and of the flux PDF of the same segments and its covariance stack
// (qfa_flux_pdf_stack_doubles, qfa_flux_pdf_workspace_bytes, qfa_flux_pdf_f32).  Kernels in qfa_p1d.h, qfa_p1d_band.h, qfa_xi.h and
// qfa_pdf.h.
#include "qfa_p1d.h"
#include "qfa_p1d_band.h"
#include "qfa_xi.h"
#include "qfa_pdf.h"
#include "../../include/qfa_hip.h"

#include <math.h>

namespace {

using namespace qfa_p1d;

constexpr int kMaxBins = 4096;
constexpr int kMaxLen = 4096;
constexpr size_t kRowsTarget = (size_t)64 << 20;   // bytes of per-segment rows (code, noise, power) a launch aims at

// How a call is cut: `Bc` spectra per launch; workspace = [table L float2 | code | noise | power] of one launch from its first
// 16-byte boundary on.  (The stack does not depend on the cut: k_p1d_reduce continues the sum of the launch before.)
struct Plan {
    int M, Bc;
    size_t segs, bytes;                        // segments of a full launch
};

bool shape_ok(int R, int S, int Nb, int L, int nseg, int nz) {
    return R >= 0 && S >= 1 && R % S == 0 && Nb >= 1 && L >= 1 && L <= kMaxLen && nseg >= 1 &&
           (int64_t)nseg * L <= Nb && nz >= 1 && nz <= kMaxBins;
}

Plan make_plan(int B, int S, int L, int nseg) {
    Plan P;
    P.M = L / 2;
    const size_t per_b = (size_t)S * nseg * (size_t)(P.M + 2) * 4;
    size_t bc = kRowsTarget / per_b;
    if (bc < 1) bc = 1;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.segs = bc * S * nseg;
    P.bytes = 16 + (size_t)L * sizeof(float2) + P.segs * (size_t)(P.M + 2) * 4;
    return P;
}

// The band call's cut: launches of `Bc` spectra that end on chunk boundaries of the per-draw segment axis (Bc a multiple of
// `unit` = kChunk / gcd(kChunk, nseg)), sized so that k_p1d's rows and the chunk partials of one launch together aim at kRowsTarget;
// workspace = [table | code | noise | power | start nband + 1 | list M | partials (chunks, S, nz, W) from the next 8-byte boundary].
struct BandPlan {
    int M, Bc, W;
    size_t segs, chunks, bytes;                // segments and chunks (per draw) of a full launch
};

BandPlan make_band_plan(int B, int S, int L, int nseg, int nz, int nband, bool partials) {
    namespace pb = qfa_p1d_band;
    BandPlan P;
    P.M = L / 2;
    P.W = 1 + nband + nband * (nband + 1) / 2;
    int g = nseg, r = pb::kChunk;
    while (r) { const int t = g % r; g = r; r = t; }
    const size_t unit = (size_t)(pb::kChunk / g);
    const size_t part_row = partials ? (size_t)S * nz * (size_t)P.W * sizeof(double) : 0;
    const size_t per_unit = unit * S * nseg * (size_t)(P.M + 2) * 4 + (unit * nseg / pb::kChunk) * part_row;
    size_t nu = kRowsTarget / per_unit;
    if (nu < 1) nu = 1;
    size_t bc = nu * unit;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.segs = bc * S * nseg;
    P.chunks = (bc * nseg + pb::kChunk - 1) / pb::kChunk;
    P.bytes = 16 + (size_t)L * sizeof(float2) + P.segs * (size_t)(P.M + 2) * 4 + (size_t)(nband + 1 + P.M) * 4 + 8 +
              P.chunks * part_row;
    return P;
}

// The correlation call's cut, the band call's with other rows: launches of `Bc` spectra that end on chunk boundaries, sized so that
// k_xi's rows (code, N0, [W | A]) and the chunk partials of one launch together aim at kRowsTarget; workspace = [code | N0 | pairs |
// partials (chunks, S, nz, 2 + 5 nlag) from the next 8-byte boundary] from its first 16-byte boundary on.
struct XiPlan {
    int Bc;
    size_t segs, chunks, bytes;                // segments and chunks (per draw) of a full launch
};

XiPlan make_xi_plan(int B, int S, int nseg, int nz, int nlag) {
    namespace xi = qfa_xi;
    XiPlan P;
    int g = nseg, r = xi::kChunk;
    while (r) { const int t = g % r; g = r; r = t; }
    const size_t unit = (size_t)(xi::kChunk / g);
    const size_t part_row = (size_t)S * nz * (size_t)(2 + 5 * nlag) * sizeof(double);
    const size_t per_unit = unit * S * nseg * (size_t)(2 * nlag + 2) * 4 + (unit * nseg / xi::kChunk) * part_row;
    size_t nu = kRowsTarget / per_unit;
    if (nu < 1) nu = 1;
    size_t bc = nu * unit;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.segs = bc * S * nseg;
    P.chunks = (bc * nseg + xi::kChunk - 1) / xi::kChunk;
    P.bytes = 16 + P.segs * (size_t)(2 * nlag + 2) * 4 + 8 + P.chunks * part_row;
    return P;
}

// The PDF call's cut: nothing but the chunk partials (chunks, S, nz, 2 + nt + nt (nt + 1) / 2) int32 is held between its kernels, from
// the workspace's first 16-byte boundary on; a launch takes as many chunks as aim at kRowsTarget (at least one).  The sums are
// integers, so the result does not depend on where the cut falls.
struct PdfPlan {
    int Bc, W;
    size_t chunks, bytes;                      // chunks (per draw) of a full launch
};

PdfPlan make_pdf_plan(int B, int S, int nseg, int nz, int nt) {
    namespace pd = qfa_pdf;
    PdfPlan P;
    P.W = 2 + nt + nt * (nt + 1) / 2;
    const size_t part_row = (size_t)S * nz * (size_t)P.W * sizeof(int);
    size_t nc = kRowsTarget / part_row;
    if (nc < 1) nc = 1;
    size_t bc = nc * pd::kChunk / (size_t)nseg;
    if (bc < 1) bc = 1;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.chunks = (bc * nseg + pd::kChunk - 1) / pd::kChunk;
    P.bytes = 16 + P.chunks * part_row;
    return P;
}

// the checks qfa_p1d_f32, qfa_p1d_band_f32, qfa_xi_f32 and qfa_flux_pdf_f32 share, in qfa_p1d_f32's order: sizes, then flags
int check_sizes(const qfa_batch_t *b, int B, int S, int Nb, const qfa_p1d_t *p) {
    if (B < 0 || S < 1 || Nb < 1 || (int64_t)B * S > INT32_MAX) return QFA_E_SIZE;
    if (p->seg_len < 1 || p->seg_len > kMaxLen || p->nseg < 1 || p->p_lo < 0 ||
        (int64_t)p->p_lo + (int64_t)p->nseg * p->seg_len > Nb || p->min_used < 1)
        return QFA_E_SIZE;
    if (!(p->dz > 0.f) || !isfinite(p->dz) || !isfinite(p->z0) || p->nz < 1 || p->nz > kMaxBins) return QFA_E_SIZE;
    if (!(p->dzT > 0.f) || !isfinite(p->dzT) || !isfinite(p->zT0) || p->nT < 1 || p->nT > kMaxBins) return QFA_E_SIZE;
    if (p->St != 1 && p->St != S) return QFA_E_SIZE;
    if (b->row_stride != 0 && b->row_stride < (int64_t)Nb) return QFA_E_SIZE;
    return 0;
}

void fill_args(Args &a, const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, const float2 *tw, int S, int Nb,
               const qfa_p1d_t *p, bool fac) {
    a.bt = *b;
    a.trans = trans;
    a.ivar = ivar;
    a.tbar = tbar;
    a.tw = tw;
    a.S = S; a.St = p->St; a.Nb = Nb; a.L = p->seg_len; a.M = p->seg_len / 2; a.nseg = p->nseg; a.p_lo = p->p_lo;
    a.min_used = p->min_used;
    a.nT = p->nT; a.nz = p->nz; a.factored = fac ? 1 : 0;
    a.zT0 = p->zT0;
    a.inv_dzT = 1.0f / p->dzT;
    a.z0 = p->z0;
    a.inv_dz = 1.0f / p->dz;
}

}  // namespace

extern "C" {

size_t qfa_p1d_stack_doubles(int S, int nz, int L) {
    if (S < 1 || nz < 1 || nz > kMaxBins || L < 1 || L > kMaxLen) return 0;
    return (size_t)S * nz * (size_t)(2 + 2 * (L / 2));
}

size_t qfa_p1d_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz) {
    if (!shape_ok(R, S, Nb, L, nseg, nz)) return 0;
    return make_plan(R / S, S, L, nseg).bytes;
}

int qfa_p1d_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                const qfa_p1d_t *p, unsigned flags, float *power, float *noise, double *stack, void *workspace,
                size_t workspace_bytes, void *stream) {
    if (!trans || !ivar || !b || !tbar || !p || !workspace || (!power && !noise && !stack)) return QFA_E_NULL;
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (!fac && !b->zabs) return QFA_E_NULL;
    if (int e = check_sizes(b, B, S, Nb, p)) return e;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz;
    const Plan P = make_plan(B, S, L, nseg);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int M = P.M;
    int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0) {
        if (stack && zero) {
            hipError_t e = hipMemsetAsync(stack, 0, (size_t)S * nz * (size_t)(2 + 2 * M) * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    float2 *tw = (float2 *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    int *code = (int *)(tw + L);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    k_p1d_twiddle<<<(unsigned)((L + 255) / 256), 256, 0, st>>>(L, tw);
    Args a;
    fill_args(a, trans, ivar, b, tbar, tw, S, Nb, p, fac);
    const size_t lds = (size_t)kRows * kStride * sizeof(float) + (size_t)L * sizeof(float2);
    const unsigned gy = (unsigned)((M > 0 ? M : 1) + kModes - 1) / kModes;
    // without a stack nothing is held between the kernels: one launch writes the caller's arrays
    const int step = stack ? P.Bc : B;
    for (int b0 = 0; b0 < B; b0 += step) {
        a.b0 = b0;
        a.Bc = B - b0 < step ? B - b0 : step;
        const size_t first = (size_t)b0 * S * nseg;                               // the launch's first segment
        a.power = power ? power + first * M : (stack ? pws : nullptr);
        a.noise = noise ? noise + first : (stack ? nws : nullptr);
        a.code = stack ? code : nullptr;
        const size_t segs = (size_t)a.Bc * S * nseg;
        k_p1d<<<dim3((unsigned)((segs + kRows - 1) / kRows), gy), kThreads, lds, st>>>(a);
        if (stack) {
            k_p1d_reduce<<<dim3((unsigned)(S * nz), (unsigned)((M > 0 ? M : 1) + 255) / 256), 256, 0, st>>>(
                code, a.power, a.noise, a.Bc, S, nseg, M, nz, zero, stack);
            zero = 0;
        }
    }
    if (flags & QFA_F_SYNC) {
        hipError_t s = hipStreamSynchronize(st);
        if (s != hipSuccess) { (void)hipGetLastError(); return (int)s; }
    }
    return (int)hipGetLastError();
}

size_t qfa_p1d_band_stack_doubles(int S, int nz, int nband) {
    if (S < 1 || nz < 1 || nz > kMaxBins || nband < 1 || nband > qfa_p1d_band::kMaxBands) return 0;
    return (size_t)S * nz * (size_t)(1 + nband + nband * nband);
}

size_t qfa_p1d_band_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nband) {
    if (!shape_ok(R, S, Nb, L, nseg, nz) || nband < 1 || nband > qfa_p1d_band::kMaxBands) return 0;
    return make_band_plan(R / S, S, L, nseg, nz, nband, true).bytes;
}

int qfa_p1d_band_chunk_segments(void) { return qfa_p1d_band::kChunk; }

int qfa_p1d_band_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_p1d_band_t *q, unsigned flags, double *bandpower, double *stack,
                     void *workspace, size_t workspace_bytes, void *stream) {
    namespace pb = qfa_p1d_band;
    if (!trans || !ivar || !b || !tbar || !p || !workspace || !q || !q->band || (!bandpower && !stack)) return QFA_E_NULL;
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (!fac && !b->zabs) return QFA_E_NULL;
    if (int e = check_sizes(b, B, S, Nb, p)) return e;
    if (q->nband < 1 || q->nband > pb::kMaxBands || (q->subtract_noise != 0 && q->subtract_noise != 1)) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz, nband = q->nband;
    // (the size is that of the workspace function whether or not a stack is asked for; without one the partials' part stays unused)
    const BandPlan P = make_band_plan(B, S, L, nseg, nz, nband, true);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int M = P.M;
    const size_t Wf = (size_t)(1 + nband + nband * nband);
    int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0) {
        if (stack && zero) {
            hipError_t e = hipMemsetAsync(stack, 0, (size_t)S * nz * Wf * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    float2 *tw = (float2 *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    int *code = (int *)(tw + L);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    int *start = (int *)(pws + P.segs * (size_t)M);
    int *list = start + nband + 1;
    double *part = (double *)(((uintptr_t)(list + M) + 7) & ~(uintptr_t)7);
    k_p1d_twiddle<<<(unsigned)((L + 255) / 256), 256, 0, st>>>(L, tw);
    pb::k_p1d_band_prep<<<1, pb::kMaxBands, 0, st>>>(q->band, M, nband, start, list);
    Args a;
    fill_args(a, trans, ivar, b, tbar, tw, S, Nb, p, fac);
    a.power = pws;
    a.noise = nws;
    a.code = code;
    pb::Args ba;
    ba.power = pws;
    ba.noise = nws;
    ba.code = code;
    ba.start = start;
    ba.list = list;
    ba.weight = q->weight;
    ba.part = stack ? part : nullptr;
    ba.S = S; ba.nseg = nseg; ba.M = M; ba.nband = nband; ba.nz = nz; ba.sub = q->subtract_noise;
    const size_t lds = (size_t)kRows * kStride * sizeof(float) + (size_t)L * sizeof(float2);
    const size_t blds = (size_t)pb::kChunk * (nband + 1) * sizeof(double);
    const unsigned gy = (unsigned)((M > 0 ? M : 1) + kModes - 1) / kModes;
    for (int b0 = 0; b0 < B; b0 += P.Bc) {                                        // (every b0 nseg is a multiple of kChunk)
        a.b0 = b0;
        a.Bc = B - b0 < P.Bc ? B - b0 : P.Bc;
        const size_t segs = (size_t)a.Bc * S * nseg;
        k_p1d<<<dim3((unsigned)((segs + kRows - 1) / kRows), gy), kThreads, lds, st>>>(a);
        ba.n = a.Bc * nseg;
        ba.bandpower = bandpower ? bandpower + (size_t)b0 * S * nseg * nband : nullptr;
        const int chunks = (ba.n + pb::kChunk - 1) / pb::kChunk;
        pb::k_p1d_band<<<(unsigned)((size_t)chunks * S), pb::kThreads, blds, st>>>(ba);
        if (stack) {
            pb::k_p1d_band_reduce<<<dim3((unsigned)(S * nz), (unsigned)((Wf + 255) / 256)), 256, 0, st>>>(part, chunks, S, nz, nband,
                                                                                                         zero, stack);
            zero = 0;
        }
    }
    if (flags & QFA_F_SYNC) {
        hipError_t s = hipStreamSynchronize(st);
        if (s != hipSuccess) { (void)hipGetLastError(); return (int)s; }
    }
    return (int)hipGetLastError();
}

size_t qfa_xi_stack_doubles(int S, int nz, int nlag) {
    if (S < 1 || nz < 1 || nz > kMaxBins || nlag < 1 || nlag > kMaxLen) return 0;
    return (size_t)S * nz * (size_t)(2 + 5 * nlag);
}

size_t qfa_xi_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nlag) {
    if (!shape_ok(R, S, Nb, L, nseg, nz) || nlag < 1 || nlag > L) return 0;
    return make_xi_plan(R / S, S, nseg, nz, nlag).bytes;
}

int qfa_xi_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
               const qfa_p1d_t *p, const qfa_xi_t *x, unsigned flags, float *pairs, float *noise0, double *stack, void *workspace,
               size_t workspace_bytes, void *stream) {
    namespace xi = qfa_xi;
    if (!trans || !ivar || !b || !tbar || !p || !workspace || !x || (!pairs && !noise0 && !stack)) return QFA_E_NULL;
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (!fac && !b->zabs) return QFA_E_NULL;
    if (int e = check_sizes(b, B, S, Nb, p)) return e;
    if (x->nlag < 1 || x->nlag > p->seg_len || !(x->sigma2_lss >= 0.f) || !isfinite(x->sigma2_lss)) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_XI_UNIT_W)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz, nlag = x->nlag;
    const XiPlan P = make_xi_plan(B, S, nseg, nz, nlag);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t Wd = (size_t)(2 + 5 * nlag);
    int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0) {
        if (stack && zero) {
            hipError_t e = hipMemsetAsync(stack, 0, (size_t)S * nz * Wd * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    int *code = (int *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    double *part = (double *)(((uintptr_t)(pws + P.segs * 2 * (size_t)nlag) + 7) & ~(uintptr_t)7);
    xi::Args a;
    a.bt = *b;
    a.trans = trans;
    a.ivar = ivar;
    a.tbar = tbar;
    a.S = S; a.St = p->St; a.Nb = Nb; a.L = L; a.nlag = nlag; a.nseg = nseg; a.p_lo = p->p_lo; a.min_used = p->min_used;
    a.nT = p->nT; a.nz = nz; a.factored = fac ? 1 : 0; a.unit_w = (flags & QFA_F_XI_UNIT_W) ? 1 : 0;
    a.tile = xi::make_tile(L, nlag);
    a.zT0 = p->zT0;
    a.inv_dzT = 1.0f / p->dzT;
    a.z0 = p->z0;
    a.inv_dz = 1.0f / p->dz;
    a.sigma2 = x->sigma2_lss;
    xi::StackArgs sa;
    sa.code = code;
    sa.part = part;
    sa.S = S; sa.nseg = nseg; sa.nlag = nlag; sa.nz = nz;
    const size_t lds = (size_t)(a.tile.dup ? 4 : 2) * a.tile.Ls * sizeof(float);
    // without a stack nothing is held between the kernels: one launch writes the caller's arrays
    const int step = stack ? P.Bc : B;
    for (int b0 = 0; b0 < B; b0 += step) {                                        // (with a stack every b0 nseg is a multiple of kChunk)
        a.b0 = b0;
        a.Bc = B - b0 < step ? B - b0 : step;
        const size_t first = (size_t)b0 * S * nseg;                               // the launch's first segment
        a.pairs = pairs ? pairs + first * 2 * (size_t)nlag : (stack ? pws : nullptr);
        a.noise0 = noise0 ? noise0 + first : (stack ? nws : nullptr);
        a.code = stack ? code : nullptr;
        const size_t segs = (size_t)a.Bc * S * nseg;
        const size_t gx = segs < ((size_t)1 << 20) ? segs : ((size_t)1 << 20);
        xi::k_xi<<<dim3((unsigned)gx, (unsigned)((segs + gx - 1) / gx)), xi::kThreads, lds, st>>>(a);
        if (stack) {
            sa.pairs = a.pairs;
            sa.noise0 = a.noise0;
            sa.n = a.Bc * nseg;
            const int chunks = (sa.n + xi::kChunk - 1) / xi::kChunk;
            xi::k_xi_stack<<<(unsigned)((size_t)chunks * S), xi::kThreads, 0, st>>>(sa);
            xi::k_xi_reduce<<<dim3((unsigned)(S * nz), (unsigned)((Wd + 255) / 256)), 256, 0, st>>>(part, chunks, S, nz, nlag, zero,
                                                                                                   stack);
            zero = 0;
        }
    }
    if (flags & QFA_F_SYNC) {
        hipError_t s = hipStreamSynchronize(st);
        if (s != hipSuccess) { (void)hipGetLastError(); return (int)s; }
    }
    return (int)hipGetLastError();
}

size_t qfa_flux_pdf_stack_doubles(int S, int nz, int nt) {
    if (S < 1 || nz < 1 || nz > kMaxBins || nt < 1 || nt > qfa_pdf::kMaxBins) return 0;
    return (size_t)S * nz * (size_t)(2 + nt + nt * nt);
}

size_t qfa_flux_pdf_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nt) {
    if (!shape_ok(R, S, Nb, L, nseg, nz) || nt < 1 || nt > qfa_pdf::kMaxBins) return 0;
    return make_pdf_plan(R / S, S, nseg, nz, nt).bytes;
}

int qfa_flux_pdf_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_pdf_t *q, unsigned flags, int *hist, double *stack, void *workspace,
                     size_t workspace_bytes, void *stream) {
    namespace pd = qfa_pdf;
    if (!trans || !ivar || !b || !tbar || !p || !workspace || !q || (!hist && !stack)) return QFA_E_NULL;
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (!fac && !b->zabs) return QFA_E_NULL;
    if (int e = check_sizes(b, B, S, Nb, p)) return e;
    if (q->nt < 1 || q->nt > pd::kMaxBins || !(q->dt > 0.f) || !isfinite(q->dt) || !isfinite(q->t0) || !(q->ivar_min >= 0.f) ||
        !isfinite(q->ivar_min))
        return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_PDF_RELATIVE | QFA_F_PDF_CLAMP)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz, nt = q->nt;
    const PdfPlan P = make_pdf_plan(B, S, nseg, nz, nt);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t Wf = (size_t)(2 + nt + nt * nt);
    int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0) {
        if (stack && zero) {
            hipError_t e = hipMemsetAsync(stack, 0, (size_t)S * nz * Wf * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    pd::Args a;
    a.bt = *b;
    a.trans = trans;
    a.ivar = ivar;
    a.tbar = tbar;
    a.hist = hist;
    a.part = stack ? (int *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15) : nullptr;
    a.S = S; a.St = p->St; a.Nb = Nb; a.L = L; a.nseg = nseg; a.p_lo = p->p_lo; a.min_used = p->min_used;
    a.nT = p->nT; a.nz = nz; a.factored = fac ? 1 : 0; a.nt = nt;
    a.relative = (flags & QFA_F_PDF_RELATIVE) ? 1 : 0;
    a.clamp = (flags & QFA_F_PDF_CLAMP) ? 1 : 0;
    a.zT0 = p->zT0;
    a.inv_dzT = 1.0f / p->dzT;
    a.z0 = p->z0;
    a.inv_dz = 1.0f / p->dz;
    a.t0 = q->t0;
    a.inv_dt = 1.0f / q->dt;
    a.ivar_min = q->ivar_min;
    const size_t lds = (size_t)pd::kChunk * (nt + 2) * sizeof(int);
    // without a stack nothing is held between the kernels: launches as large as the grid allows write the caller's array
    size_t cap = (((size_t)1 << 30) / (size_t)S) * pd::kChunk / (size_t)nseg;
    if (cap < 1) cap = 1;
    const int step = stack ? P.Bc : (int)(cap < (size_t)B ? cap : (size_t)B);
    for (int b0 = 0; b0 < B; b0 += step) {
        a.b0 = b0;
        a.Bc = B - b0 < step ? B - b0 : step;
        const int chunks = (int)(((size_t)a.Bc * nseg + pd::kChunk - 1) / pd::kChunk);
        pd::k_pdf<<<(unsigned)((size_t)chunks * S), pd::kThreads, lds, st>>>(a);
        if (stack) {
            pd::k_pdf_reduce<<<dim3((unsigned)(S * nz), (unsigned)((Wf + 255) / 256)), 256, 0, st>>>(a.part, chunks, S, nz, nt, zero,
                                                                                                    stack);
            zero = 0;
        }
    }
    if (flags & QFA_F_SYNC) {
        hipError_t s = hipStreamSynchronize(st);
        if (s != hipSuccess) { (void)hipGetLastError(); return (int)s; }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
