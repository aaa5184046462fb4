// qfa_p1d.hip -- C-ABI of the 1D flux power spectrum of forest segments and its (k, z) stack (include/qfa_hip.h:
// qfa_p1d_stack_doubles, qfa_p1d_workspace_bytes, qfa_p1d_f32) and of its band powers and their covariance stack
// (qfa_p1d_band_stack_doubles, qfa_p1d_band_workspace_bytes, qfa_p1d_band_chunk_segments, qfa_p1d_band_f32): argument checks, the
// launch plans and the launches; and of the pair-weighted correlation function of the same segments and its (lag, z) stack
// (qfa_xi_stack_doubles, qfa_xi_workspace_bytes, qfa_xi_f32); and of the flux PDF of the same segments and its covariance stack
// (qfa_flux_pdf_stack_doubles, qfa_flux_pdf_workspace_bytes, qfa_flux_pdf_f32); and of the variance function of the same segments
// and its (v-bin, z) stack (qfa_variance_stack_doubles, qfa_variance_workspace_bytes, qfa_variance_f32); and of the z-bin codes of
// the same segments (qfa_segment_codes_f32, what the sightline bootstrap of qfa_bootstrap.hip sorts its rows by).  Kernels in qfa_p1d.h,
// qfa_p1d_band.h, qfa_xi.h, qfa_pdf.h, qfa_variance.h and qfa_bootstrap.h.
#include "qfa_p1d.h"
#include "qfa_p1d_band.h"
#include "qfa_xi.h"
#include "qfa_pdf.h"
#include "qfa_variance.h"
#include "qfa_bootstrap.h"
#include "qfa_call.h"

#include <math.h>

namespace {

using namespace qfa_p1d;
using qfa_segment::kChunk;

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

// The cut of a call whose stack is summed by chunks (band powers, xi): launches of `Bc` spectra that end on chunk boundaries of the
// per-draw segment axis (Bc a multiple of `unit` = kChunk / gcd(kChunk, nseg)), sized so that the per-segment rows (`seg_bytes` a
// segment) and the chunk partials (`part_row` bytes a chunk) of one launch together aim at kRowsTarget; `fixed`: the bytes of the
// workspace in front of and between the two.
struct ChunkPlan {
    int Bc;
    size_t segs, chunks, bytes;                // segments and chunks (per draw) of a full launch
};

ChunkPlan make_chunk_plan(int B, int S, int nseg, size_t seg_bytes, size_t part_row, size_t fixed) {
    ChunkPlan P;
    int g = nseg, r = kChunk;
    while (r) { const int t = g % r; g = r; r = t; }
    const size_t unit = (size_t)(kChunk / g);
    const size_t per_unit = unit * S * nseg * seg_bytes + (unit * nseg / kChunk) * part_row;
    size_t nu = kRowsTarget / per_unit;
    if (nu < 1) nu = 1;
    size_t bc = nu * unit;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.segs = bc * S * nseg;
    P.chunks = (bc * nseg + kChunk - 1) / kChunk;
    P.bytes = fixed + P.segs * seg_bytes + P.chunks * part_row;
    return P;
}

// the band call: workspace = [table | code | noise | power | start nband + 1 | list M | partials (chunks, S, nz, W) from the next
// 8-byte boundary] from its first 16-byte boundary on, W = 1 + nband + nband (nband + 1) / 2
ChunkPlan make_band_plan(int B, int S, int L, int nseg, int nz, int nband) {
    const int M = L / 2, W = 1 + nband + nband * (nband + 1) / 2;
    return make_chunk_plan(B, S, nseg, (size_t)(M + 2) * 4, (size_t)S * nz * (size_t)W * sizeof(double),
                           16 + (size_t)L * sizeof(float2) + (size_t)(nband + 1 + M) * 4 + 8);
}

// the correlation call: workspace = [code | N0 | pairs | partials (chunks, S, nz, 2 + 5 nlag) from the next 8-byte boundary]
ChunkPlan make_xi_plan(int B, int S, int nseg, int nz, int nlag) {
    return make_chunk_plan(B, S, nseg, (size_t)(2 * nlag + 2) * 4, (size_t)S * nz * (size_t)(2 + 5 * nlag) * sizeof(double), 16 + 8);
}

// The PDF call's cut: nothing but the chunk partials (chunks, S, nz, 2 + nt + nt (nt + 1) / 2) int32 is held between its kernels, from
// the workspace's first 16-byte boundary on; a launch takes as many chunks as aim at kRowsTarget (at least one), on no chunk
// boundary: the sums are integers, so the result does not depend on where the cut falls.
struct PdfPlan {
    int Bc;
    size_t chunks, bytes;                      // chunks (per draw) of a full launch
};

PdfPlan make_pdf_plan(int B, int S, int nseg, int nz, int nt) {
    PdfPlan P;
    const size_t part_row = (size_t)S * nz * (size_t)(2 + nt + nt * (nt + 1) / 2) * sizeof(int);
    size_t nc = kRowsTarget / part_row;
    if (nc < 1) nc = 1;
    size_t bc = nc * kChunk / (size_t)nseg;
    if (bc < 1) bc = 1;
    if (bc > (size_t)(B > 0 ? B : 1)) bc = (size_t)(B > 0 ? B : 1);
    P.Bc = (int)bc;
    P.chunks = (bc * nseg + kChunk - 1) / kChunk;
    P.bytes = 16 + P.chunks * part_row;
    return P;
}

// the variance call: workspace = [code | rows (segments, 1 + 5 nv) from the next 8-byte boundary | partials (chunks, S, nz, 2 + 5 nv)]
// from its first 16-byte boundary on
ChunkPlan make_var_plan(int B, int S, int nseg, int nz, int nv) {
    return make_chunk_plan(B, S, nseg, 4 + (size_t)(1 + 5 * nv) * sizeof(double), (size_t)S * nz * (size_t)(2 + 5 * nv) * sizeof(double),
                           16 + 8 + 8);
}

// The checks the five calls share behind their own NULL checks, in qfa_p1d_f32's order: the redshift form (`fac`: zq1 x pix_ratio),
// then the sizes.  The statistic's own sizes and the flags follow in the caller.
int check_call(const qfa_batch_t *b, int B, int S, int Nb, const qfa_p1d_t *p, bool &fac) {
    fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (!fac && !b->zabs) return QFA_E_NULL;
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

// the fields the Args of k_p1d, k_xi, k_pdf and k_var share (qfa_segment.h)
template <typename A>
void seg_args(A &a, const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int S, int Nb, const qfa_p1d_t *p,
              bool fac) {
    a.bt = *b;
    a.trans = trans;
    a.ivar = ivar;
    a.tbar = tbar;
    a.b0 = 0; a.Bc = 0;
    a.S = S; a.St = p->St; a.Nb = Nb; a.L = p->seg_len; a.nseg = p->nseg; a.p_lo = p->p_lo; a.min_used = p->min_used;
    a.nT = p->nT; a.nz = p->nz; a.factored = fac ? 1 : 0;
    a.zT0 = p->zT0;
    a.inv_dzT = 1.0f / p->dzT;
    a.z0 = p->z0;
    a.inv_dz = 1.0f / p->dz;
}

template <typename T>
T *aligned(void *p, uintptr_t to) { return (T *)(((uintptr_t)p + (to - 1)) & ~(to - 1)); }

// The body of a call behind its checks.  No spectra: a stack of `doubles` that QFA_F_ZERO_ACCUM asks to start from zero is cleared.
// Else launches of `step` spectra: launch(zero) finds a.b0 and a.Bc set, and `zero` set for the first launch that adds to a stack
// under QFA_F_ZERO_ACCUM (every later one continues the sum).  Then the QFA_F_SYNC tail.
template <typename A, typename F>
int run_call(A &a, int B, int step, unsigned flags, double *stack, size_t doubles, hipStream_t st, F &&launch) {
    int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0) return stack && zero ? (int)hipMemsetAsync(stack, 0, doubles * sizeof(double), st) : 0;
    for (int b0 = 0; b0 < B; b0 += step) {
        a.b0 = b0;
        a.Bc = B - b0 < step ? B - b0 : step;
        launch(zero);
        if (stack) zero = 0;
    }
    return hip_status(st, flags);
}

// stack (S, nz, head + n^2) += the partials (chunks, S, nz, head + n (n + 1) / 2) of a launch
template <typename T>
void chunk_reduce(const T *part, int chunks, int S, int nz, int head, int n, int zero, double *stack, hipStream_t st) {
    qfa_segment::k_chunk_reduce<T><<<dim3((unsigned)(S * nz), (unsigned)((head + n * n + 255) / 256)), 256, 0, st>>>(part, chunks, S, nz, head,
                                                                                                                     n, zero, stack);
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
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz;
    const Plan P = make_plan(B, S, L, nseg);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int M = P.M;
    float2 *tw = aligned<float2>(workspace, 16);
    int *code = (int *)(tw + L);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    Args a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.tw = tw;
    a.M = M;
    const size_t lds = (size_t)kRows * kStride * sizeof(float) + (size_t)L * sizeof(float2);
    const unsigned gy = (unsigned)((M > 0 ? M : 1) + kModes - 1) / kModes;
    if (B > 0) k_p1d_twiddle<<<(unsigned)((L + 255) / 256), 256, 0, st>>>(L, tw);
    // without a stack nothing is held between the kernels: one launch writes the caller's arrays
    return run_call(a, B, stack ? P.Bc : B, flags, stack, qfa_p1d_stack_doubles(S, nz, L), st, [&](int zero) {
        const size_t first = (size_t)a.b0 * S * nseg;                             // the launch's first segment
        a.power = power ? power + first * M : (stack ? pws : nullptr);
        a.noise = noise ? noise + first : (stack ? nws : nullptr);
        a.code = stack ? code : nullptr;
        const size_t segs = (size_t)a.Bc * S * nseg;
        k_p1d<<<dim3((unsigned)((segs + kRows - 1) / kRows), gy), kThreads, lds, st>>>(a);
        if (stack)
            k_p1d_reduce<<<dim3((unsigned)(S * nz), (unsigned)((M > 0 ? M : 1) + 255) / 256), 256, 0, st>>>(
                code, a.power, a.noise, a.Bc, S, nseg, M, nz, zero, stack);
    });
}

size_t qfa_p1d_band_stack_doubles(int S, int nz, int nband) {
    if (S < 1 || nz < 1 || nz > kMaxBins || nband < 1 || nband > qfa_p1d_band::kMaxBands) return 0;
    return (size_t)S * nz * (size_t)(1 + nband + nband * nband);
}

size_t qfa_p1d_band_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nband) {
    if (!shape_ok(R, S, Nb, L, nseg, nz) || nband < 1 || nband > qfa_p1d_band::kMaxBands) return 0;
    return make_band_plan(R / S, S, L, nseg, nz, nband).bytes;
}

int qfa_p1d_band_chunk_segments(void) { return kChunk; }

int qfa_p1d_band_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_p1d_band_t *q, unsigned flags, double *bandpower, double *stack,
                     void *workspace, size_t workspace_bytes, void *stream) {
    namespace pb = qfa_p1d_band;
    if (!trans || !ivar || !b || !tbar || !p || !workspace || !q || !q->band || (!bandpower && !stack)) return QFA_E_NULL;
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if (q->nband < 1 || q->nband > pb::kMaxBands || (q->subtract_noise != 0 && q->subtract_noise != 1)) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz, nband = q->nband;
    // (the size is that of the workspace function whether or not a stack is asked for; without one the partials' part stays unused)
    const ChunkPlan P = make_band_plan(B, S, L, nseg, nz, nband);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int M = L / 2;
    float2 *tw = aligned<float2>(workspace, 16);
    int *code = (int *)(tw + L);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    int *start = (int *)(pws + P.segs * (size_t)M);
    int *list = start + nband + 1;
    double *part = aligned<double>(list + M, 8);
    Args a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.tw = tw;
    a.M = M;
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
    const size_t blds = (size_t)kChunk * (nband + 1) * sizeof(double);
    const unsigned gy = (unsigned)((M > 0 ? M : 1) + kModes - 1) / kModes;
    if (B > 0) {
        k_p1d_twiddle<<<(unsigned)((L + 255) / 256), 256, 0, st>>>(L, tw);
        pb::k_p1d_band_prep<<<1, pb::kMaxBands, 0, st>>>(q->band, M, nband, start, list);
    }
    // (every b0 nseg is a multiple of kChunk)
    return run_call(a, B, P.Bc, flags, stack, qfa_p1d_band_stack_doubles(S, nz, nband), st, [&](int zero) {
        const size_t segs = (size_t)a.Bc * S * nseg;
        k_p1d<<<dim3((unsigned)((segs + kRows - 1) / kRows), gy), kThreads, lds, st>>>(a);
        ba.n = a.Bc * nseg;
        ba.bandpower = bandpower ? bandpower + (size_t)a.b0 * S * nseg * nband : nullptr;
        const int chunks = (ba.n + kChunk - 1) / kChunk;
        pb::k_p1d_band<<<(unsigned)((size_t)chunks * S), pb::kThreads, blds, st>>>(ba);
        if (stack) chunk_reduce(part, chunks, S, nz, 1 + nband, nband, zero, stack, st);
    });
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
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if (x->nlag < 1 || x->nlag > p->seg_len || !(x->sigma2_lss >= 0.f) || !isfinite(x->sigma2_lss)) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_XI_UNIT_W)) return QFA_E_FLAGS;
    const int L = p->seg_len, nseg = p->nseg, nz = p->nz, nlag = x->nlag;
    const ChunkPlan P = make_xi_plan(B, S, nseg, nz, nlag);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int *code = aligned<int>(workspace, 16);
    float *nws = (float *)(code + P.segs);
    float *pws = nws + P.segs;
    double *part = aligned<double>(pws + P.segs * 2 * (size_t)nlag, 8);
    xi::Args a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.nlag = nlag;
    a.unit_w = (flags & QFA_F_XI_UNIT_W) ? 1 : 0;
    a.tile = xi::make_tile(L, nlag);
    a.sigma2 = x->sigma2_lss;
    xi::StackArgs sa;
    sa.code = code;
    sa.part = part;
    sa.S = S; sa.nseg = nseg; sa.nlag = nlag; sa.nz = nz;
    const size_t lds = (size_t)(a.tile.dup ? 4 : 2) * a.tile.Ls * sizeof(float);
    // without a stack nothing is held between the kernels: one launch writes the caller's arrays
    // (with a stack every b0 nseg is a multiple of kChunk)
    return run_call(a, B, stack ? P.Bc : B, flags, stack, qfa_xi_stack_doubles(S, nz, nlag), st, [&](int zero) {
        const size_t first = (size_t)a.b0 * S * nseg;                             // the launch's first segment
        a.pairs = pairs ? pairs + first * 2 * (size_t)nlag : (stack ? pws : nullptr);
        a.noise0 = noise0 ? noise0 + first : (stack ? nws : nullptr);
        a.code = stack ? code : nullptr;
        const size_t segs = (size_t)a.Bc * S * nseg;
        const size_t gx = segs < ((size_t)1 << 20) ? segs : ((size_t)1 << 20);
        xi::k_xi<<<dim3((unsigned)gx, (unsigned)((segs + gx - 1) / gx)), xi::kThreads, lds, st>>>(a);
        if (!stack) return;
        sa.pairs = a.pairs;
        sa.noise0 = a.noise0;
        sa.n = a.Bc * nseg;
        const int chunks = (sa.n + kChunk - 1) / kChunk;
        xi::k_xi_stack<<<(unsigned)((size_t)chunks * S), xi::kThreads, 0, st>>>(sa);
        chunk_reduce(part, chunks, S, nz, 2 + 5 * nlag, 0, zero, stack, st);
    });
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
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if (q->nt < 1 || q->nt > pd::kMaxBins || !(q->dt > 0.f) || !isfinite(q->dt) || !isfinite(q->t0) || !(q->ivar_min >= 0.f) ||
        !isfinite(q->ivar_min))
        return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_PDF_RELATIVE | QFA_F_PDF_CLAMP)) return QFA_E_FLAGS;
    const int nseg = p->nseg, nz = p->nz, nt = q->nt;
    const PdfPlan P = make_pdf_plan(B, S, nseg, nz, nt);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    pd::Args a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.hist = hist;
    a.part = stack ? aligned<int>(workspace, 16) : nullptr;
    a.nt = nt;
    a.relative = (flags & QFA_F_PDF_RELATIVE) ? 1 : 0;
    a.clamp = (flags & QFA_F_PDF_CLAMP) ? 1 : 0;
    a.t0 = q->t0;
    a.inv_dt = 1.0f / q->dt;
    a.ivar_min = q->ivar_min;
    const size_t lds = (size_t)kChunk * (nt + 2) * sizeof(int);
    // without a stack nothing is held between the kernels: launches as large as the grid allows write the caller's array
    size_t cap = (((size_t)1 << 30) / (size_t)S) * kChunk / (size_t)nseg;
    if (cap < 1) cap = 1;
    const int step = stack ? P.Bc : (int)(cap < (size_t)B ? cap : (size_t)B);
    return run_call(a, B, step, flags, stack, qfa_flux_pdf_stack_doubles(S, nz, nt), st, [&](int zero) {
        const int chunks = (int)(((size_t)a.Bc * nseg + kChunk - 1) / kChunk);
        pd::k_pdf<<<(unsigned)((size_t)chunks * S), pd::kThreads, lds, st>>>(a);
        if (stack) chunk_reduce(a.part, chunks, S, nz, 2 + nt, nt, zero, stack, st);
    });
}

size_t qfa_variance_stack_doubles(int S, int nz, int nv) {
    if (S < 1 || nz < 1 || nz > kMaxBins || nv < 1 || nv > qfa_variance::kMaxBins) return 0;
    return (size_t)S * nz * (size_t)(2 + 5 * nv);
}

size_t qfa_variance_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nv) {
    if (!shape_ok(R, S, Nb, L, nseg, nz) || nv < 1 || nv > qfa_variance::kMaxBins) return 0;
    return make_var_plan(R / S, S, nseg, nz, nv).bytes;
}

int qfa_variance_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_var_t *q, unsigned flags, double *moments, double *stack, void *workspace,
                     size_t workspace_bytes, void *stream) {
    namespace vf = qfa_variance;
    if (!trans || !ivar || !b || !tbar || !p || !workspace || !q || (!moments && !stack)) return QFA_E_NULL;
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if (q->sub < 0 || q->sub > 4 || q->n_oct < 1 || q->n_oct > vf::kMaxBins || (q->n_oct << q->sub) > vf::kMaxBins || q->e_lo < -126 ||
        (int64_t)q->e_lo + q->n_oct > 127 || !(q->d_max > 0.f))
        return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const int nseg = p->nseg, nz = p->nz, nv = q->n_oct << q->sub;
    const ChunkPlan P = make_var_plan(B, S, nseg, nz, nv);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t W = 1 + 5 * (size_t)nv;
    int *code = aligned<int>(workspace, 16);
    double *rows = aligned<double>(code + P.segs, 8);
    double *part = rows + P.segs * W;
    vf::Args a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.moments = moments;
    a.nv = nv;
    a.shift = 23 - q->sub;
    a.c0 = (q->e_lo + 127) << q->sub;
    a.d_max = q->d_max;
    vf::StackArgs sa;
    sa.rows = rows;
    sa.code = code;
    sa.part = part;
    sa.S = S; sa.nseg = nseg; sa.nv = nv; sa.nz = nz;
    // without a stack nothing is held between the kernels: one launch writes the caller's array
    // (with a stack every b0 nseg is a multiple of kChunk)
    return run_call(a, B, stack ? P.Bc : B, flags, stack, qfa_variance_stack_doubles(S, nz, nv), st, [&](int zero) {
        a.rows = stack ? rows : nullptr;
        a.code = stack ? code : nullptr;
        const size_t segs = (size_t)a.Bc * S * nseg;
        const size_t gx = segs < ((size_t)1 << 20) ? segs : ((size_t)1 << 20);
        vf::k_var<<<dim3((unsigned)gx, (unsigned)((segs + gx - 1) / gx)), vf::kThreads, 0, st>>>(a);
        if (!stack) return;
        sa.n = a.Bc * nseg;
        const int chunks = (sa.n + kChunk - 1) / kChunk;
        vf::k_var_stack<<<(unsigned)((size_t)chunks * S), vf::kThreads, 0, st>>>(sa);
        chunk_reduce(part, chunks, S, nz, 2 + 5 * nv, 0, zero, stack, st);
    });
}

int qfa_segment_codes_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                          const qfa_p1d_t *p, int32_t *codes, void *stream) {
    namespace bt = qfa_bootstrap;
    if (!trans || !ivar || !b || !tbar || !p || !codes) return QFA_E_NULL;
    bool fac;
    if (int e = check_call(b, B, S, Nb, p, fac)) return e;
    if ((int64_t)B * S * p->nseg > INT32_MAX) return QFA_E_SIZE;
    if (B == 0) return 0;
    bt::CodeArgs a;
    seg_args(a, trans, ivar, b, tbar, S, Nb, p, fac);
    a.Bc = B;
    a.codes = codes;
    const size_t segs = (size_t)B * S * p->nseg;
    constexpr size_t per = bt::kCodeThreads / 64;
    bt::k_segment_codes<<<(unsigned)((segs + per - 1) / per), bt::kCodeThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // extern "C"
