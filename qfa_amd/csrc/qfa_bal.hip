// qfa_bal.hip -- C-ABI of the BAL finder (include/qfa_hip.h: qfa_bal_scan_f32, qfa_bal_mask_f32): argument checks, the launch shape
// and the launches.  Kernels in qfa_bal.h.
#include "qfa_bal.h"
#include "qfa_call.h"

#include <math.h>

namespace {

using namespace qfa_bal;

constexpr int64_t kBlocks = 4096;             // blocks a call aims at before it cuts the draws of a (spectrum, line) into groups
constexpr int64_t kMaskGrid = 2048;

}  // namespace

extern "C" {

int qfa_bal_scan_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, int B, int S, int Npix, int Nb, int Nh,
                     const qfa_bal_t *q, float cont_min, unsigned flags, double *value, double *var, int32_t *counts,
                     int32_t *line_counts, double *troughs, void *stream) {
    if (!b || !q) return QFA_E_NULL;
    if (B < 0 || S < 1 || Npix < 1 || Nb < 0 || Nb > Npix || Nh < 1 || Nh > 32) return QFA_E_SIZE;
    if (q->n_lines < 1 || q->n_lines > QFA_BAL_MAX_LINES || q->n_indices < 1 || q->n_indices > QFA_BAL_MAX_INDICES) return QFA_E_SIZE;
    if (q->trough_index < 0 || q->trough_index >= q->n_indices) return QFA_E_SIZE;
    if (q->smooth < 1 || q->smooth > 15 || (q->smooth & 1) == 0 || q->max_gap < 0 || q->max_gap > 16) return QFA_E_SIZE;
    if (!(q->thr > 0.0) || !isfinite(q->thr)) return QFA_E_SIZE;
    int nmax = 0;
    for (int l = 0; l < q->n_lines; ++l) {
        if (!q->vedge[l]) return QFA_E_NULL;
        if (q->p_lo[l] < Nb || q->p_lo[l] > q->p_hi[l] || q->p_hi[l] > Npix) return QFA_E_SIZE;
        if (q->p_hi[l] - q->p_lo[l] > kMaxWin) return QFA_E_SIZE;
        if (q->p_hi[l] - q->p_lo[l] > nmax) nmax = q->p_hi[l] - q->p_lo[l];
    }
    for (int x = 0; x < q->n_indices; ++x) {
        const qfa_bal_index_t &ix = q->index[x];
        if (!isfinite(ix.v_lo) || !isfinite(ix.v_hi) || !(ix.v_lo < ix.v_hi) || !(ix.w_min >= 0.0) || !isfinite(ix.w_min) ||
            (ix.mode != QFA_BAL_WHOLE && ix.mode != QFA_BAL_AFTER))
            return QFA_E_SIZE;
    }
    if (b->row_stride != 0 && b->row_stride < (int64_t)Npix) return QFA_E_SIZE;
    if ((int64_t)B * S * q->n_lines > ((int64_t)1 << 30)) return QFA_E_SIZE;
    if (flags & ~QFA_F_SYNC) return QFA_E_FLAGS;
    if (B == 0) return 0;
    if (!F || !mu || !h || !value || !var || !counts || !line_counts || !troughs || !b->delta || !b->error) return QFA_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    Args a;
    a.bt = norm_batch(*b, Npix);
    a.F = F; a.mu = mu; a.h = h;
    for (int l = 0; l < QFA_BAL_MAX_LINES; ++l) {
        const bool on = l < q->n_lines;
        a.vedge[l] = on ? q->vedge[l] : nullptr;
        a.p_lo[l] = on ? q->p_lo[l] : 0;
        a.p_hi[l] = on ? q->p_hi[l] : 0;
    }
    for (int x = 0; x < QFA_BAL_MAX_INDICES; ++x) a.index[x] = q->index[x < q->n_indices ? x : 0];
    a.thr = q->thr;
    a.value = value; a.var = var; a.troughs = troughs; a.counts = counts; a.line_counts = line_counts;
    a.B = B; a.S = S; a.Npix = Npix; a.Nh = Nh; a.n_lines = q->n_lines; a.n_indices = q->n_indices;
    a.smooth = q->smooth; a.max_gap = q->max_gap; a.trough_index = q->trough_index;
    // the draws of a (spectrum, line) are cut into groups when the call has few of those; a draw's result does not depend on the cut
    const int64_t pairs = (int64_t)B * q->n_lines;
    int64_t nsg = (kBlocks + pairs - 1) / pairs;
    if (nsg > S) nsg = S;
    if (nsg < 1) nsg = 1;
    a.spg = (int)((S + nsg - 1) / nsg);
    a.nsg = (S + a.spg - 1) / a.spg;
    a.nmax = (nmax + 7) & ~7;
    if (a.nmax < 8) a.nmax = 8;
    a.cont_min = cont_min;
    const size_t lds = (size_t)a.nmax * kLdsPerPixel;
    const unsigned grid = (unsigned)(pairs * a.nsg);
    by_nhm(Nh, [&](auto nhm) { k_bal_scan<decltype(nhm)::value><<<grid, kWave, lds, st>>>(a); });
    return hip_status(st, flags);
}

int qfa_bal_mask_f32(const unsigned char *mask_in, const double *wav, const double *troughs, int B, int S, int n_lines, int s_ref,
                     int Npix, const double *mask_lines, int n_mask_lines, double pad_kms, unsigned char *mask_out, int32_t *n_masked,
                     void *stream) {
    if (B < 0 || S < 1 || Npix < 1 || n_lines < 1 || n_lines > QFA_BAL_MAX_LINES || s_ref < 0 || s_ref >= S || n_mask_lines < 1 ||
        n_mask_lines > QFA_BAL_MAX_LINES || !(pad_kms >= 0.0) || !isfinite(pad_kms))
        return QFA_E_SIZE;
    if (!mask_lines) return QFA_E_NULL;
    for (int l = 0; l < n_mask_lines; ++l)
        if (!(mask_lines[l] > 0.0) || !isfinite(mask_lines[l])) return QFA_E_SIZE;
    if (B == 0) return 0;
    if (!wav || !troughs || !mask_out || !n_masked) return QFA_E_NULL;
    MaskArgs a;
    a.mask_in = mask_in; a.wav = wav; a.troughs = troughs; a.mask_out = mask_out; a.n_masked = n_masked;
    for (int l = 0; l < QFA_BAL_MAX_LINES; ++l) a.lam[l] = l < n_mask_lines ? mask_lines[l] : 0.0;
    a.pad = pad_kms;
    a.B = B; a.S = S; a.L = n_lines; a.s_ref = s_ref; a.Npix = Npix; a.nlam = n_mask_lines;
    const unsigned grid = (unsigned)((int64_t)B < kMaskGrid ? (int64_t)B : kMaskGrid);
    k_bal_mask<<<grid, kMaskThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // extern "C"
