// qfa_preprocess.hip -- C-ABI of the observed-frame preprocessing (include/qfa_hip.h: qfa_preprocess_workspace_bytes,
// qfa_preprocess_f32): argument checks and the two launches.  Kernels in qfa_preprocess.h.
#include "qfa_preprocess.h"

#include <math.h>

namespace {

using namespace qfa_preprocess;

constexpr int64_t kGrid = 2048;               // workgroups of a large call (one is resident per CU; the rest queue behind them)

bool shape_ok(int N, int Npix, int max_n_in) {
    return N >= 0 && Npix >= 1 && Npix <= kMaxNpix && max_n_in >= 0 && max_n_in <= kMaxIn;
}

size_t window_bytes(int Npix) { return ((size_t)Npix + 15) & ~(size_t)15; }

bool window_ok(double lo, double hi) { return isfinite(lo) && isfinite(hi) && lo < hi; }

}  // namespace

extern "C" {

size_t qfa_preprocess_workspace_bytes(int N, int Npix, int max_n_in) {
    if (!shape_ok(N, Npix, max_n_in)) return 0;
    return 16 + window_bytes(Npix);
}

int qfa_preprocess_f32(const double *wave, const float *flux, const float *ivar, const uint8_t *bad, const int64_t *offsets,
                       const double *zqso, int N, int max_n_in, const double *out_edges, const double *wav_grid, int Npix,
                       const qfa_preprocess_t *q, float *flux_out, float *error_out, double *record_f64,
                       int32_t *record_i32, void *workspace, size_t workspace_bytes, void *stream) {
    if (!q) return QFA_E_NULL;
    if (!shape_ok(N, Npix, max_n_in)) return QFA_E_SIZE;
    if (!(q->min_coverage > 0.0 && q->min_coverage <= 1.0) || !window_ok(q->norm_lo, q->norm_hi) ||
        !window_ok(q->snr_lo, q->snr_hi) || q->norm_min_pixels < 1)
        return QFA_E_SIZE;
    if (N == 0) return 0;
    // (a call whose spectra are all empty has no input pixels: wave, flux, ivar may then be NULL, as an empty tensor's pointer is)
    if (max_n_in > 0 && (!wave || !flux || !ivar)) return QFA_E_NULL;
    if (!offsets || !zqso || !out_edges || !wav_grid || !flux_out || !error_out || !record_f64 || !record_i32 || !workspace)
        return QFA_E_NULL;
    if (workspace_bytes < 16 + window_bytes(Npix)) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *win = (uint8_t *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    k_preprocess_windows<<<(unsigned)((Npix + 255) / 256), 256, 0, st>>>(wav_grid, Npix, q->norm_lo, q->norm_hi, q->snr_lo,
                                                                        q->snr_hi, win);
    Args a;
    a.wave = wave; a.flux = flux; a.ivar = ivar; a.bad = bad; a.offsets = offsets; a.zqso = zqso;
    a.edges = out_edges; a.win = win;
    a.flux_out = flux_out; a.error_out = error_out; a.rec_f64 = record_f64; a.rec_i32 = record_i32;
    a.N = N; a.Npix = Npix; a.max_n_in = max_n_in; a.norm_min_pixels = q->norm_min_pixels;
    a.min_coverage = q->min_coverage;
    const unsigned grid = (unsigned)((int64_t)N < kGrid ? (int64_t)N : kGrid);
    k_preprocess<<<grid, kThreads, 0, st>>>(a);
    return (int)hipGetLastError();
}

}  // extern "C"
