// qfa_absorber.hip -- C-ABI of the absorber / bad-wavelength masking (include/qfa_hip.h: qfa_absorber_workspace_bytes,
// qfa_absorber_mask_f32): argument checks and the launch.  Kernel in qfa_absorber.h.
#include "qfa_absorber.h"

#include <math.h>

namespace {

using namespace qfa_absorber;

constexpr int64_t kGrid = 2048;               // workgroups of a large call (eight of 256 threads per CU; the rest queue behind them)

bool shape_ok(int N, int Npix) { return N >= 0 && Npix >= 1 && Npix <= kMaxNpix; }

}  // namespace

extern "C" {

size_t qfa_absorber_workspace_bytes(int N, int Npix) { return shape_ok(N, Npix) ? 16 : 0; }

int qfa_absorber_mask_f32(const float *flux, const float *error, const double *zqso, const double *wav_grid, int N, int Npix,
                          const int64_t *abs_offsets, const double *abs_z, const double *abs_lognhi,
                          const double *obs_intervals, int n_obs, const int64_t *rest_offsets, const double *rest_intervals,
                          const qfa_absorber_t *q, float *flux_out, float *error_out, float *trans_out, double *record_f64,
                          int32_t *record_i32, void *workspace, size_t workspace_bytes, void *stream) {
    if (!q) return QFA_E_NULL;
    if (!shape_ok(N, Npix) || n_obs < 0) return QFA_E_SIZE;
    if (!(q->t_min >= 0.0 && q->t_min < 1.0) || !(q->b_kms > 0.0 && isfinite(q->b_kms)) ||
        !(isfinite(q->snr_lo) && isfinite(q->snr_hi) && q->snr_lo < q->snr_hi))
        return QFA_E_SIZE;
    if (q->flags & ~(unsigned)(QFA_ABS_LYB | QFA_ABS_CORRECT)) return QFA_E_FLAGS;
    if (N == 0) return 0;
    if (!flux || !error || !zqso || !wav_grid || !flux_out || !error_out || !record_f64 || !record_i32 || !workspace)
        return QFA_E_NULL;
    if ((abs_offsets && (!abs_z || !abs_lognhi)) || (n_obs > 0 && !obs_intervals) || (rest_offsets && !rest_intervals))
        return QFA_E_NULL;
    if (workspace_bytes < 16) return QFA_E_WORKSPACE;
    Args a;
    a.flux = flux; a.error = error; a.zqso = zqso; a.grid = wav_grid;
    a.abs_off = abs_offsets; a.abs_z = abs_z; a.abs_lognhi = abs_lognhi;
    a.obs = obs_intervals; a.rest_off = rest_offsets; a.rest = rest_intervals;
    a.flux_out = flux_out; a.error_out = error_out; a.trans_out = trans_out;
    a.rec_f64 = record_f64; a.rec_i32 = record_i32;
    a.N = N; a.Npix = Npix; a.n_obs = n_obs;
    a.lyb = (q->flags & QFA_ABS_LYB) ? 1 : 0; a.correct = (q->flags & QFA_ABS_CORRECT) ? 1 : 0;
    a.t_min = q->t_min; a.b_kms = q->b_kms; a.snr_lo = q->snr_lo; a.snr_hi = q->snr_hi;
    const unsigned grid = (unsigned)((int64_t)N < kGrid ? (int64_t)N : kGrid);
    k_absorber<<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // extern "C"
