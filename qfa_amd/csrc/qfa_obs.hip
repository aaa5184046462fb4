// qfa_obs.hip -- C-ABI of the observed-frame residual stack and of the calibration (include/qfa_hip.h: qfa_obs_stack_doubles,
// qfa_obs_stack_workspace_bytes, qfa_obs_stack_f32, qfa_calibrate_f32): argument checks, the launch plan and the launches.
// Kernels in qfa_obs.h.
#include "qfa_obs.h"
#include "qfa_call.h"

#include <math.h>

namespace {

using namespace qfa_obs;

constexpr int kMaxBins = 32768;
constexpr int64_t kBlocks = 2048;             // blocks of a large call (eight per CU)
constexpr int64_t kMaxChunks = 64;            // rows of partial sums the reducer adds per entry, at the most
constexpr size_t kRowBytes = (size_t)256 << 20;   // bytes of rows the plan aims at (one row, whatever its size, always fits)
constexpr int64_t kCalGrid = 2048;

// How a call is cut: a block owns (tile of kThreads bins, group of `sc` draws, chunk of `rpc` spectra); workspace = `chunks` rows of
// S 4 nbin doubles from its first 16-byte boundary on.  A function of the shape alone, so that two calls on one shape add in one order.
struct Plan {
    int tiles, sc, sgroups, rpc;
    int64_t chunks;
    size_t nent, bytes;
};

bool shape_ok(int B, int S, int Npix, int Nh, int nbin) {
    return B >= 0 && S >= 1 && Npix >= 1 && Nh >= 1 && Nh <= 32 && nbin >= 1 && nbin <= kMaxBins &&
           (int64_t)S * 4 * nbin <= ((int64_t)1 << 40);
}

Plan make_plan(int B, int S, int nbin) {
    Plan P;
    P.tiles = (nbin + kThreads - 1) / kThreads;
    P.sc = S == 1 ? 1 : kDraws;
    P.sgroups = (S + P.sc - 1) / P.sc;
    P.nent = (size_t)S * 4 * nbin;
    const int64_t per = (int64_t)P.tiles * P.sgroups;
    int64_t want = (kBlocks + per - 1) / per;
    const int64_t fit = (int64_t)(kRowBytes / (P.nent * sizeof(double)));
    if (want > fit) want = fit;
    if (want > kMaxChunks) want = kMaxChunks;
    if (want < 1) want = 1;
    const int64_t Bn = B > 0 ? B : 1;
    if (want > Bn) want = Bn;
    P.rpc = (int)((Bn + want - 1) / want);
    P.chunks = (Bn + P.rpc - 1) / P.rpc;
    P.bytes = 16 + (size_t)P.chunks * P.nent * sizeof(double);
    return P;
}

template <int NHM>
void launch(const Args &a, const Plan &P, hipStream_t st) {
    const unsigned grid = (unsigned)(P.chunks * P.sgroups * P.tiles);
    if (P.sc == 1) k_obs_stack<NHM, 1><<<grid, kThreads, 0, st>>>(a);
    else k_obs_stack<NHM, kDraws><<<grid, kThreads, 0, st>>>(a);
}

}  // namespace

extern "C" {

size_t qfa_obs_stack_doubles(int S, int nbin) {
    if (S < 1 || nbin < 1 || nbin > kMaxBins || (int64_t)S * 4 * nbin > ((int64_t)1 << 40)) return 0;
    return (size_t)S * 4 * nbin;
}

size_t qfa_obs_stack_workspace_bytes(int B, int S, int Npix, int Nh, int nbin) {
    if (!shape_ok(B, S, Npix, Nh, nbin)) return 0;
    return make_plan(B, S, nbin).bytes;
}

int qfa_obs_stack_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, const float *unc, const double *pix_u,
                      const double *spec_u, int B, int S, int Npix, int Nh, const qfa_obs_bins_t *bins, float cont_min,
                      unsigned flags, double *stack, void *workspace, size_t workspace_bytes, void *stream) {
    if (!F || !mu || !b || !h || !pix_u || !spec_u || !bins || !workspace || !stack) return QFA_E_NULL;
    if (!b->delta || !b->error) return QFA_E_NULL;
    if (B < 0 || S < 1 || Npix < 1 || Nh < 1 || Nh > 32) return QFA_E_SIZE;
    if (!(bins->du > 0.0) || !isfinite(bins->du) || !isfinite(bins->u0) || !isfinite(1.0 / bins->du) || bins->nbin < 1 ||
        bins->nbin > kMaxBins || bins->p_lo < 0 || bins->p_lo > bins->p_hi || bins->p_hi > Npix ||
        (bins->mode != QFA_OBS_LOG && bins->mode != QFA_OBS_LINEAR))
        return QFA_E_SIZE;
    if (!shape_ok(B, S, Npix, Nh, bins->nbin)) return QFA_E_SIZE;
    if (b->row_stride != 0 && b->row_stride < (int64_t)Npix) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC | QFA_F_OBS_UNIT_W)) return QFA_E_FLAGS;
    const int nbin = bins->nbin;
    const Plan P = make_plan(B, S, nbin);
    if (workspace_bytes < P.bytes) return QFA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0 || bins->p_lo == bins->p_hi) {
        if (zero) {
            hipError_t e = hipMemsetAsync(stack, 0, P.nent * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    Args a;
    a.bt = norm_batch(*b, Npix);
    a.F = F; a.mu = mu; a.h = h; a.unc = unc; a.pix_u = pix_u; a.spec_u = spec_u;
    a.rows = (double *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    a.u0 = bins->u0;
    a.inv_du = 1.0 / bins->du;
    a.B = B; a.S = S; a.Npix = Npix; a.Nh = Nh; a.nbin = nbin; a.p_lo = bins->p_lo; a.p_hi = bins->p_hi;
    a.tiles = P.tiles; a.sgroups = P.sgroups; a.rpc = P.rpc;
    a.linear = bins->mode == QFA_OBS_LINEAR ? 1 : 0;
    a.unit_w = (flags & QFA_F_OBS_UNIT_W) ? 1 : 0;
    a.cont_min = cont_min;
    by_nhm(Nh, [&](auto nhm) { launch<decltype(nhm)::value>(a, P, st); });
    k_obs_reduce<<<(unsigned)((P.nent + 255) / 256), 256, 0, st>>>(a.rows, (int)P.chunks, P.nent, zero, stack);
    return hip_status(st, flags);
}

int qfa_calibrate_f32(const float *flux, const float *error, const double *pix_u, const double *spec_u, int N, int Npix,
                      const double *cal, int ncal, double u0, double du, unsigned mode, double c_min, float *flux_out,
                      float *error_out, int32_t *n_uncal, void *stream) {
    if (N < 0 || Npix < 1 || ncal < 2) return QFA_E_SIZE;
    if (!(du > 0.0) || !isfinite(du) || !isfinite(u0) || !isfinite(1.0 / du) || !(c_min > 0.0) || !isfinite(c_min) ||
        (mode != QFA_OBS_LOG && mode != QFA_OBS_LINEAR))
        return QFA_E_SIZE;
    if (N == 0) return 0;
    if (!flux || !error || !pix_u || !spec_u || !cal || !flux_out || !error_out || !n_uncal) return QFA_E_NULL;
    CalArgs a;
    a.flux = flux; a.error = error; a.pix_u = pix_u; a.spec_u = spec_u; a.cal = cal;
    a.flux_out = flux_out; a.error_out = error_out; a.n_uncal = n_uncal;
    a.u0 = u0; a.inv_du = 1.0 / du; a.c_min = c_min;
    a.N = N; a.Npix = Npix; a.ncal = ncal; a.linear = mode == QFA_OBS_LINEAR ? 1 : 0;
    const unsigned grid = (unsigned)((int64_t)N < kCalGrid ? (int64_t)N : kCalGrid);
    k_calibrate<<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // extern "C"
