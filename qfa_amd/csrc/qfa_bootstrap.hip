// qfa_bootstrap.hip -- C-ABI of the sightline bootstrap of the per-segment rows (include/qfa_hip.h: qfa_bootstrap_workspace_bytes,
// qfa_bootstrap_f64): argument checks and the launch.  Kernels in qfa_bootstrap.h; qfa_segment_codes_f32 lives in qfa_p1d.hip, beside
// the checks of qfa_p1d_f32 it shares.
#include "qfa_bootstrap.h"
#include "qfa_call.h"

namespace {

using namespace qfa_bootstrap;

constexpr int kMaxWidth = 4096;                 // W and nz: the forest's limits
constexpr int kMaxReplicates = 65536;           // grid.y = R / 256; the quad index keeps far below bit 30 of the counter word
constexpr size_t kWorkspace = 16;               // nothing is held between kernels: a token size, so that 0 keeps meaning "unsupported"

bool shape_ok(int64_t B, int S, int nseg, int W, int nz, int R) {
    if (B < 0 || S < 1 || nseg < 1 || W < 1 || W > kMaxWidth || nz < 1 || nz > kMaxWidth || R < 1 || R > kMaxReplicates) return false;
    if (B * S * nseg > INT32_MAX) return false;                                   // the segment index of a draw is an int
    return (int64_t)S * nz * ((W + 1 + kCols - 1) / kCols) <= INT32_MAX;          // grid.x
}

template <typename T>
void launch(const void *rows, const int *codes, int B, int S, int nseg, int W, int nz, int R, uint64_t seed, int64_t row0, int zero,
            double *boot, hipStream_t st) {
    Args<T> a;
    a.rows = (const T *)rows;
    a.codes = codes;
    a.boot = boot;
    a.n = B * nseg;
    a.S = S; a.nseg = nseg; a.W = W; a.nz = nz; a.R = R; a.zero = zero;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.row0 = row0;
    const unsigned gx = (unsigned)((size_t)S * nz * ((W + 1 + kCols - 1) / kCols));
    const unsigned gy = (unsigned)((R + 4 * kQuadsPerBlock - 1) / (4 * kQuadsPerBlock));
    k_bootstrap<T><<<dim3(gx, gy), kThreads, 0, st>>>(a);
}

}  // namespace

extern "C" {

size_t qfa_bootstrap_workspace_bytes(int n_spectra, int S, int nseg, int W, int nz, int R) {
    return shape_ok(n_spectra, S, nseg, W, nz, R) ? kWorkspace : 0;
}

int qfa_bootstrap_f64(const void *rows, int row_type, const int32_t *codes, int B, int S, int nseg, int W, int nz, int R, uint64_t seed,
                      int64_t row_offset, unsigned flags, double *boot, void *ws, size_t ws_bytes, void *stream) {
    if (!boot || !ws) return QFA_E_NULL;
    if (!shape_ok(B, S, nseg, W, nz, R) || row_offset < 0 || row_offset > INT64_MAX - B) return QFA_E_SIZE;
    if (row_type != QFA_ROW_F32 && row_type != QFA_ROW_F64 && row_type != QFA_ROW_I32) return QFA_E_SIZE;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    if (ws_bytes < kWorkspace) return QFA_E_WORKSPACE;
    if (B > 0 && (!rows || !codes)) return QFA_E_NULL;                           // (an empty tensor has a NULL pointer)
    hipStream_t st = (hipStream_t)stream;
    const int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    if (B == 0)
        return zero ? (int)hipMemsetAsync(boot, 0, (size_t)S * R * nz * (size_t)(W + 1) * sizeof(double), st) : 0;
    if (row_type == QFA_ROW_F32) launch<float>(rows, codes, B, S, nseg, W, nz, R, seed, row_offset, zero, boot, st);
    else if (row_type == QFA_ROW_F64) launch<double>(rows, codes, B, S, nseg, W, nz, R, seed, row_offset, zero, boot, st);
    else launch<int32_t>(rows, codes, B, S, nseg, W, nz, R, seed, row_offset, zero, boot, st);
    return hip_status(st, flags);
}

}  // extern "C"
