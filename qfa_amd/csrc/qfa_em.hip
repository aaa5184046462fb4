// qfa_em.hip -- C-ABI of the closed-form EM update of the factor loadings (include/qfa_hip.h: qfa_em_floats,
// qfa_em_workspace_bytes, qfa_em_stats_f32, qfa_em_update_f_f32): argument checks, workspace layout, launch geometry.
// Kernels in qfa_em.h; the E-step (images, pass 1, solve) is the training step's own, run through qfa_estep.h.
#include "qfa_em.h"
#include "qfa_estep.h"

namespace {

using namespace qfa_em;

// workspace = [the step's workspace | REC B x ncp | SLAB R x Npix x ncp | CNT R x Npix]; the batch is cut into R ranges of `per`
// spectra (a multiple of four: one MFMA step).  A function of the shape alone: the same call sums in the same order.
struct EmPlan {
    int R, per, ncp;
    size_t oREC, oSLAB, oCNT, total;     // bytes
};

constexpr int kTargetBlocks = 1024;                 // four workgroups of 256 threads per CU of a 256-CU device
constexpr size_t kSlabBudget = (size_t)256 << 20;   // bytes of slab rows at most (one range always fits)

EmPlan em_plan(int B, int Npix, int Nh) {
    EmPlan P;
    P.ncp = rec_cols(Nh);
    const int nblk = (Npix + 63) / 64;
    long long R = (kTargetBlocks + nblk - 1) / nblk;
    const long long by_batch = ((long long)B + 255) / 256;                         // ranges of at least 256 spectra
    if (R > by_batch) R = by_batch;
    const long long by_mem = (long long)(kSlabBudget / ((size_t)Npix * P.ncp * sizeof(float)));
    if (R > by_mem) R = by_mem;
    if (R < 1) R = 1;
    long long per = ((long long)B + R - 1) / R;
    per = (per + 3) / 4 * 4;
    P.per = (int)per;
    P.R = (int)(((long long)B + per - 1) / per);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    P.oREC = up(qfa_workspace_bytes(B, Npix, Nh));
    P.oSLAB = P.oREC + up((size_t)B * P.ncp * sizeof(float));
    P.oCNT = P.oSLAB + up((size_t)P.R * Npix * P.ncp * sizeof(float));
    P.total = P.oCNT + up((size_t)P.R * Npix * sizeof(float));
    return P;
}

bool shape_ok(int Npix, int Nh) { return Npix >= 1 && Nh >= 1 && Nh <= 32 && (long long)64 * Npix < (1LL << 31); }

template <int NT>
void launch_stats(const BatchCall &c, const QfaEStep &es, const EmPlan &P, int t0, const float *REC, float *SLAB, float *CNT) {
    const dim3 grid((unsigned)((c.Npix + 63) / 64), (unsigned)P.R);
    by_form(c.b, es.ZS != nullptr, false, [&](auto f) {
        using Fm = decltype(f);
        k_em_stats<NT, Fm::zf, Fm::hasa><<<grid, 256, 0, c.st>>>(c.p, c.b, c.tau, c.B, c.Npix, c.Nb, c.Nh, P.per, t0, es.ZS, es.ZP, REC, SLAB, CNT);
    });
}

}  // namespace

extern "C" {

size_t qfa_em_floats(int Npix, int Nh) {
    if (!shape_ok(Npix, Nh)) return 0;
    return (size_t)Npix * ((size_t)Nh * Nh + Nh + 1) + 4;
}

size_t qfa_em_workspace_bytes(int B, int Npix, int Nh) {
    if (B < 1 || B > (1 << 24) || !shape_ok(Npix, Nh)) return 0;
    return em_plan(B, Npix, Nh).total;
}

int qfa_em_stats_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh,
                     float *stats, float *nll, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (!stats || !ws) return QFA_E_NULL;
    if (int e = qfa_estep_check(p, b, tau, B, Npix, Nb, Nh)) return e;
    if (flags & ~(QFA_F_ZERO_ACCUM | QFA_F_SYNC)) return QFA_E_FLAGS;
    const EmPlan P = em_plan(B, Npix, Nh);
    if (ws_bytes < P.total) return QFA_E_WORKSPACE;
    const BatchCall c{*p, norm_batch(*b, Npix), *tau, B, Npix, Nb, Nh, (float *)ws, (hipStream_t)stream, flags};
    hipStream_t st = c.st;
    char *base = (char *)ws;
    float *REC = (float *)(base + P.oREC), *SLAB = (float *)(base + P.oSLAB), *CNT = (float *)(base + P.oCNT);
    QfaEStep es{};
    if (int e = qfa_estep(c, nll, &es)) return e;
    const size_t nrec = (size_t)B * P.ncp;
    k_em_record<<<(unsigned)((nrec + 255) / 256), 256, 0, st>>>(es.SOL, es.nsol, es.KP, es.sol_ci, B, Nh, REC);
    const int ntl = P.ncp / 16;
    if (ntl <= 2) launch_stats<2>(c, es, P, 0, REC, SLAB, CNT);
    else if (ntl <= 4) launch_stats<4>(c, es, P, 0, REC, SLAB, CNT);
    else
        for (int t0 = 0; t0 < ntl; t0 += 10) launch_stats<10>(c, es, P, t0, REC, SLAB, CNT);
    const int zero = (flags & QFA_F_ZERO_ACCUM) ? 1 : 0;
    const size_t n = (size_t)Npix * ((size_t)Nh * Nh + Nh + 1);
    k_em_reduce<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(SLAB, CNT, P.R, Npix, Nh, zero, stats);
    k_em_nll<<<1, 1024, 0, st>>>(es.nll, B, zero, stats + n);
    return hip_status(st, flags);
}

int qfa_em_update_f_f32(const float *stats, const float *F, int Npix, int Nh, double ridge, double damping, float *F_out,
                        unsigned *n_skipped, void *stream) {
    if (!stats || !F || !F_out) return QFA_E_NULL;
    if (!shape_ok(Npix, Nh) || !(ridge >= 0.0) || !(damping == damping)) return QFA_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    if (n_skipped) (void)hipMemsetAsync(n_skipped, 0, sizeof(unsigned), st);
    k_em_solve_f<<<(unsigned)((Npix + 3) / 4), 256, 0, st>>>(stats, F, Npix, Nh, ridge, damping, F_out, n_skipped);
    return (int)hipGetLastError();
}

}  // extern "C"
