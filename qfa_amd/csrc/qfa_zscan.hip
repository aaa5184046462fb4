// qfa_zscan.hip -- C-ABI of the quasar-redshift finder (include/qfa_hip.h: qfa_zscan_workspace_bytes, qfa_redshift_scan_f32):
// argument checks, workspace layout, launch geometry.  Kernels in qfa_zscan.h.
#include "qfa_zscan.h"
#include "qfa_estep.h"

namespace {

using namespace qfa_zscan;

constexpr int kMaxShift = 4096;
constexpr size_t kChunkBudget = (size_t)64 << 20;   // bytes of per-spectrum rows (records, moments, scalars, NLLs) of one chunk
constexpr size_t kLdsRecords = (size_t)64 << 10;    // a spectrum's records stay in LDS up to this size

// workspace = [PF Npad x pc | MQ Npad | per chunk of Bc spectra: REC | MOM | SC | NLL].  The batch is walked in chunks of Bc spectra; a
// spectrum's row is computed from its own records, so the cut changes no bit.
struct ZPlan {
    int Npad, RL, nc, nct, ncp, pc, Bc;
    size_t oPF, oMQ, oREC, oMOM, oSC, oNLL, total;                // bytes
};

bool shape_ok(int B, int Npix, int Nh, int m) {
    return B >= 1 && B <= (1 << 24) && Npix >= 1 && (long long)64 * Npix < (1LL << 31) && Nh >= 1 && Nh <= 32 && m >= 0 &&
           m <= kMaxShift && (long long)2 * m + 1 <= Npix;
}

ZPlan zscan_plan(int B, int Npix, int Nh, int m) {
    ZPlan P;
    P.Npad = round_up(Npix, 16);
    P.RL = P.Npad + 2 * m;
    P.nc = 2 * m + 1;
    P.nct = (P.nc + 15) / 16;
    P.ncp = 16 * P.nct;
    P.pc = pf_cols(Nh);
    const size_t rec = (size_t)P.RL * sizeof(float4), mom = (size_t)P.ncp * P.pc * sizeof(double);
    const size_t sc = (size_t)P.ncp * SC_COLS * sizeof(double), nll = (size_t)P.nc * sizeof(double);
    size_t bc = kChunkBudget / (rec + mom + sc + nll);
    if (bc < 4) bc = 4;
    if (bc > (size_t)B) bc = (size_t)B;
    P.Bc = (int)bc;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    P.oPF = 0;
    P.oMQ = P.oPF + up((size_t)P.Npad * P.pc * sizeof(float));
    P.oREC = P.oMQ + up((size_t)P.Npad * sizeof(float4));
    P.oMOM = P.oREC + up(bc * rec);
    P.oSC = P.oMOM + up(bc * mom);
    P.oNLL = P.oSC + up(bc * sc);
    P.total = P.oNLL + up(bc * nll);
    return P;
}

template <int NTL>
void launch_zscan(const ZPlan &P, int nspec, int Nh, int m, const float4 *REC, const float *PF, const float4 *MQ, double *MOM, double *SC,
                  hipStream_t st) {
    const size_t lds = (size_t)P.RL * sizeof(float4);
    if (lds <= kLdsRecords) k_zscan<NTL, true><<<(unsigned)nspec, 256, lds, st>>>(REC, PF, MQ, P.Npad, P.RL, Nh, m, P.nct, MOM, SC);
    else k_zscan<NTL, false><<<(unsigned)nspec, 256, 0, st>>>(REC, PF, MQ, P.Npad, P.RL, Nh, m, P.nct, MOM, SC);
}

}  // namespace

extern "C" {

size_t qfa_zscan_workspace_bytes(int B, int Npix, int Nh, int max_shift) {
    return shape_ok(B, Npix, Nh, max_shift) ? zscan_plan(B, Npix, Nh, max_shift).total : 0;
}

int qfa_redshift_scan_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *pix_ratio_full,
                          int max_shift, int B, int Npix, int Nb, int Nh, float *llr, float *nll0, int32_t *best_s, float *best_llr,
                          double *off, double *sig, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (!mu || !pix_ratio_full || !llr || !nll0 || !ws) return QFA_E_NULL;
    if (int e = qfa_estep_check(p, b, tau, B, Npix, Nb, Nh)) return e;
    if (b->A_blue) return QFA_E_NULL;                            // a custom tau callable has no in-kernel form here
    if (Nb > 0 && !b->zq1) return QFA_E_NULL;                    // z at data pixels beyond Nb: the factored form only
    const int m = max_shift;
    if (!shape_ok(B, Npix, Nh, m)) return QFA_E_SIZE;
    if (flags & ~QFA_F_SYNC) return QFA_E_FLAGS;
    const ZPlan P = zscan_plan(B, Npix, Nh, m);
    if (ws_bytes < P.total) return QFA_E_WORKSPACE;
    const qfa_batch_t bt = norm_batch(*b, Npix);
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    float *PF = (float *)(base + P.oPF);
    float4 *MQ = (float4 *)(base + P.oMQ), *REC = (float4 *)(base + P.oREC);
    double *MOM = (double *)(base + P.oMOM), *SC = (double *)(base + P.oSC), *NLL = (double *)(base + P.oNLL);
    auto blocks = [](size_t n) { return (unsigned)((n + 255) / 256); };
    qfa_dla::k_scan_pf<<<blocks((size_t)P.Npad * P.pc), 256, 0, st>>>(p->F, Npix, P.Npad, Nh, PF);
    k_zscan_model<<<blocks((size_t)P.Npad), 256, 0, st>>>(*p, mu, Npix, P.Npad, Nb, MQ);
    const int ntl = P.pc / 16;
    for (int s0 = 0; s0 < B; s0 += P.Bc) {
        const int ns = B - s0 < P.Bc ? B - s0 : P.Bc;
        k_zscan_prep<<<blocks((size_t)ns * P.RL), 256, 0, st>>>(*p, bt, *tau, pix_ratio_full, s0, ns, Npix, P.RL, Nb, m, REC);
        if (ntl <= 2) launch_zscan<2>(P, ns, Nh, m, REC, PF, MQ, MOM, SC, st);
        else if (ntl <= 4) launch_zscan<4>(P, ns, Nh, m, REC, PF, MQ, MOM, SC, st);
        else if (ntl <= 10) launch_zscan<10>(P, ns, Nh, m, REC, PF, MQ, MOM, SC, st);
        else launch_zscan<18>(P, ns, Nh, m, REC, PF, MQ, MOM, SC, st);
        k_zscan_close<<<(unsigned)(((size_t)ns * P.nc + 3) / 4), 256, 0, st>>>(MOM, SC, ns, P.nc, P.ncp, Nh, NLL);
        k_zscan_best<<<(unsigned)ns, 64, 0, st>>>(NLL, P.nc, m, llr + (size_t)s0 * P.nc, nll0 + s0, best_s ? best_s + s0 : nullptr,
                                                  best_llr ? best_llr + s0 : nullptr, off ? off + s0 : nullptr, sig ? sig + s0 : nullptr);
    }
    return hip_status(st, flags);
}

}  // extern "C"
