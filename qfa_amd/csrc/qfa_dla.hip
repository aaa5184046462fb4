// qfa_dla.hip -- C-ABI of the DLA finder (include/qfa_hip.h: qfa_dla_profiles_f32, qfa_template_scan_workspace_bytes,
// qfa_template_scan_f32): argument checks, workspace layout, launch geometry.  Kernels in qfa_dla.h.
#include "qfa_dla.h"
#include "qfa_estep.h"

#include <math.h>

namespace {

using namespace qfa_dla;

constexpr int kMaxNz = 4096, kMaxNn = 64;
constexpr size_t kChunkBudget = (size_t)256 << 20;   // bytes of per-spectrum rows (records and moments) of one chunk, at least four spectra

// workspace = [PF Npad x pc | VT Npad x ncp | FLAG nct x Npad / 16 | per chunk of Bc spectra: REC | NULLM | NUL0 | MOM].  The batch is
// walked in chunks of Bc spectra; a spectrum's row is computed from its own records, so the cut changes no bit.
struct ScanPlan {
    int Npad, ncp, pc, Bc;
    size_t oPF, oVT, oFLAG, oREC, oNULLM, oNUL0, oMOM, total;     // bytes
};

bool shape_ok(int B, int Npix, int Nh, int nc) {
    return B >= 1 && B <= (1 << 24) && Npix >= 1 && (long long)64 * Npix < (1LL << 31) && Nh >= 1 && Nh <= 32 && nc >= 1 &&
           nc <= kMaxNz * kMaxNn;
}

ScanPlan scan_plan(int B, int Npix, int Nh, int nc) {
    ScanPlan P;
    P.Npad = round_up(Npix, 16);
    P.ncp = round_up(nc, 16);
    P.pc = pf_cols(Nh);
    const size_t rec = (size_t)R_ROWS * P.Npad * sizeof(float), mom = (size_t)P.ncp * mom_cols(Nh) * sizeof(float);
    const size_t nul = (size_t)null_cols(Nh) * sizeof(double);
    size_t bc = kChunkBudget / (rec + mom + nul + 16);
    bc = bc / 4 * 4;
    if (bc < 4) bc = 4;
    if (bc > (size_t)B) bc = (size_t)B;
    P.Bc = (int)bc;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    P.oPF = 0;
    P.oVT = P.oPF + up((size_t)P.Npad * P.pc * sizeof(float));
    P.oFLAG = P.oVT + up((size_t)P.Npad * P.ncp * sizeof(float));
    P.oREC = P.oFLAG + up((size_t)(P.ncp / 16) * (P.Npad / 16));
    P.oNULLM = P.oREC + up(bc * rec);
    P.oNUL0 = P.oNULLM + up(bc * nul);
    P.oMOM = P.oNUL0 + up(bc * 2 * sizeof(double));
    P.total = P.oMOM + up(bc * mom);
    return P;
}

template <int NTL>
void launch_scan(const ScanPlan &P, int nspec, int Nh, const float *REC, const float *PF, const float *VT, const unsigned char *FLAG,
                 float *MOM, hipStream_t st) {
    const dim3 grid((unsigned)(P.ncp / 16), (unsigned)((nspec + 3) / 4));
    k_template_scan<NTL><<<grid, 256, 0, st>>>(REC, PF, VT, FLAG, nspec, P.Npad, Nh, P.ncp, MOM);
}

}  // namespace

extern "C" {

int qfa_dla_profiles_f32(const double *wav_grid, int Npix, double lam_hi, double dv_kms, int nz, double logn_lo, double dlogn, int nN,
                         double b_kms, int lyb, float *V_out, void *stream) {
    if (!wav_grid || !V_out) return QFA_E_NULL;
    if (Npix < 1 || nz < 1 || nz > kMaxNz || nN < 1 || nN > kMaxNn || (long long)64 * Npix >= (1LL << 31)) return QFA_E_SIZE;
    if (!(lam_hi > 0.0 && isfinite(lam_hi)) || !(dv_kms >= 0.0 && isfinite(dv_kms)) || !isfinite(logn_lo) || !isfinite(dlogn) ||
        !(b_kms > 0.0 && isfinite(b_kms)))
        return QFA_E_SIZE;
    hipStream_t st = (hipStream_t)stream;
    double ends[2];                                              // the one read of the grid on the host (this call synchronises `stream`)
    hipError_t e = hipMemcpyAsync(&ends[0], wav_grid, sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], wav_grid + (Npix - 1), sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    const double lam_lo = lam_hi * exp(-(double)(nz - 1) * dv_kms / qfa_voigt::kC);
    if (!(ends[0] <= lam_lo && lam_hi <= ends[1])) return QFA_E_SIZE;
    const size_t n = (size_t)nz * nN * Npix;
    k_dla_profiles<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(wav_grid, Npix, lam_hi, dv_kms, nz, logn_lo, dlogn, nN, b_kms, lyb ? 1 : 0,
                                                                V_out);
    return (int)hipGetLastError();
}

size_t qfa_template_scan_workspace_bytes(int B, int Npix, int Nh, int nc) {
    return shape_ok(B, Npix, Nh, nc) ? scan_plan(B, Npix, Nh, nc).total : 0;
}

int qfa_template_scan_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *V, int nc,
                          int B, int Npix, int Nb, int Nh, float *llr, float *nll0, int32_t *best_c, float *best_llr, void *ws,
                          size_t ws_bytes, unsigned flags, void *stream) {
    if (!mu || !V || !llr || !nll0 || !ws) return QFA_E_NULL;
    if (int e = qfa_estep_check(p, b, tau, B, Npix, Nb, Nh)) return e;
    if (b->A_blue) return QFA_E_NULL;                            // a custom tau callable has no in-kernel form here
    if (!shape_ok(B, Npix, Nh, nc)) return QFA_E_SIZE;
    if (flags & ~QFA_F_SYNC) return QFA_E_FLAGS;
    const ScanPlan P = scan_plan(B, Npix, Nh, nc);
    if (ws_bytes < P.total) return QFA_E_WORKSPACE;
    const qfa_batch_t bt = norm_batch(*b, Npix);
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    float *PF = (float *)(base + P.oPF), *VT = (float *)(base + P.oVT), *REC = (float *)(base + P.oREC), *MOM = (float *)(base + P.oMOM);
    unsigned char *FLAG = (unsigned char *)(base + P.oFLAG);
    double *NULLM = (double *)(base + P.oNULLM), *NUL0 = (double *)(base + P.oNUL0);
    auto blocks = [](size_t n) { return (unsigned)((n + 255) / 256); };
    k_scan_pf<<<blocks((size_t)P.Npad * P.pc), 256, 0, st>>>(p->F, Npix, P.Npad, Nh, PF);
    k_scan_vt<<<blocks((size_t)P.Npad * P.ncp), 256, 0, st>>>(V, nc, P.ncp, Npix, P.Npad, VT);
    k_scan_flags<<<blocks((size_t)(P.ncp / 16) * (P.Npad / 16)), 256, 0, st>>>(VT, P.ncp, P.Npad, FLAG);
    const int ntl = P.pc / 16;
    for (int s0 = 0; s0 < B; s0 += P.Bc) {
        const int ns = B - s0 < P.Bc ? B - s0 : P.Bc;
        k_scan_prep<<<blocks((size_t)ns * P.Npad), 256, 0, st>>>(*p, bt, *tau, mu, s0, ns, Npix, P.Npad, Nb, REC);
        k_scan_null<<<(unsigned)ns, 256, 0, st>>>(REC, PF, P.Npad, Nh, NULLM);
        k_scan_solve<<<(unsigned)((ns + 3) / 4), 256, 0, st>>>(MOM, NULLM, NUL0, ns, nc, P.ncp, Nh, 1, nll0 + s0);
        if (ntl <= 2) launch_scan<2>(P, ns, Nh, REC, PF, VT, FLAG, MOM, st);
        else if (ntl <= 4) launch_scan<4>(P, ns, Nh, REC, PF, VT, FLAG, MOM, st);
        else if (ntl <= 10) launch_scan<10>(P, ns, Nh, REC, PF, VT, FLAG, MOM, st);
        else launch_scan<35>(P, ns, Nh, REC, PF, VT, FLAG, MOM, st);
        k_scan_solve<<<(unsigned)(((size_t)ns * nc + 3) / 4), 256, 0, st>>>(MOM, NULLM, NUL0, ns, nc, P.ncp, Nh, 0, llr + (size_t)s0 * nc);
    }
    if (best_c || best_llr) k_scan_best<<<(unsigned)B, 256, 0, st>>>(llr, nc, best_c, best_llr);
    return hip_status(st, flags);
}

}  // extern "C"
