// qfa_sample.hip -- C-ABI of the draws from the model (include/qfa_hip.h: qfa_sample_latent_f32, qfa_continua_workspace_bytes,
// qfa_continua_f32, qfa_mock_workspace_bytes, qfa_mock_spectra_f32): argument checks and launch geometry.  Kernels in qfa_sample.h.
#include "qfa_sample.h"
#include "qfa_call.h"

namespace {

using namespace qfa_sample;

int pad_of(int Npix) { return (Npix + kWriterThreads - 1) / kWriterThreads * kWriterThreads; }

template <int NH>
void launch_cont(const float *img, int pad, const float *h, int64_t R, int Npix, float *out, hipStream_t st) {
    const int strips = pad / kWriterThreads;
    // about 32 blocks per CU-sized slice of 256 CUs; at least 16 rows per block so that the image loads are amortised,
    // at most 256 so that the grid still spreads a large call over every CU
    int64_t rpb = (R * strips + 8191) / 8192;
    rpb = rpb < 16 ? 16 : (rpb > 256 ? 256 : rpb);
    const int64_t cap = (R * strips + 0x3fffffff) / 0x40000000;      // grid.x stays below 2^30 blocks
    if (rpb < cap) rpb = cap;
    const int64_t chunks = (R + rpb - 1) / rpb;
    k_sample_cont<NH><<<(unsigned)(chunks * strips), kWriterThreads, 0, st>>>(img, pad, h, R, Npix, strips, rpb, out);
}

template <int NH>
void dispatch_cont(int Nh, const float *img, int pad, const float *h, int64_t R, int Npix, float *out, hipStream_t st) {
    if constexpr (NH > 1) {
        if (Nh < NH) return dispatch_cont<NH - 1>(Nh, img, pad, h, R, Npix, out, st);
    }
    launch_cont<NH>(img, pad, h, R, Npix, out, st);
}

// mock spectra: the workspace holds [image (Nh + 3) rows of `pad` floats | ZP `pad` float4], from its first 16-byte boundary on
int mock_pad_of(int Npix) { return (Npix + kMockStrip - 1) / kMockStrip * kMockStrip; }

}  // namespace

extern "C" {

size_t qfa_continua_workspace_bytes(int Npix, int Nh) {
    if (Npix < 1 || Nh < 1 || Nh > 32) return 0;
    return (size_t)(Nh + 1) * pad_of(Npix) * sizeof(float);
}

int qfa_sample_latent_f32(const float *hmean, const float *hcov, int B, int Nh, int S, uint64_t seed, int64_t row0,
                          float *h, void *stream) {
    if (!hmean || !hcov || !h) return QFA_E_NULL;
    if (B < 0 || S < 1 || Nh < 1 || Nh > 32 || row0 < 0 || row0 > INT64_MAX - B) return QFA_E_SIZE;
    if (B == 0) return 0;
    // at most 65535 chunks along grid y: 256 samples per wave (four per lane) or more when S is larger than 16.7 M
    int spb = 4 * kLatentThreads;
    const int64_t need = ((int64_t)S + 65534) / 65535;
    if (need > spb) spb = (int)((need + kLatentThreads - 1) / kLatentThreads * kLatentThreads);
    const dim3 grid((unsigned)B, (unsigned)((S + (int64_t)spb - 1) / spb));
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipStream_t st = (hipStream_t)stream;
    by_nhm(Nh, [&](auto nhm) {
        k_sample_latent<decltype(nhm)::value><<<grid, kLatentThreads, 0, st>>>(hmean, hcov, Nh, S, spb, k0, k1, row0, h);
    });
    return (int)hipGetLastError();
}

int qfa_continua_f32(const float *F, const float *mu, const float *h, int64_t R, int Npix, int Nh, float *out,
                     void *workspace, size_t workspace_bytes, void *stream) {
    if (!F || !mu || !h || !out || !workspace) return QFA_E_NULL;
    if (R < 0 || Npix < 1 || Nh < 1 || Nh > 32) return QFA_E_SIZE;
    if (workspace_bytes < qfa_continua_workspace_bytes(Npix, Nh)) return QFA_E_WORKSPACE;
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int pad = pad_of(Npix);
    float *img = (float *)workspace;
    const int64_t n = (int64_t)(Nh + 1) * pad;
    k_sample_image<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(F, mu, Npix, Nh, pad, img);
    dispatch_cont<32>(Nh, img, pad, h, R, Npix, out, st);
    return (int)hipGetLastError();
}

size_t qfa_mock_workspace_bytes(int Npix, int Nh) {
    if (Npix < 1 || Nh < 1 || Nh > 32) return 0;
    return (size_t)(Nh + 3 + 4) * mock_pad_of(Npix) * sizeof(float) + 16;
}

int qfa_mock_spectra_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *h,
                         int B, int S, int Npix, int Nb, int Nh, uint64_t seed, int64_t row0, float *flux, float *delta,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (!p || !mu || !b || !tau || !h || !workspace || (!flux && !delta)) return QFA_E_NULL;
    if (!p->F || !p->Psi || !p->tau0 || !p->c0 || !p->beta || !b->error) return QFA_E_NULL;
    if (B < 0 || S < 1 || Nh < 1 || Nh > 32 || row0 < 0 || row0 > INT64_MAX - B) return QFA_E_SIZE;
    if (Npix < 1 || Nb < 0 || Nb > Npix) return QFA_E_SIZE;
    // the blue side as check_batch (qfa_host.h) takes it: zabs, or zq1 + pix_ratio; A_blue on materialised zabs in batch order
    const bool fac = b->zq1 || b->pix_ratio;
    if (fac && !(b->zq1 && b->pix_ratio)) return QFA_E_NULL;
    if (b->A_blue && (fac || b->rows)) return QFA_E_NULL;
    if (Nb > 0 && (!p->omega || (!fac && !b->zabs))) return QFA_E_NULL;
    if (b->row_stride != 0 && b->row_stride < (int64_t)Npix) return QFA_E_SIZE;
    if (workspace_bytes < qfa_mock_workspace_bytes(Npix, Nh)) return QFA_E_WORKSPACE;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const qfa_batch_t bt = norm_batch(*b, Npix);
    const int pad = mock_pad_of(Npix);
    float *img = (float *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    float4 *ZP = (float4 *)(img + (size_t)(Nh + 3) * pad);
    const int64_t nimg = (int64_t)(Nh + 3) * pad;
    k_mock_image<<<(unsigned)((nimg + 255) / 256), 256, 0, st>>>(p->F, mu, p->Psi, p->omega, Npix, Nb, Nh, pad, img);
    int mode = kMockZabs;
    if (Nb > 0 && fac) {
        mode = kMockFactored;
        k_zfac_pix<<<(Nb + 255) / 256, 256, 0, st>>>(b->pix_ratio, *p, *tau, Nb, ZP);
    } else if (Nb > 0 && b->A_blue) {
        mode = kMockABlue;
    }
    // about 8192 blocks for a large call; a block writes at least 16 rows (b, s) so that its image loads are amortised; grid.x
    // stays below 2^30 blocks
    const int strips = pad / kMockStrip;
    int64_t rpb = ((int64_t)B * strips + 8191) / 8192;
    const int64_t least = (16 + S - 1) / S;
    if (rpb < least) rpb = least;
    const int64_t cap = ((int64_t)B * strips + 0x3fffffff) / 0x40000000;
    if (rpb < cap) rpb = cap;
    const int64_t chunks = (B + rpb - 1) / rpb;
    const unsigned grid = (unsigned)(chunks * strips);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    by_nhm(Nh, [&](auto nhm) {
        k_mock_spectra<decltype(nhm)::value><<<grid, kMockThreads, 0, st>>>(*p, bt, *tau, mode, img, pad, ZP, h, B, S, Npix, Nb, Nh, strips,
                                                                           (int)rpb, k0, k1, row0, flux, delta);
    });
    return (int)hipGetLastError();
}

}  // extern "C"
