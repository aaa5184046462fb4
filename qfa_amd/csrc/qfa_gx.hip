// qfa_gx.hip -- pass 2 on the XDL pipe (qfa_grads_x.h) in its own translation unit: the kernel is large and
// is iterated on separately from the rest of the library.
#include "qfa_grads_x.h"
#include "qfa_grads_t.h"       // (GTT: the image size; the kernel itself is built in qfa_gt.hip)
#include "qfa_predict_x.h"

#include "qfa_host.h"

size_t qfa_gx_image_bytes(int KP, int ntiles32) {            // the largest of the forms' images (one region serves all)
    return by_kp<16>(KP, [&](auto kp) {
        constexpr int K = decltype(kp)::value;
        return (size_t)ntiles32 * std::max(2 * (size_t)GTT<K>::TILE_B, (size_t)GXT<K>::TILE_B);      // (two 16-pixel tiles of k_grads_t per 32 pixels)
    });
}

// pass 2, two-role form (qfa_grads_x.h); its image is built by k_prep_step below
void qfa_gx_launch(int KP, const Pass2Call &a, int ntiles32, const WorkPlan &wp, unsigned char *PGX) {
    by_kp<16>(KP, [&](auto kp) {
        by_form(a.b, a.ZS != nullptr, a.exact != 0, [&](auto f) {
            using Fm = decltype(f);
            k_grads_x<decltype(kp)::value, Fm::hasa, Fm::zf><<<wp.items(), 512, 0, a.st>>>(a.p, a.b, a.tau, a.B, a.Npix, a.Nb, a.Nh, ntiles32, wp, PGX, a.SOL, a.ZS,
                                                                                         a.accum, a.rows, a.rowsS, a.row_stride, a.sc64, a.exact);
        });
    });
}

// ---- everything a training step derives from the parameters before pass 1, in ONE launch (N_h <= 16): the pass-1 image,
// the pass-2 image of the form that will run, the per-spectrum factors of the factored-z form, and (QFA_F_ZERO_ACCUM) the
// zeroing of the packed buffer.  The step of a small batch -- the reference's default is 500 spectra -- is a chain of a dozen
// dependent kernels of 3 - 30 us with ~3 us of dispatch latency between any two: five of them were these preparations
// (k_zfac_spec, k_zfac_pix, k_prep_pfx, a kernel of its own for the pass-2 image, torch's fill).  Block ranges: [pfx tiles | pass-2 tiles |
// 256 spectra each | 1024 floats of accum each]; the per-pixel factors are computed where they are needed (ZPSrc).
template <int KP, bool PIXRES>
__global__ __launch_bounds__(256) void k_prep_step(qfa_params_t p, qfa_tau_t tau, const float *__restrict__ zq1,
                                                   const float *__restrict__ pix_ratio, const int *__restrict__ rows, int B,
                                                   int Npix, int Nb, int Nh, int n_pfx, int n_p2, int n_zs,
                                                   unsigned char *__restrict__ PFX, unsigned char *__restrict__ P2,
                                                   float4 *__restrict__ ZS, float *__restrict__ zero, size_t n_zero,
                                                   unsigned *__restrict__ tick1) {
    const int b = (int)blockIdx.x;
    if (b == 0 && threadIdx.x == 0) *tick1 = 0u;             // arrival counter of k_solve<.., NLLRED> later in this step
    const ZPSrc zp{nullptr, pix_ratio, p.beta, tau.expo, -QFA_LOG2E * tau.offset};      // (offp as load_consts forms it)
    if (b < n_pfx) prep_pfx_body<KP>(b, n_pfx, p.F, p.Psi, p.omega, nullptr, zp, Npix, Nb, Nh, PFX);
    else if (b < n_pfx + n_p2) {
        if constexpr (PIXRES) prep_pgt_body<KP>(b - n_pfx, p.F, p.Psi, p.omega, zp, Npix, Nb, Nh, P2);
        else prep_pgx_body<KP>(b - n_pfx, p.F, p.Psi, p.omega, zp, Npix, Nb, Nh, P2);
    } else if (b < n_pfx + n_p2 + n_zs) zfac_spec_body((b - n_pfx - n_p2) * 256 + (int)threadIdx.x, zq1, rows, p, tau, B, ZS);
    else {
        const size_t i0 = (size_t)(b - n_pfx - n_p2 - n_zs) * 1024 + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + 256 * k < n_zero) zero[i0 + 256 * k] = 0.f;
    }
}
void qfa_prep_step_launch(int KP, bool pixres, const BatchCall &c, int ntiles32, unsigned char *PFX, unsigned char *P2, float4 *ZS,
                          float *zero, size_t n_zero, unsigned *tick1) {
    const bool zf = ZS != nullptr;
    const int n_pfx = ntiles32, n_zs = zf ? (c.B + 255) / 256 : 0;
    const size_t nz = zero ? n_zero : 0;
    const float *zq1 = zf ? c.b.zq1 : nullptr, *ratio = zf ? c.b.pix_ratio : nullptr;
    by_kp<16>(KP, [&](auto kp) {
        constexpr int K = decltype(kp)::value;
        const int n_p2 = pixres ? (c.Npix + GTT<K>::PXW - 1) / GTT<K>::PXW * GTT<K>::TPW : ntiles32;
        const unsigned grid = (unsigned)(n_pfx + n_p2 + n_zs + (nz + 1023) / 1024);
        if (XCfg<K>::F16) {         // the column maxima of the pass-1 image, in front of its builder
            unsigned *cm = pfx_colmax<K>(PFX, n_pfx);
            (void)hipMemsetAsync(cm, 0, sizeof(unsigned) * XCfg<K>::NCOL, c.st);
            k_colmax<K><<<n_pfx, 1024, 0, c.st>>>(c.p.F, c.p.Psi, c.Npix, c.Nh, cm);
        }
        auto go = [&](auto px) {
            k_prep_step<K, decltype(px)::value><<<grid, 256, 0, c.st>>>(c.p, c.tau, zq1, ratio, c.b.rows, c.B, c.Npix, c.Nb, c.Nh, n_pfx, n_p2, n_zs,
                                                                       PFX, P2, ZS, zero, nz, tick1);
        };
        if (pixres) go(std::true_type{});
        else go(std::false_type{});
    });
}

size_t qfa_px_image_bytes(int KP, int ntiles32) {
    return by_kp<16>(KP, [&](auto kp) { return (size_t)ntiles32 * PX<decltype(kp)::value>::TILE_B; });
}

void qfa_px_launch(int KP, const BatchCall &c, const float *mu, int ntiles32, const WorkPlan &wp, unsigned char *PXI, const float *SOL,
                   float *cont, float *unc) {
    by_kp<16>(KP, [&](auto kp) {
        constexpr int K = decltype(kp)::value;
        k_prep_px<K><<<ntiles32, 256, 0, c.st>>>(c.p.F, c.Npix, c.Nh, PXI);
        if constexpr (K == 8) {
            if (QFA_PX_SPW8 == 1 && px_realign(KP, c.Npix, cont, unc))
                k_predict_x<8, 1, true><<<wp.items(), 256, 0, c.st>>>(mu, c.B, c.Npix, ntiles32, wp, PXI, SOL, cont, unc);
            else
                k_predict_x<8, QFA_PX_SPW8><<<wp.items(), 256, 0, c.st>>>(mu, c.B, c.Npix, ntiles32, wp, PXI, SOL, cont, unc);
        } else {
            k_predict_x<16, QFA_PX_SPW><<<wp.items(), 256, 0, c.st>>>(mu, c.B, c.Npix, ntiles32, wp, PXI, SOL, cont, unc);
        }
    });
}

#if QFA_GX_STAMPS
extern "C" int qfa_gx_debug_stamps(unsigned long long *out) {      // diagnostic build only
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(qfa_gx_stamps), 64 * sizeof(unsigned long long));
}
#endif
