// qfa_s12_x.h -- pass 2 for N_h = 17..32, stages 1 and 2 on the XDL pipe (k_s12_x).
//
// k_grads_x (qfa_grads_x.h) does not scale to KP = 32: its hand-over slots, staging buffers and a 110 KiB image ring
// need 250 KiB of LDS, and stage 3 would need Z of 16 spectra for 32 columns in registers.  Pass 2 is therefore cut
// differently there:
//   k_s12_x      stage 1 ([f^T y | f^T C^-1' f], K = 32 + 528 as 18 K-steps of three v_mfma_f32_16x16x32_f16) and stage 2
//                (u, diag Sigma^-1, dG, the Psi / omega / tau0 / beta / c0 sums) for every (spectrum, pixel); the per-pixel
//                sums are flushed, beta = wD A^2 and gamma = A u go to HBM ([Bpad64][NpixPad] each);
//   k_grads_s3   (below) stage 3 from beta / gamma, once per 16 output columns.
// Lane layout, image builder, operand and stage 2 are those of role A of k_grads_x (qfa_stage1.h): a wave = 16 spectra,
// lane (lo = lane & 15, g = lane >> 4) owns spectra s0 + 4 g + r (r = 0..3) at the pixels 32 t + 2 lo + h of half h of
// tile t; the A operand of stage 1 (y, C^-1' of the wave's spectra as two float16 pieces, 144 registers) is loaded once
// per work item -- one wave per SIMD, 512 registers, built in the N_h > 16 translation unit.  Workgroup = 4 such waves =
// 64 spectra, no roles.
//
// The image of a 16-pixel half (18 K-steps x 2 pieces x 1 KiB = 36 KiB) moves through LDS in two QUARTERS of 9
// K-steps (ring of 3 x 19 KiB: a quarter + the parameter KiB of the half): a tile step is four sub-steps
// [issue the LDS-DMA of the quarter two ahead | the 27 MFMAs of this one (+ stage 2 of the half behind its second
// quarter) | counted wait for the next quarter | barrier].  The spectra go the way of k_grads_x: every wave streams the
// row segments of its 16 spectra (delta, sigma, zabs, mask) into its own LDS staging buffers by LDS-DMA TWO tiles ahead
// and copies the tile it starts on into registers.  Every request of the hot path is an asm statement, so hipcc inserts
// no vmcnt wait of its own (ordinary loads did: pass 2 at c5 5.2 ms against 4.2); the waits count the requests that
// may stay in flight (dma_wait_n), the requests per sub-step being known numbers.
#pragma once
#include "qfa_common.h"
#include "qfa_xdl_kernels.h"
#include "qfa_stage1.h"

template <int KP>
struct S12 : S1Layout<KP> {
    using L = S1Layout<KP>;
    static_assert(L::NKS % 2 == 0, "two quarters of NKS / 2 K-steps");
    static constexpr int NKQ = L::NKS / 2;                     // K-steps per quarter (9 of 18 at KP = 32): 27 MFMAs per 16 spectra x 16 pixels
    static constexpr int Q_B = NKQ * L::KS_B;                  // bytes of a quarter image (18 KiB)
    static constexpr int SLOT_B = Q_B + 1024;                  // ring slot: + the parameter KiB of the half
    static constexpr int HALF_B = 2 * Q_B + 1024;              // global: [quarter 0 | parameter KiB | quarter 1]
    static constexpr int TILE_B = 2 * HALF_B;                  // 74 KiB per 32-pixel tile
};

// ------------------------------------------------------------------------------------------------
// k_prep_s12 : F, Psi, omega -> the image above, one block per 32-pixel tile.
//   half h, K-step ks, piece, lane (g, lo), 8 k:  B[k = 32 ks + 8 g + j][px = 2 lo + h];  ks = 0: F[px][k];
//   ks >= 1: pair q = 32 (ks - 1) + 8 g + j -> F[px][a_q] F[px][b_q]
// ------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void k_prep_s12(const float *__restrict__ F, const float *__restrict__ Psi,
                                                  const float *__restrict__ omega, const float4 *__restrict__ ZP,
                                                  int Npix, int Nb, int Nh, unsigned char *__restrict__ IMG) {
    using X = S12<KP>;
    unsigned char *tile = IMG + (size_t)blockIdx.x * X::TILE_B;
    const int p0 = 32 * blockIdx.x;
    __shared__ S1Tile<KP + 1> T;
    s1_image<KP>(T, F, p0, Npix, Nh, [&](int h, int ks) {
        return tile + h * X::HALF_B + (ks / X::NKQ) * (X::Q_B + 1024) + (ks % X::NKQ) * X::KS_B;
    }, s1_no_hook);
    s1_params<KP>(T, p0, Psi, omega, zp_table(ZP), Npix, Nb, [&](int h) { return reinterpret_cast<float *>(tile + h * X::HALF_B + X::Q_B); });
}

// ------------------------------------------------------------------------------------------------
// The quarter ring of k_s12_x and k_predict_x32: quarter u = 4 c + 2 h + j (tile c of the work item, half h, K-range j) of
// the image goes into ring slot u % 3 two sub-steps ahead.
// ------------------------------------------------------------------------------------------------
// the tile order of a work item, de-phased between workgroups (a small window: the workgroups of an XCD then stream the
// same few tiles of the image through its L2)
struct TileWalk {
    int t0, n, rot;
    __device__ __forceinline__ TileWalk(int blk, int t0_, int n_)
        : t0(t0_), n(n_), rot(n_ > 0 ? (int)(((unsigned)blk * 2654435761u) % (unsigned)min(n_, 4)) : 0) {}
    __device__ __forceinline__ int operator()(int c) const {
        int x = c + rot;
        if (x >= n) x -= n;
        return t0 + x;
    }
};
// LDS-DMA of quarter u of tile tg into `dst`; wave wv moves the 1-KiB pieces wv, wv + 4, ...; the quarter with j = 0 is
// followed by the half's parameter KiB
template <int KP>
__device__ __forceinline__ void get_quarter(const unsigned char *__restrict__ IMG, int tg, int u, unsigned char *dst, int wv, int lane) {
    using X = S12<KP>;
    const int h = (u >> 1) & 1, j = u & 1;
    const unsigned char *src = uniform_ptr(IMG + (size_t)tg * X::TILE_B + h * X::HALF_B + j * (X::Q_B + 1024));
    constexpr int NCH = X::Q_B / 1024;
#pragma unroll
    for (int i = 0; i < (NCH + 1 + 3) / 4; ++i) {
        const int ch = wv + 4 * i;
        if (ch < NCH) glds16a(src + ch * 1024, (unsigned)lane * 16u, wave_uniform(lds_addr(dst + ch * 1024)));
        else if (ch == NCH && j == 0)
            glds16a(src + X::Q_B, (unsigned)lane * 16u, wave_uniform(lds_addr(dst + X::Q_B)));
    }
}
// pieces of quarter u moved by wave wv (get_quarter; piece NCH = the parameter KiB, j = 0): what the counted waits count
template <int KP>
__device__ __forceinline__ int cnt_q(int u, int wv) {
    constexpr int NCHQ = S12<KP>::Q_B / 1024;
    return (NCHQ - wv + 3) / 4 + ((NCHQ % 4 == wv && !(u & 1)) ? 1 : 0);
}
// The K-steps of quarter J of a half on ring slot `img`: B pieces of K-step ks + 1 are read while the three MFMAs of ks
// run.  J = 0 starts the half: it1 / it2 = 1 / t, 1 / t^2 of the lane's pixel, and par(po) reads what else the kernel
// takes from the parameter KiB po; J = 1 ends it with the powers of two back in (element r <-> spectrum 4 g + r).
template <int KP, int J, class Par>
__device__ __forceinline__ void quarter(const unsigned char *img, int lane, const S1Op<KP> &A, f32x4 &afy, f32x4 &aq, float &it1,
                                        float &it2, Par par) {
    using X = S12<KP>;
    const unsigned char *bp = img + lane * 16;
    if (J == 0) {
        afy = f32x4{0.f, 0.f, 0.f, 0.f};
        aq = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *po = reinterpret_cast<const float *>(img + X::Q_B);
        par(po);
        it1 = po[X::PAR_IT1 + (lane & 15)]; it2 = po[X::PAR_IT2 + (lane & 15)];
    }
    constexpr int NP = X::NP;
    u32x4 bq[2][NP];
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) bq[0][pc] = *reinterpret_cast<const u32x4 *>(bp + pc * 1024);
#pragma unroll
    for (int kq = 0; kq < X::NKQ; ++kq) {
        if (kq + 1 < X::NKQ) {
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                bq[(kq + 1) & 1][pc] = *reinterpret_cast<const u32x4 *>(bp + (kq + 1) * X::KS_B + pc * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        const u32x4 &bh = bq[kq & 1][0], &bm = bq[kq & 1][1];
        // (ks = NKQ J + kq is a compile-time constant per (J, kq))
        if (J == 0) {
            if (kq == 0) afy = xdl3h(A.h[0], A.m[0], bh, bm, afy);
            else aq = xdl3h(A.h[kq], A.m[kq], bh, bm, aq);
        } else {
            aq = xdl3h(A.h[X::NKQ + kq], A.m[X::NKQ + kq], bh, bm, aq);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (J == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            afy[r] = (afy[r] * A.is0[r]) * it1;
            aq[r] = (aq[r] * A.is1[r]) * it2;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_s12_x.  One work item = (block of 64 spectra, range of 32-pixel tiles).  slab != NULL: deterministic mode (the
// per-pixel sums go to row blk of the slab by plain stores, the scalar sums to slabS[item][wave][3]).
// ------------------------------------------------------------------------------------------------
template <int KP, bool HASA, bool ZF, bool EXACT>   // EXACT: QFA_F_EXACT_GRAD's tau0 / c0 / beta terms (as in k_grads_t)
__global__ __launch_bounds__(256, 1) void k_s12_x(qfa_params_t p, qfa_batch_t bt, qfa_tau_t tau, int B, int Npix, int Nb,
                                                  int Nh, int ntiles, WorkPlan wp, const unsigned char *__restrict__ IMG,
                                                  const float *__restrict__ SOL, float *__restrict__ BG,
                                                  float *__restrict__ GG, int bg_stride, float *__restrict__ accum,
                                                  float *__restrict__ slab, double *__restrict__ slabS, int slab_stride,
                                                  Scal64 *__restrict__ sc64, const float4 *__restrict__ ZS) {
    using C = Cfg<KP>;
    using X = S12<KP>;
    constexpr int RING = 3;                                    // quarters in LDS: two of DMA distance (the image streams
                                                               // from the Infinity Cache: 27.5 MB at c5 against 4 MB of L2)
    __shared__ __attribute__((aligned(16))) unsigned char lds[RING][X::SLOT_B];
    __shared__ __attribute__((aligned(16))) unsigned char lstg[4][2][X::STG_B];      // [wave][tile parity]
    __shared__ float lpsum[2][4][4][32];                       // [tile parity][wave][sumA | gPsi | gOmega | cnt][32 px]
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    const int lo = lane & 15, g = lane >> 4;
    int blk, seg, t0, t1;
    plan_item(wp, blockIdx.x, ntiles, blk, seg, t0, t1);
    const int s0 = blk * 64 + wv * 16;
    const bool active = s0 < B;                                // wave-uniform
    const int n = t1 - t0;
    const int nbt = (Nb + 31) >> 5;
    const DevConsts k = load_consts(p, tau);
    const bool det = slab != nullptr;
    float *accA = (det ? slab + (size_t)blk * (size_t)slab_stride : accum) + (size_t)Npix * Nh;   // sumA | gPsi | gOmega | cnt
    float *accS = accum + (size_t)Npix * Nh + 3 * (size_t)Npix + Nb;
    for (int i = tid; i < 2 * 4 * 4 * 32; i += 256) (&lpsum[0][0][0][0])[i] = 0.f;      // inactive waves' rows stay 0

    S1Op<KP> A;                                                // [y | C^-1'] pieces, inverse powers of two of the spectra 4 g + r
    {
        const bool v = active && (s0 + lo) < B;
        s1_operand<KP>(SOL + (size_t)(v ? s0 + lo : 0) * C::NSOL, v, g, A);
    }
    bool sv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sv[r] = active && (s0 + 4 * g + r) < B;
    const TileWalk tile_of(blk, t0, n);

    // Staging (qfa_grads_x.h): slot q of an array holds row q ^ ((q >> 2) & 1); 16-byte pieces, two instructions per
    // float array, the mask as 4-byte pieces.  Returns the requests issued: 8 (all 32 pixels inside the row and, on a blue
    // tile, inside the blue side), else 0 = "ragged: ordinary loads and LDS stores, wait for everything".
    const int last_row = active ? min(15, B - 1 - s0) : 0;          // wave-uniform
    // Spectrum s0 + r of the batch is row batch_row(s0 + r) of the batch arrays (ABI v3: rows / row_stride, qfa_common.h);
    // the rows of the lane's two 16-byte pieces per array stay in registers (one wave per SIMD: room to spare)
    const unsigned RS = (unsigned)bt.row_stride;                     // (elements; < 2^31: check_batch)
    unsigned R2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) R2[i] = (unsigned)batch_row(bt, (active ? s0 : 0) + (int)slot_row(8 * i + (lane >> 3), last_row));
    auto stage_tile = [&](int tg, int par) -> int {
        const bool zblue = !ZF && tg < nbt;                                               // wave-uniform
        const bool fast = (32 * tg + 31 < Npix) && (!zblue || 32 * tg + 31 < Nb) && !QFA_TRACKED_LOADS;
        // the third array: zabs rows (Nb apart, Nb long) on a blue tile, else the delta rows again
        const float *zb = zblue ? bt.zabs : bt.delta;
        const unsigned zpitch = zblue ? (unsigned)Nb : RS;
        const int zlen = zblue ? Nb : Npix;
        unsigned char *buf = lstg[wv][par];
        if (fast) {
            const unsigned dst = wave_uniform(lds_addr(buf));
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned pc = 32u * (unsigned)tg + 4u * (unsigned)(lane & 7);       // first pixel of the piece
                const unsigned long long o = (unsigned long long)R2[i] * RS + pc;
                glds16p(lane_ptr<2>(bt.delta, o), dst + 0 * X::STG_ARR + i * 1024);
                glds16p(lane_ptr<2>(bt.error, o), dst + 1 * X::STG_ARR + i * 1024);
                if (!ZF) glds16p(lane_ptr<2>(zb, (unsigned long long)R2[i] * zpitch + pc), dst + 2 * X::STG_ARR + i * 1024);
                glds4p(lane_ptr<0>(bt.mask, o), dst + X::STG_MASK + i * 256);
            }
            return ZF ? 6 : 8;
        }
        float *sf = reinterpret_cast<float *>(buf);
        unsigned char *mb = buf + X::STG_MASK;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const int q = 2 * i + (lane >> 5), pxl = lane & 31;
            const unsigned long long R = batch_row(bt, (active ? s0 : 0) + (int)slot_row(q, last_row));
            const int px = 32 * tg + pxl;
            const unsigned long long o = R * RS + (unsigned)min(px, Npix - 1);
            sf[0 * (X::STG_ARR / 4) + q * 32 + pxl] = bt.delta[o];
            sf[1 * (X::STG_ARR / 4) + q * 32 + pxl] = bt.error[o];
            if (!ZF) sf[2 * (X::STG_ARR / 4) + q * 32 + pxl] = zb[R * zpitch + (unsigned)min(px, zlen - 1)];
            mb[q * 32 + pxl] = px < Npix ? bt.mask[o] : (unsigned char)0;
        }
        return 0;
    };
    // (the copy-out of k_grads_x on scalars: with its float pairs hipcc packs and contracts stage 2 below differently, and
    // the gradients change in their last bits -- qfa_stage1.h)
    struct Spec {                      // one lane's 4 spectra x 2 pixels of a tile; sigma < 0: masked
        float d[4][2], sg[4][2], z[4][2];
    };
    auto take_tile = [&](int par, Spec &cur) {
        const unsigned char *sb = lstg[wv][par] + 8 * lo;
        const unsigned char *mb = lstg[wv][par] + X::STG_MASK + 2 * lo;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int slot = 4 * g + (r ^ (g & 1));
            const f32x2 d2 = *reinterpret_cast<const f32x2 *>(sb + 0 * X::STG_ARR + slot * 128);
            const f32x2 e2 = *reinterpret_cast<const f32x2 *>(sb + 1 * X::STG_ARR + slot * 128);
            f32x2 z2 = {0.f, 0.f};
            if (!ZF) z2 = *reinterpret_cast<const f32x2 *>(sb + 2 * X::STG_ARR + slot * 128);
            const unsigned mk = *reinterpret_cast<const unsigned short *>(mb + slot * 32);
            cur.d[r][0] = d2[0]; cur.d[r][1] = d2[1];
            cur.sg[r][0] = (mk & 0xffu) ? fabsf(e2[0]) : -1.f;        // (sign bit = masked; only sigma^2 is used)
            cur.sg[r][1] = (mk & 0xff00u) ? fabsf(e2[1]) : -1.f;
            cur.z[r][0] = z2[0]; cur.z[r][1] = z2[1];
        }
    };
    auto get_q = [&](int u) { get_quarter<KP>(IMG, tile_of(u >> 2), u, lds[u % RING], wv, lane); };

    double s_tau0 = 0.0, s_c0 = 0.0, s_beta = 0.0;
    f32x4 afy, aq;
    S2Pix pxp{0.f, 0.f, 0.f, 0.f, 0.f};
    float it1H = 1.f, it2H = 1.f;
    ZFac zs[4];                                   // factored-z form: per-spectrum factors of the lane's four spectra
#pragma unroll
    for (int r = 0; r < 4; ++r) zs[r] = zfac_load(ZS, s0 + 4 * g + r, ZF && sv[r]);
    auto params = [&](const float *po) {          // the lane's pixel of a half, from its parameter KiB
        pxp.Psi = po[X::PAR_PSI + lo];
        pxp.om = po[X::PAR_OM + lo];
        if (ZF) { pxp.ti = po[X::PAR_TI + lo]; pxp.pwi = po[X::PAR_PWI + lo]; pxp.l2i = po[X::PAR_L2I + lo]; }
    };

    // stage 2 of the lane's four elements of half h of tile tg (as role A of k_grads_x), beta / gamma to HBM, per-pixel
    // sums of the wave to its LDS row
    float t_tau0 = 0.f, t_c0 = 0.f, t_beta = 0.f;
    auto stage2 = [&](auto blue_tag, int tg, int h, const Spec &cur, int par) {
        constexpr bool BLUE = decltype(blue_tag)::value;
        const int px = 32 * tg + 2 * lo + h;
        const bool inb = px < Npix;
        const bool blue = px < Nb;
        const float Psi = pxp.Psi, om = pxp.om;
        float gPsi = 0.f, gOm = 0.f, sA = 0.f, cnt = 0.f;
        float betaR[4], gamR[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sg = cur.sg[r][h];
            const bool wv_ = inb & sv[r] & (__float_as_int(sg) >= 0);
            const float dd = wv_ ? cur.d[r][h] : 0.f;
            if (BLUE) {
                float l2, pw, Ab, re, ex;
                if (ZF) {                                                                         // qfa_common.h, ZFac
                    l2 = zs[r].l2 + pxp.l2i;
                    pw = zs[r].pw * pxp.pwi;
                    Ab = fast_exp2(fmaf(zs[r].ts, pxp.ti, k.offp));                               // QFA/model.py:125
                    ex = fast_exp2(k.k1 * pw);
                    re = k.omc0 - ex;                                                             // QFA/utils.py:91
                } else {
                    l2 = fast_log2(1.0f + cur.z[r][h]);
                    pw = fast_exp2(k.beta * l2);
                    const float tauv = k.t_amp * fast_exp2(k.t_expo * (l2 + k.t_lscale)) + k.t_off;   // QFA/utils.py:105-141
                    Ab = fast_exp2(-tauv * QFA_LOG2E);                                            // QFA/model.py:125
                    ex = fast_exp2(-k.tau0 * pw * QFA_LOG2E);
                    re = 1.0f - k.c0 - ex;                                                        // QFA/utils.py:91
                }
                if (HASA) Ab = bt.A_blue[(size_t)(active ? min(s0 + 4 * g + r, B - 1) : 0) * Nb + min(px, Nb - 1)];
                const float Av = blue ? Ab : 1.f;
                const float zd = blue ? re * re : 0.f;
                // exact mode: exp(-t) enters the tau0 / beta terms through pw at once (one register less across the element:
                // with ex live the factored instantiation spilled two VGPRs)
                const float er2 = EXACT ? 2.0f * om * (blue ? re : 0.f) : 0.f;
                if (EXACT) pw *= ex;
                const float A2 = Av * Av;
                const float D = A2 * Psi + om * zd + sg * sg;
                const float wD = wv_ ? fast_rcp(D) : 0.f;
                const float wDA = wD * Av;
                const float uu = wD * (dd - Av * afy[r]);                   // (Sigma^-1 delta)_i
                const float dS = wD - wDA * wDA * aq[r];                    // diag(Sigma^-1)_i
                const float dG = 0.5f * (dS - uu * uu);                     // QFA/model.py:136,138
                gPsi += A2 * dG;                                            // :139
                gOm += dG * zd;                                             // :140
                const float root = 1.0f - k.tau0 * pw - k.c0;               // :141
                const float er = dG * (om * zd) * zd * 2.0f * root;
                // exact: dNLL/dzd = dG omega, dzd/dc0 = -2 re, dzd/dtau0 = 2 re exp(-t) (1+z)^beta (qfa_hip.h); pw = (1+z)^beta exp(-t)
                const float ee = dG * er2;
                const float e = EXACT ? ee : er, et = EXACT ? -ee : er;
                t_tau0 -= et * pw;                                          // :142
                t_beta -= et * (k.tau0 * pw * (l2 * QFA_LN2));              // :143
                t_c0 -= e;                                                  // :144
                cnt += wv_ ? 1.f : 0.f;
                betaR[r] = wDA * Av;
                sA += betaR[r] * Av;
                gamR[r] = Av * uu;
            } else {                                                        // red side: A = 1, zd = 0
                const float D = Psi + sg * sg;
                const float wD = wv_ ? fast_rcp(D) : 0.f;
                const float uu = wD * (dd - afy[r]);
                const float dS = wD - wD * wD * aq[r];
                gPsi += 0.5f * (dS - uu * uu);
                cnt += wv_ ? 1.f : 0.f;
                betaR[r] = wD;
                sA += wD;
                gamR[r] = uu;
            }
        }
        if (active) {  // (bg_stride >= 32 ntiles: every pixel of the last tile has its own slot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t o = (size_t)(s0 + 4 * g + r) * bg_stride + px;
                BG[o] = betaR[r];
                GG[o] = gamR[r];
            }
        }
        // per-pixel sums over the wave's 16 spectra: quantity q ends up in the 16-lane row q
        lpsum[par][wv][g][2 * lo + h] = wave_pixel_sums(sA, gPsi, gOm, cnt);
        if (BLUE && h == 1) {
            s_tau0 += (double)t_tau0;
            s_c0 += (double)t_c0;
            s_beta += (double)t_beta;
            t_tau0 = 0.f; t_c0 = 0.f; t_beta = 0.f;
        }
    };
    // per-pixel sums [sumA | gPsi | gOmega | cnt] of tile tg: thread (which = tid >> 5, pxl = tid & 31) of the first 128.
    // Every lane issues its request (the waits count it): a lane outside the arrays adds 0 to an element inside them, a
    // different one per lane, or -- deterministic mode -- stores into the spare floats at the end of the slab row.
    float *sink = (det ? slab + (size_t)blk * (size_t)slab_stride + (slab_stride - 64) : accum) + lane;
    auto flush_P = [&](int tg, int par) {
        if (tid >= 128) return;
        const int which = tid >> 5, pxl = tid & 31;
        const float v = (lpsum[par][0][which][pxl] + lpsum[par][1][which][pxl]) +
                        (lpsum[par][2][which][pxl] + lpsum[par][3][which][pxl]);
        const int px = 32 * tg + pxl;
        const bool ok = (px < Npix) & ((which != 2) | (px < Nb));
        const int pxc = min(px, Npix - 1);
        // (a red pixel's lane of the gOmega group adds 0 to the pixel's count instead)
        const int offc = (which == 2 && pxc >= Nb) ? 2 * Npix + Nb + pxc : which * Npix - (which == 3 ? Npix - Nb : 0) + pxc;
        if (det) *(ok ? accA + offc : sink) = v;
        else atomicAdd(accA + offc, ok ? v : 0.f);
    };

    if (n > 0) {
        // requests a sub-step puts into this wave's queue BEHIND its image DMA: the flush atomic of (h0, j0) (waves 0, 1),
        // the staging of tile c + 2 issued there, the eight beta / gamma stores of a sub-step with stage 2
        int stag_a = 0, stag_b = 0;                 // staging requests in flight for buffer 0 / 1 (0: not a counted issue)
        bool drain = false;                         // a ragged staging is pending: wait for everything
        if (active) {
            stag_a = stage_tile(tile_of(0), 0);
            if (n > 1) stag_b = stage_tile(tile_of(1), 1);
        }
        get_q(0);
        if (4 * n > 1) get_q(1);
        dma_wait<0>();
        step_barrier();
        int rest_prev = 0;                          // requests of the previous sub-step behind its image DMA
        Spec cur;
        auto tile_step = [&](int c, int &stag_cur) {
            const int tg = tile_of(c);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int u = 4 * c + 2 * h + j;
                    const bool more = u + 2 < 4 * n;
                    if (more) get_q(u + 2);                       // (slot of quarter u - 1: free behind the barrier)
                    int rest = 0;
                    if (h == 0 && j == 0) {
                        if (c >= 1) {
                            flush_P(tile_of(c - 1), (c - 1) & 1);
                            rest += tid < 128 ? 1 : 0;
                        }
                        if (active) {
                            take_tile(c & 1, cur);
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // staging buffer read: it may be overwritten
                            stag_cur = 0;
                            if (c + 2 < n) {
                                stag_cur = stage_tile(tile_of(c + 2), c & 1);
                                if (stag_cur == 0) drain = true;
                                rest += stag_cur;
                            }
                        }
                    }
                    if (active) {
                        if (j == 0) quarter<KP, 0>(lds[u % RING], lane, A, afy, aq, it1H, it2H, params);
                        else quarter<KP, 1>(lds[u % RING], lane, A, afy, aq, it1H, it2H, params);
                        if (j == 1) {
                            if (tg < nbt) stage2(std::true_type{}, tg, h, cur, c & 1);
                            else stage2(std::false_type{}, tg, h, cur, c & 1);
                            rest += 8;
                        }
                    }
                    // the DMA of quarter u + 1 (issued at the start of the previous sub-step) must have landed; behind it in
                    // the queue: the rest of the previous sub-step, this sub-step's DMA and its rest
                    if (!more || drain) dma_wait<0>();
                    else dma_wait_n(rest_prev + cnt_q<KP>(u + 2, wv) + rest);
                    if (drain && (h == 1 && j == 1)) drain = false;       // (everything has been waited for since)
                    rest_prev = rest;
                    step_barrier();
                }
            }
        };
        for (int c = 0; c < n; c += 2) {
            tile_step(c, stag_a);
            if (c + 1 < n) tile_step(c + 1, stag_b);
        }
        flush_P(tile_of(n - 1), (n - 1) & 1);
    }
    if (active) {
        for (int o = 32; o >= 1; o >>= 1) {
            s_tau0 += __shfl_xor(s_tau0, o);
            s_c0 += __shfl_xor(s_c0, o);
            s_beta += __shfl_xor(s_beta, o);
        }
    }
    if (lane == 0) {
        if (det) {
            double *q = slabS + ((size_t)blockIdx.x * 4 + wv) * 3;
            q[0] = active ? s_tau0 : 0.0; q[1] = active ? s_c0 : 0.0; q[2] = active ? s_beta : 0.0;
        } else {
            scal64_commit(sc64, active ? s_tau0 : 0.0, active ? s_c0 : 0.0, active ? s_beta : 0.0, gridDim.x * 4u, accS);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_predict_x32 (N_h = 17..32): the posterior writer on the XDL pipe -- cont = F hmean + mu, unc = sqrt(f^T hcov f) for
// ALL pixels of every spectrum (reference QFA/model.py:177-180).  It is stage 1 of k_s12_x with [hmean | hcov'] (as
// k_solve<KP, true> leaves them in SOL) in the place of [y | C^-1']: same image (k_prep_s12 called with mu in the place
// of Psi, so the half's KiB carries mu of the lane's pixel), same quarter ring, same counted waits; no spectra are read.
// Lane (lo, g) owns the pixels 32 t + 2 lo + h of the spectra s0 + 4 g + r: one 8-byte store per spectrum row and
// array behind the second half (128 contiguous bytes per row and wave instruction), eight requests per tile.
// ------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256, 1) void k_predict_x32(int B, int Npix, int ntiles, WorkPlan wp,
                                                        const unsigned char *__restrict__ IMG,
                                                        const float *__restrict__ SOL, float *__restrict__ cont,
                                                        float *__restrict__ unc) {
    using C = Cfg<KP>;
    using X = S12<KP>;
    constexpr int RING = 3;
    __shared__ __attribute__((aligned(16))) unsigned char lds[RING][X::SLOT_B];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    const int lo = lane & 15, g = lane >> 4;
    int blk, seg, t0, t1;
    plan_item(wp, blockIdx.x, ntiles, blk, seg, t0, t1);
    const int s0 = blk * 64 + wv * 16;
    const bool active = s0 < B;                                // wave-uniform
    const int n = t1 - t0;
    if (n <= 0) return;

    S1Op<KP> A;                                                // [hmean | hcov'] pieces, inverse powers of two of the spectra 4 g + r
    {
        const bool v = active && (s0 + lo) < B;
        s1_operand<KP>(SOL + (size_t)(v ? s0 + lo : 0) * C::NSOL, v, g, A);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // (the operand loads above are the only tracked loads)
    const bool full_wave = active && s0 + 16 <= B;
    const TileWalk tile_of(blk, t0, n);
    auto get_q = [&](int u) { get_quarter<KP>(IMG, tile_of(u >> 2), u, lds[u % RING], wv, lane); };
    f32x4 afy, aq;
    float muH = 0.f, it1H = 1.f, it2H = 1.f;
    auto params = [&](const float *po) { muH = po[X::PAR_PSI + lo]; };       // (the image was built with mu in the place of Psi)

    get_q(0);
    if (4 * n > 1) get_q(1);
    dma_wait<0>();
    step_barrier();
    int rest_prev = 0;                             // stores of the previous sub-step, behind its image DMA in the queue
    float co0[4], un0[4];
    for (int c = 0; c < n; ++c) {
        const int tg = tile_of(c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int u = 4 * c + 2 * h + j;
                const bool more = u + 2 < 4 * n;
                if (more) get_q(u + 2);
                int rest = 0;
                bool drain = false;
                if (active) {
                    if (j == 0) quarter<KP, 0>(lds[u % RING], lane, A, afy, aq, it1H, it2H, params);
                    else quarter<KP, 1>(lds[u % RING], lane, A, afy, aq, it1H, it2H, params);
                    if (j == 1 && h == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            co0[r] = afy[r] + muH;
                            un0[r] = __builtin_amdgcn_sqrtf(aq[r]);
                        }
                    }
                    if (j == 1 && h == 1) {
                        const int px = 32 * tg + 2 * lo;
                        if (full_wave && 32 * tg + 31 < Npix) {          // wave-uniform: exactly eight store instructions
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const size_t o = (size_t)(s0 + 4 * g + r) * Npix + px;
                                store2_nt(cont + o, co0[r], afy[r] + muH);
                                store2_nt(unc + o, un0[r], __builtin_amdgcn_sqrtf(aq[r]));
                            }
                            rest = 8;
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int sp = s0 + 4 * g + r;
                                if (sp < B && px < Npix) {
                                    cont[(size_t)sp * Npix + px] = co0[r];
                                    unc[(size_t)sp * Npix + px] = un0[r];
                                }
                                if (sp < B && px + 1 < Npix) {
                                    cont[(size_t)sp * Npix + px + 1] = afy[r] + muH;
                                    unc[(size_t)sp * Npix + px + 1] = __builtin_amdgcn_sqrtf(aq[r]);
                                }
                            }
                            drain = true;
                        }
                    }
                }
                // the DMA of quarter u + 1 (issued at the start of the previous sub-step) must have landed; behind it in the
                // queue: the stores of the previous sub-step, this sub-step's DMA and its stores
                if (!more || drain) dma_wait<0>();
                else dma_wait_n(rest_prev + cnt_q<KP>(u + 2, wv) + rest);
                rest_prev = drain ? 0 : rest;
                step_barrier();
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_grads_s3 (N_h = 17..32): stage 3 of pass 2 alone, for the output columns 16 bhalf .. 16 bhalf + 15, from the
// beta / gamma k_s12_x (or k_grads) stored:  accF[px][b] += sum_s beta_{s,px} (F_tile Z_s)[px][b] + sum_s gamma_{s,px} p_s[b].
// Work items and flush as k_grads (16-pixel tiles, 4 waves = 64 spectra, per-wave LDS slots summed in fixed order);
// lane (px = lane & 15, g = lane >> 4): rows 4 g + r of the products.  Z_s (K = a = 32) as two bf16 pieces of all 16
// spectra in 128 registers, TERMS piece products per spectrum (template argument: six by default, on float16 pieces; three with QFA_F_S3_FAST); 54 MFMAs and 64 FMAs per tile, no transcendental.
// Inputs of a tile arrive by LDS-DMA TWO tiles ahead into the wave's own buffers (ring of 3 x 4 KiB): the beta and gamma
// tiles of its 16 spectra ([s][16 px] float, 64-byte row segments: one instruction each, and already the layout the
// beta-scaling reads) and the two F pieces (1 KiB each).  A wave's queue holds those four requests per tile and its one
// flush request; the wait at the start of a tile leaves the ten youngest in flight.
// ------------------------------------------------------------------------------------------------
template <int KP, int TERMS>      // TERMS: bf16 piece products per stage-3 contraction -- 6 (default: float32 grade; the third
                                  // piece of Z is 64 more registers: one workgroup per CU), 4 or 3 (QFA_F_S3_FAST)
__global__ __launch_bounds__(256, 2) void k_grads_s3(int B, int Npix, int Nh, int ntiles, WorkPlan wp, int bhalf,
                                                     const float *__restrict__ PFT, const float *__restrict__ SOL,
                                                     const float *__restrict__ BG, const float *__restrict__ GG,
                                                     int bg_stride, float *__restrict__ accum, float *__restrict__ slab,
                                                     int slab_stride) {
    static_assert(KP == 32, "k_grads_s3: N_h = 17..32");
    using C = Cfg<KP>;
    // Round 5 (TERMS == 6 only): G_s = F_tile Z_s on TWO float16 pieces per operand, three products.  Both operands are
    // prepared: F t_px (k_prep_pft; 1 / t_px rides as a fifth KiB) and Z_s 2^k of the wave's own spectra (scaled by their largest
    // element below); beta multiplies G in float32 behind the MFMA as before, so nothing here depends on the range of the data.
    constexpr bool F16 = TERMS == 6;
    constexpr int RING = 3, BUF_B = TERMS == 6 ? 5120 : 4096;   // per wave and tile: beta 1 KiB | gamma 1 KiB | Fh 1 KiB | Fm 1 KiB (| F16: 1 / t)
    constexpr int NREQ = TERMS == 6 ? 5 : 4;                    // input requests per wave and tile
    __shared__ __attribute__((aligned(16))) unsigned char lin[4][RING][BUF_B];
    __shared__ float ldspart[2][4][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    const int lo = lane & 15, g = lane >> 4;
    int blk, seg, t0, t1;
    plan_item(wp, blockIdx.x, ntiles, blk, seg, t0, t1);
    const int s0 = (blk * 4 + wv) * 16;
    const bool active = s0 < B;
    const int n = t1 - t0;
    const bool det = slab != nullptr;
    float *accF = det ? slab + (size_t)blk * (size_t)slab_stride : accum;
    float *sink = (det ? accF + (slab_stride - 64) : accum) + lane;
    for (int i = tid; i < 2 * 4 * 256; i += 256) (&ldspart[0][0][0])[i] = 0.f;      // inactive waves' slots stay 0

    // B operands: Z_s[a = 8g + j][col] of all 16 spectra as two bf16 pieces, p of the spectra 4g + j (gamma term)
    u32x4 Zh[16], Zm[16];
    float iz[16];                                               // F16: 1 / scale of Z_s (wave-uniform)
    u32x2 ph, pm, pl;
    {
        const int zcol = 16 * bhalf + lo;
        float zraw[16][8];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const bool v = active && (s0 + s) < B && zcol < KP;
            const float *sol = SOL + (size_t)(v ? s0 + s : 0) * C::NSOL + C::SOL_Z + zcol;
#pragma unroll
            for (int j = 0; j < 8; ++j) zraw[s][j] = v ? sol[(8 * g + j) * KP] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if constexpr (F16) {
                float mx = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(zraw[s][j]));
#pragma unroll
                for (int o = 1; o <= 32; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));      // the 32 x 16 block of Z_s this wave holds
                const float sc = f16_row_scale(mx, iz[s]);
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = zraw[s][j] * sc;
                split8h(x, Zh[s], Zm[s]);
            } else {
                iz[s] = 1.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned h, m, l;
                    split2(zraw[s][2 * q], zraw[s][2 * q + 1], h, m, l);
                    Zh[s][q] = h;
                    Zm[s][q] = m;
                }
            }
        }
        float pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool v = active && (s0 + 4 * g + r) < B && zcol < KP;
            pr[r] = v ? SOL[(size_t)(s0 + 4 * g + r) * C::NSOL + C::SOL_P + zcol] : 0.f;
        }
        unsigned h0, m0, l0, h1, m1, l1;
        split2(pr[0], pr[1], h0, m0, l0);
        split2(pr[2], pr[3], h1, m1, l1);
        ph = u32x2{h0, h1}; pm = u32x2{m0, m1}; pl = u32x2{l0, l1};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the operand loads above are the only tracked ones)
    const int rot = n > 0 ? (int)(((unsigned)blk * 2654435761u) % (unsigned)min(n, 32)) : 0;
    auto tile_of = [&](int c) {
        int x = c + rot;
        if (x >= n) x -= n;
        return t0 + x;
    };
    // the four input requests of tile tg: lane = (row = lane >> 2, 16-byte piece = lane & 3) of the 64-byte row segments
    const float *bgw = uniform_ptr(BG + (size_t)(active ? s0 : 0) * bg_stride);
    const float *ggw = uniform_ptr(GG + (size_t)(active ? s0 : 0) * bg_stride);
    auto get_tile = [&](int c) {
        const int tg = tile_of(c);
        const unsigned dst = wave_uniform(lds_addr(lin[wv][c % RING]));
        const unsigned o = 4u * ((unsigned)(lane >> 2) * (unsigned)bg_stride + 16u * (unsigned)tg + 4u * (unsigned)(lane & 3));
        glds16a(bgw, o, dst);
        glds16a(ggw, o, dst + 1024);
        const float *fg = uniform_ptr(PFT + (size_t)tg * C::TILE_PFT + C::PFT_MAIN);
        if constexpr (F16) {                    // float16 pieces h, m and the KiB with 1 / t_px
            glds16a(fg + C::PFT_F16H, (unsigned)lane * 16u, dst + 2048);
            glds16a(fg + C::PFT_F16M, (unsigned)lane * 16u, dst + 3072);
            glds16a(fg + C::PFT_F16IT, (unsigned)lane * 16u, dst + 4096);
        } else {
            glds16a(fg, (unsigned)lane * 16u, dst + 2048);
            glds16a(fg + 256, (unsigned)lane * 16u, dst + 3072);
        }
    };
    auto flush = [&](int tg, const float (*pp)[256]) {
        const int idx = lane + 64 * wv;
        const float v = (pp[0][idx] + pp[1][idx]) + (pp[2][idx] + pp[3][idx]);
        const int px = 16 * tg + (idx >> 4), b = 16 * bhalf + (idx & 15);
        const bool ok = (b < Nh) & (px < Npix);
        // every lane issues its request (the wait counts it): a lane outside the array adds 0 inside it / stores to the sink
        float *q = accF + (size_t)min(px, Npix - 1) * Nh + (b < Nh ? b : b % Nh);
        if (det) *(ok ? q : sink) = v;
        else atomicAdd(q, ok ? v : 0.f);
    };
    if (n <= 0) return;
    get_tile(0);
    if (n > 1) get_tile(1);
    if (n > 1) dma_wait<NREQ>();                                // tile 0 has landed (tile 1 may be in flight)
    else dma_wait<0>();
    __syncthreads();                                            // (also the zeroing of ldspart)
    for (int c = 0; c < n; ++c) {
        const int pbuf = c & 1;
        if (c + 2 < n) get_tile(c + 2);
        if (active) {
            const unsigned char *in = lin[wv][c % RING];
            const float *bet = reinterpret_cast<const float *>(in);           // [s][16 px]
            const float *gam = reinterpret_cast<const float *>(in + 1024);

            const u32x4 Fh = *reinterpret_cast<const u32x4 *>(in + 2048 + lane * 16),
                        Fm = *reinterpret_cast<const u32x4 *>(in + 3072 + lane * 16);
            float itp[4] = {1.f, 1.f, 1.f, 1.f};                              // F16: 1 / t of the pixels 4 g + r of the tile
            if constexpr (F16) {
                const float4 q4 = *reinterpret_cast<const float4 *>(in + 4096 + 16 * g);
                itp[0] = q4.x; itp[1] = q4.y; itp[2] = q4.z; itp[3] = q4.w;
            }

            float *part = ldspart[pbuf][wv];
            __builtin_amdgcn_s_setprio(2);          // (around the products of a tile: c5 pass 2 3.11 / 3.18 -> 3.08 / 3.14 ms, same box)
            unsigned h0, m0, l0, h1, m1, l1;
            split2(gam[(4 * g + 0) * 16 + lo], gam[(4 * g + 1) * 16 + lo], h0, m0, l0);
            split2(gam[(4 * g + 2) * 16 + lo], gam[(4 * g + 3) * 16 + lo], h1, m1, l1);
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 gterm = xdl16_6(u32x2{h0, h1}, u32x2{m0, m1}, u32x2{l0, l1}, ph, pm, pl, zero);
            f32x4 acc = F16 ? zero : gterm;
            const float4 *brow = reinterpret_cast<const float4 *>(bet) + g;          // beta[s][px = 4g .. 4g + 3]
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                f32x4 G;
                if constexpr (F16) {
                    G = xdl3h(Fh, Fm, Zh[s], Zm[s], zero);
                    const float4 bq = brow[s * 4];
                    const float z = iz[s];
                    acc[0] = fmaf(bq.x * z, G[0], acc[0]);
                    acc[1] = fmaf(bq.y * z, G[1], acc[1]);
                    acc[2] = fmaf(bq.z * z, G[2], acc[2]);
                    acc[3] = fmaf(bq.w * z, G[3], acc[3]);
                    continue;
                } else {
                    G = xdl(Fm, Zh[s], zero);
                    if (TERMS >= 4) G = xdl(Fm, Zm[s], G);
                    G = xdl(Fh, Zm[s], G);
                    G = xdl(Fh, Zh[s], G);
                }
                const float4 bq = brow[s * 4];
                acc[0] = fmaf(bq.x, G[0], acc[0]);
                acc[1] = fmaf(bq.y, G[1], acc[1]);
                acc[2] = fmaf(bq.z, G[2], acc[2]);
                acc[3] = fmaf(bq.w, G[3], acc[3]);
            }
            if constexpr (F16) {                   // 1 / t of the row's pixel, then the (unscaled) gamma term
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[rr] = fmaf(acc[rr], itp[rr], gterm[rr]);
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) part[(4 * g + rr) * 16 + lo] = acc[rr];
            __builtin_amdgcn_s_setprio(0);
        }
        // The wave's inputs of tile c + 1 must have landed before it goes round; behind them in its queue are the
        // flush of tile c - 1 and the requests of tile c + 2, which stay in flight.
        if (c + 1 < n) dma_wait_n((c + 2 < n ? NREQ : 0) + (c >= 1 ? 1 : 0));
        step_barrier();
        flush(tile_of(c), ldspart[pbuf]);          // ldspart[pbuf] is rewritten two tiles later, behind the next barrier
    }
}
