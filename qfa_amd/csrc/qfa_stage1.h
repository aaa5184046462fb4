// qfa_stage1.h -- the "role A" lane layout of the XDL kernels and what is built on it, defined once for k_grads_x
// (qfa_grads_x.h), k_s12_x / k_predict_x32 (qfa_s12_x.h) and k_predict_x (qfa_predict_x.h).
//
// A wave holds 16 spectra.  Lane (lo = lane & 15, g = lane >> 4) owns the spectra 4 g + r (r = 0..3) at the pixels
// 32 t + 2 lo + h of half h of tile t.  Stage 1 contracts A = [y | C^-1'] (the writers: [hmean | hcov']) of the wave's
// spectra against the tile image B = [F^T | pair products]; both operands are TWO float16 pieces, three
// v_mfma_f32_16x16x32_f16 per K-step (qfa_common.h "float16 pieces"):
//   image     B[k = 32 ks + 8 g + j][px = 2 lo + h] = t F[px][k] (ks = 0) or t^2 F[px][a_q] F[px][b_q] of the pair
//             q = 32 (ks - 1) + 8 g + j, t the pixel's power of two; per (half, K-step) two 1-KiB pieces [lane][8 k];
//   operand   row lo of the wave: SOL[k] (ks = 0) or SOL[SOL_CI + q], scaled by one power of two per part (S1Op).
// Here: the layout constants (S1Layout), the image builder (s1_image, s1_params), the operand (s1_operand), the lane's
// pixel parameters (S2Pix) and the per-pixel sums of a wave (wave_pixel_sums).  The quarter ring of N_h = 17..32 is in
// qfa_s12_x.h.
#pragma once
#include "qfa_common.h"
#include "qfa_xdl_kernels.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int KP_>
struct S1Layout {
    static constexpr int KP = KP_, KK2 = KP * (KP + 1) / 2;
    static constexpr int NKS = 1 + (KK2 + 31) / 32;      // K-steps: [y, 0 | pair products, 32 per step]: 3 / 6 / 18 at KP = 8 / 16 / 32
    static constexpr int NP = 2;                         // pieces per K-step (float16 h, m; A/B against three bf16 pieces: profiles/r5_ab_f16_*.txt)
    static constexpr int KS_B = NP * 1024;
    // the parameter KiB of a 16-pixel half (GXT, S12): float PAR_x + lo belongs to pixel 2 lo + h
    static constexpr int PAR_PSI = 0, PAR_OM = 16;       // Psi (the writer of N_h = 17..32: mu), omega
    static constexpr int PAR_TI = 32, PAR_PWI = 48, PAR_L2I = 64;      // factored-z form: ti | pwi | l2i (qfa_common.h, ZPSrc)
    static constexpr int PAR_IT1 = 80, PAR_IT2 = 96;     // 1 / t, 1 / t^2
    // staging of a wave's spectra of one tile (k_grads_x, k_s12_x)
    static constexpr int STG_ARR = 16 * 128;             // one array of one tile, [16 rows][32 px] float
    static constexpr int STG_MASK = 3 * STG_ARR;         // mask bytes [16 rows][32 px]
    static constexpr int STG_B = 3 * STG_ARR + 512;      // delta | sigma | zabs | mask (6.5 KiB per wave and tile)
};

// 4-byte aligned 8-byte non-temporal store (cont / unc of the writers are never read back by the call: writer at c3
// 0.87 - 0.91 -> 0.82 ms, same box)
typedef float f32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ void store2_nt(float *dst, float a, float b) {
    __builtin_nontemporal_store(f32x2a4{a, b}, reinterpret_cast<f32x2a4 *>(dst));
}

// ------------------------------------------------------------------------------------------------
// The image builder: one block of 256 threads per 32-pixel tile.
// ------------------------------------------------------------------------------------------------
template <int FS>
struct S1Tile {                      // in LDS: F of the tile (rows of FS floats, FS - 1 columns loaded) and per pixel t, 1 / t, 1 / t^2
    float f[32][FS];
    float tsc[32][3];
};
__device__ __forceinline__ void s1_no_hook(int, int, int, u32x4 &) {}
// dst(h, ks): where the two pieces of K-step ks of half h go (piece m 1 KiB behind piece h); hook(ks, g, px, ph): applied
// to the h piece in front of its store
template <int KP, int FS, class Dst, class Hook>
__device__ __forceinline__ void s1_image(S1Tile<FS> &T, const float *__restrict__ F, int p0, int Npix, int Nh, Dst dst, Hook hook) {
    using L = S1Layout<KP>;
    constexpr int NA = FS - 1;
    for (int i = threadIdx.x; i < 32 * NA; i += 256) {
        const int px = i / NA, a = i % NA;
        T.f[px][a] = (p0 + px < Npix && a < Nh) ? F[(size_t)(p0 + px) * Nh + a] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        float mx = 0.f;
        for (int a = 0; a < KP; ++a) mx = fmaxf(mx, fabsf(T.f[threadIdx.x][a]));
        int e = 7;
        if (mx > 0.f && mx < 3.0e38f) (void)frexpf(mx, &e);       // t f_a in [2^6, 2^7) for the largest: pairs below 2^14
        e = e < -50 ? -50 : (e > 60 ? 60 : e);
        T.tsc[threadIdx.x][0] = ldexpf(1.f, 7 - e);
        T.tsc[threadIdx.x][1] = ldexpf(1.f, e - 7);
        T.tsc[threadIdx.x][2] = ldexpf(1.f, 2 * (e - 7));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * L::NKS * 64; i += 256) {
        const int lane = i & 63, ks = (i >> 6) % L::NKS, h = i / (64 * L::NKS);
        const int lo = lane & 15, g = lane >> 4, px = 2 * lo + h;
        const float t1 = T.tsc[px][0], t2 = t1 * t1;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 8 * g + j;
            float x = 0.f;
            if (ks == 0) {
                if (kk < KP) x = T.f[px][kk] * t1;
            } else {
                const int q = 32 * (ks - 1) + kk;
                if (q < L::KK2) {
                    int a = 0;
                    while (a + 1 < KP && pair_index(a + 1, a + 1, KP) <= q) ++a;
                    const int b = a + (q - pair_index(a, a, KP));
                    x = T.f[px][a] * T.f[px][b] * t2;
                }
            }
            v[j] = x;
        }
        unsigned char *d = dst(h, ks) + lane * 16;
        u32x4 ph, pm;
        split8h(v, ph, pm);
        hook(ks, g, px, ph);
        *reinterpret_cast<u32x4 *>(d) = ph;
        *reinterpret_cast<u32x4 *>(d + 1024) = pm;
    }
}
// the parameter KiB of both halves (S1Layout::PAR_*, zero padded) to po(h)
template <int KP, int FS, class Po>
__device__ __forceinline__ void s1_params(const S1Tile<FS> &T, int p0, const float *__restrict__ Psi, const float *__restrict__ omega,
                                          const ZPSrc &ZP, int Npix, int Nb, Po po) {
    using L = S1Layout<KP>;
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int h = i >> 8, j = i & 255;
        const int px = p0 + 2 * (j & 15) + h;
        float v = 0.f;
        if (j < L::PAR_OM) v = px < Npix ? Psi[px] : 0.f;
        else if (j < L::PAR_TI) v = px < Nb ? omega[px] : 0.f;
        else if (j < L::PAR_IT1 && ZP.on() && px < Nb) {
            const float4 q = ZP.at(px);
            v = j < L::PAR_PWI ? q.x : (j < L::PAR_L2I ? q.y : q.z);
        } else if (j >= L::PAR_IT1 && j < L::PAR_IT2 + 16) v = T.tsc[2 * (j & 15) + h][j < L::PAR_IT2 ? 1 : 2];
        po(h)[j] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// The A operand of a wave: the pieces of every K-step of row lo and, for the lane's OUTPUT rows 4 g + r, the inverse
// powers of two of the two parts (K-step 0 | the pair values).
// ------------------------------------------------------------------------------------------------
template <int KP>
struct S1Op {
    u32x4 h[S1Layout<KP>::NKS], m[S1Layout<KP>::NKS];
    float is0[4], is1[4];
};
// sol: the SOL row of spectrum s0 + lo (any readable row when !v)
template <int KP>
__device__ __forceinline__ void s1_operand(const float *__restrict__ sol, bool v, int g, S1Op<KP> &A) {
    using C = Cfg<KP>;
    using L = S1Layout<KP>;
    float xs[L::NKS][8];                                  // (read once: small batches are latency-bound)
#pragma unroll
    for (int ks = 0; ks < L::NKS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 8 * g + j;
            float val = 0.f;
            if (ks == 0) {
                if (v && kk < KP) val = sol[kk];
            } else {
                const int q = 32 * (ks - 1) + kk;
                if (v && q < L::KK2) val = sol[C::SOL_CI + q];
            }
            xs[ks][j] = val;
        }
    float m0 = 0.f, m1 = 0.f;
#pragma unroll
    for (int ks = 0; ks < L::NKS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (ks == 0) m0 = fmaxf(m0, fabsf(xs[ks][j])); else m1 = fmaxf(m1, fabsf(xs[ks][j]));
        }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) { m0 = fmaxf(m0, __shfl_xor(m0, o)); m1 = fmaxf(m1, __shfl_xor(m1, o)); }
    float i0, i1;
    const float sc0 = f16_row_scale(m0, i0), sc1 = f16_row_scale(m1, i1);
#pragma unroll
    for (int r = 0; r < 4; ++r) { A.is0[r] = __shfl(i0, 4 * g + r); A.is1[r] = __shfl(i1, 4 * g + r); }
#pragma unroll
    for (int ks = 0; ks < L::NKS; ++ks) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = xs[ks][j] * (ks == 0 ? sc0 : sc1);
        split8h(x, A.h[ks], A.m[ks]);
    }
}

// ------------------------------------------------------------------------------------------------
// What the staging and stage 2 of k_grads_x and k_s12_x share.  Stage 2 of an element and the copy-out of a staged tile
// stay written out in both kernels: with either in a shared function (the copy-out: on k_grads_x's float pairs) hipcc
// contracts and packs the element arithmetic of k_s12_x or of both differently, and the gradients change in their last bits.
// ------------------------------------------------------------------------------------------------
// staging slot q of an array holds row q ^ ((q >> 2) & 1): the four rows 4 g + r that one ds_read_b64 of take_tile touches
// then alternate between the two halves of the banks (2-way = the minimum for 512 bytes)
__device__ __forceinline__ unsigned slot_row(int q, int last_row) { return (unsigned)min(q ^ ((q >> 2) & 1), last_row); }
struct S2Pix {                       // the lane's pixel: Psi, omega and the factored-z per-pixel factors (parameter KiB)
    float Psi, om, ti, pwi, l2i;
};
// per-pixel sums over the wave's 16 spectra (lanes lo + 16 g'): v_permlane16_swap / v_permlane32_swap -- three exchanges
// and three adds leave the sum of quantity g (sumA | gPsi | gOmega | cnt) over the four 16-lane rows in row g
__device__ __forceinline__ float wave_pixel_sums(float sA, float gPsi, float gOm, float cnt) {
    const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(sA), __float_as_uint(gPsi), false, false);
    const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(gOm), __float_as_uint(cnt), false, false);
    const float u01 = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);   // rows: sA(0+1) gPsi(0+1) sA(2+3) gPsi(2+3)
    const float u23 = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);   //       gOm     cnt       gOm     cnt
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(u01), __float_as_uint(u23), false, false);
    // t[0] rows: sA(0+1) gPsi(0+1) gOm(0+1) cnt(0+1);  t[1] rows: sA(2+3) gPsi(2+3) gOm(2+3) cnt(2+3)
    return __uint_as_float(t[0]) + __uint_as_float(t[1]);
}
