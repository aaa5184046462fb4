// qfa_sample.h -- posterior draws: latent vectors h ~ N(hmean, hcov) and continua mu + F h (include/qfa_hip.h,
// qfa_sample_latent_f32 / qfa_continua_f32).  Built in qfa_sample.hip.
//
//   k_sample_image   F (Npix, Nh) row-major -> image (Nh + 1, pad): row j = F[:, j], row Nh = mu  (coalesced per-lane loads)
//   k_sample_latent  one wave per (spectrum, chunk of samples): float64 Cholesky of hcov in LDS, Philox4x32-10 + Box-Muller
//                    in registers, h = hmean + C z in float64, rounded once
//   k_sample_cont    the writer: a lane owns one pixel (its Nh + 1 image values in registers) and walks a run of latent rows;
//                    the row's h is wave-uniform (scalar loads), one fmaf chain per output, one dword store per lane
//
// The draw contract (what every port must reproduce) is spelled out in include/qfa_hip.h above qfa_sample_latent_f32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfa_sample {

constexpr int kWriterThreads = 256;       // k_sample_cont: 4 waves on 256 consecutive pixels of the same rows
constexpr int kLatentThreads = 64;        // k_sample_latent: one wave

// Philox4x32-10 (Salmon et al., SC'11; the constants and round structure of Random123's philox4x32_10)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// four standard normals of counter (q, s, r_lo, r_hi): uniforms (x + 0.5) 2^-32 in (0, 1), Box-Muller in float64,
// each rounded once to float32
__device__ __forceinline__ void normals4(uint32_t q, uint32_t s, uint64_t r, uint32_t k0, uint32_t k1, float z[4]) {
    uint32_t c[4] = {q, s, (uint32_t)r, (uint32_t)(r >> 32)};
    philox4x32_10(c, k0, k1);
    const double sc = 2.3283064365386963e-10;            // 2^-32
    const double twopi = 6.283185307179586;              // (double)(2 pi)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double u0 = ((double)c[2 * h] + 0.5) * sc, u1 = ((double)c[2 * h + 1] + 0.5) * sc;
        const double rad = sqrt(-2.0 * log(u0));
        const double t = twopi * u1;
        z[2 * h] = (float)(rad * cos(t));
        z[2 * h + 1] = (float)(rad * sin(t));
    }
}

__global__ void k_sample_image(const float *__restrict__ F, const float *__restrict__ mu, int Npix, int Nh, int pad,
                               float *__restrict__ img) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)(Nh + 1) * pad) return;
    const int j = (int)(i / pad), p = (int)(i % pad);
    float v = 0.f;
    if (p < Npix) v = j < Nh ? F[(int64_t)p * Nh + j] : mu[p];
    img[i] = v;
}

// grid (B, chunks): block (b, c) draws samples [c spb, min(S, (c + 1) spb)) of spectrum b.  NHM >= Nh (8, 16 or 32).
template <int NHM>
__global__ __launch_bounds__(kLatentThreads) void k_sample_latent(const float *__restrict__ hmean, const float *__restrict__ hcov,
                                                                  int Nh, int S, int spb, uint32_t k0, uint32_t k1, int64_t row0,
                                                                  float *__restrict__ h) {
    __shared__ double L[NHM * NHM];                       // lower triangle, row-major with stride NHM
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *A = hcov + (int64_t)b * Nh * Nh;
    const float *m = hmean + (int64_t)b * Nh;
    bool bad = false;
    for (int e = lane; e < Nh * Nh; e += kLatentThreads) bad |= !isfinite(A[e]);
    // the whole NHM x NHM array: zeros above the diagonal and outside Nh x Nh, so that the mat-vec below runs over NHM columns
    for (int e = lane; e < NHM * NHM; e += kLatentThreads) {
        const int i = e / NHM, j = e % NHM;
        L[e] = (i < Nh && j <= i) ? (double)A[i * Nh + j] : 0.0;
    }
    for (int j = lane; j < Nh; j += kLatentThreads) bad |= !isfinite(m[j]);
    bad = __ballot(bad) != 0;                             // one wave: the vote covers the whole spectrum
    __syncthreads();
    // right-looking Cholesky; a pivot <= 0 zeroes its column (near-singular hcov of high-S/N spectra)
    for (int k = 0; k < Nh; ++k) {
        const double piv = L[k * NHM + k];
        const double d = piv > 0.0 ? sqrt(piv) : 0.0;
        const double inv = piv > 0.0 ? 1.0 / d : 0.0;
        __syncthreads();
        for (int i = k + 1 + lane; i < Nh; i += kLatentThreads) L[i * NHM + k] *= inv;
        if (lane == 0) L[k * NHM + k] = d;
        __syncthreads();
        const int n = Nh - k - 1;
        for (int e = lane; e < n * n; e += kLatentThreads) {
            const int i = k + 1 + e / n, j = k + 1 + e % n;
            if (j <= i) L[i * NHM + j] -= L[i * NHM + k] * L[j * NHM + k];
        }
        __syncthreads();
    }
    const uint64_t r = (uint64_t)(row0 + b);
    const int s1 = min(S, (int)(((int64_t)blockIdx.y + 1) * spb));
    for (int s = blockIdx.y * spb + lane; s < s1; s += kLatentThreads) {
        float z[NHM];
#pragma unroll
        for (int q = 0; q < NHM / 4; ++q) {
            if (4 * q < Nh) {
                normals4((uint32_t)q, (uint32_t)s, r, k0, k1, z + 4 * q);
            } else {
                z[4 * q] = z[4 * q + 1] = z[4 * q + 2] = z[4 * q + 3] = 0.f;
            }
        }
        float *o = h + ((int64_t)b * S + s) * Nh;
        // row i of L is wave-uniform (LDS broadcast); columns past i are zero, so the full-width sum is the triangular one
        for (int i = 0; i < Nh; ++i) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < NHM; ++j) y += L[i * NHM + j] * (double)z[j];
            o[i] = bad ? __builtin_nanf("") : (float)((double)m[i] + y);
        }
    }
}

// grid (strips * row_chunks): block x = chunk * strips + strip, so that the blocks that write the same rows are dispatched
// together and the 128-byte lines two strips share are completed in L2 at about the same time.
template <int NH>
__global__ __launch_bounds__(kWriterThreads) void k_sample_cont(const float *__restrict__ img, int pad,
                                                                const float *__restrict__ h, int64_t R, int Npix, int strips,
                                                                int64_t rows_per_block, float *__restrict__ out) {
    const int strip = blockIdx.x % strips;
    const int64_t chunk = blockIdx.x / strips;
    const int p = strip * kWriterThreads + threadIdx.x;
    if (strip * kWriterThreads + (int)(threadIdx.x & ~63u) >= Npix) return;   // a wave with no pixel of the row
    const int64_t r0 = chunk * rows_per_block;
    const int64_t r1 = min(R, r0 + rows_per_block);
    float f[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) f[j] = img[(int64_t)j * pad + p];        // p < pad: the image rows are padded to 256
    const float m = img[(int64_t)NH * pad + p];
    const bool live = p < Npix;
    // retire the image loads here (vmcnt(0); expcnt, lgkmcnt untouched): the compiler's own wait for them would sit at the
    // head of the row loop -- under the `live` branch it cannot prove taken -- and there also wait for the previous step's stores
    __builtin_amdgcn_s_waitcnt(0x0F70);
    float *o = out + r0 * Npix + p;
    const float *hr = h + r0 * NH;
    // U rows per step: their U * NH latent values are loaded (scalar loads, <= 64 registers) before the first fma, so that one
    // wait covers U rows
    constexpr int U = NH >= 32 ? 2 : (NH > 8 ? 64 / NH : 8);
    int64_t r = r0;
    for (; r + U <= r1; r += U) {
        float hv[U * NH];
#pragma unroll
        for (int k = 0; k < U * NH; ++k) hv[k] = hr[k];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = m;
#pragma unroll
            for (int j = 0; j < NH; ++j) acc = fmaf(f[j], hv[u * NH + j], acc);
            if (live) o[(int64_t)u * Npix] = acc;
        }
        o += (int64_t)U * Npix;
        hr += U * NH;
    }
    for (; r < r1; ++r) {
        float acc = m;
#pragma unroll
        for (int j = 0; j < NH; ++j) acc = fmaf(f[j], hr[j], acc);
        if (live) *o = acc;
        o += Npix;
        hr += NH;
    }
}

}  // namespace qfa_sample
