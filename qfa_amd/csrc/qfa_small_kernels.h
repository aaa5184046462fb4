// qfa_small_kernels.h -- normalisation, optimiser, parameter maintenance and public helper kernels.
#pragma once
#include "qfa_common.h"

// ------------------------------------------------------------------------------------------------
// k_finalize : grad = sum / count, elementwise, 0/0 = NaN (QFA/model.py:104); loss = sum NLL / B.
// The buffer's scalar slot 6 selects the semantics (include/qfa_hip.h, QFA_F_EXACT_GRAD): 0 = the reference's (above);
// = slot 5 (every launch in exact mode) = the gradient of sum NLL / B: gF = -accF, everything divided by B = slot 5;
// anything else (launches of both modes in one buffer) = NaN in the loss and in every gradient.
// ------------------------------------------------------------------------------------------------
enum { GMODE_REF = 0, GMODE_EXACT = 1, GMODE_MIXED = 2 };
__device__ __forceinline__ int grad_mode(const float *accS) {
    return accS[6] == 0.f ? GMODE_REF : (accS[6] == accS[5] ? GMODE_EXACT : GMODE_MIXED);
}

__global__ void k_finalize(const float *__restrict__ accum, const float *__restrict__ F, int Npix, int Nb, int Nh,
                           int normalize, float *__restrict__ gF, float *__restrict__ gPsi, float *__restrict__ gOm,
                           float *__restrict__ gTau0, float *__restrict__ gC0, float *__restrict__ gBeta,
                           float *__restrict__ loss) {
    const float *accF = accum;
    const float *accA = accF + (size_t)Npix * Nh;
    const float *accPsi = accA + Npix;
    const float *accOm = accPsi + Npix;
    const float *accCnt = accOm + Nb;
    const float *accS = accCnt + Npix;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int mode = grad_mode(accS);
    if (mode != GMODE_REF) {
        const float nan = __builtin_nanf("");
        const float ok = mode == GMODE_EXACT ? 1.f : nan;             // (x * NaN = NaN for every x)
        const float n = normalize ? accS[5] : 1.f;
        if (idx < (size_t)Npix * Nh) gF[idx] = ok * (-accF[idx] / n);
        if (idx < (size_t)Npix) gPsi[idx] = ok * (accPsi[idx] / n);
        if (idx < (size_t)Nb) gOm[idx] = ok * (accOm[idx] / n);
        if (idx == 0) {
            *gTau0 = ok * (accS[0] / n);
            *gC0 = ok * (accS[1] / n);
            *gBeta = ok * (accS[2] / n);
            *loss = ok * (normalize ? accS[4] / accS[5] : accS[4]);
        }
        return;
    }
    if (idx < (size_t)Npix * Nh) {
        const int i = (int)(idx / Nh);
        const float v = F[idx] * accA[i] - accF[idx];
        gF[idx] = normalize ? v / accCnt[i] : v;
    }
    if (idx < (size_t)Npix) gPsi[idx] = normalize ? accPsi[idx] / accCnt[idx] : accPsi[idx];
    if (idx < (size_t)Nb) gOm[idx] = normalize ? accOm[idx] / accCnt[idx] : accOm[idx];
    if (idx == 0) {
        const float cs = normalize ? accS[3] : 1.f;
        *gTau0 = accS[0] / cs;
        *gC0 = accS[1] / cs;
        *gBeta = accS[2] / cs;
        *loss = normalize ? accS[4] / accS[5] : accS[4];
    }
}

// ------------------------------------------------------------------------------------------------
// k_adam_clip : Adam.update + clip for one tensor (QFA/optimizer.py:47-52, QFA/model.py:237-241)
// ------------------------------------------------------------------------------------------------
// The update of one element, shared by the three kernels below so that they cannot drift apart (include/qfa_hip.h promises
// "same arithmetic").  Where v / bc2 overflows float32 although v is finite (|g| beyond ~1e18 early in training) the root is
// formed as sqrt(v) / sqrt(bc2): the reference's float32 gives inf there and stops moving the element; every other input
// keeps the reference's operations and roundings.
__device__ __forceinline__ float adam_clip_update(float pi, float g, float *__restrict__ m, float *__restrict__ v, float lr,
                                                  float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1,
                                                  float bc2, float lo, float hi) {
    const float gi = g + wd * pi;
    const float mi = omb1 * gi + b1 * *m;
    const float vi = omb2 * gi * gi + b2 * *v;
    *m = mi;
    *v = vi;
    const float vh = vi / bc2;
    float root = __fsqrt_rn(vh);
    if (vh == __builtin_inff() && vi < __builtin_inff()) root = __fsqrt_rn(vi) / __fsqrt_rn(bc2);
    float q = pi - lr * (mi / bc1) / (root + eps);
    if (lo <= hi) q = q < lo ? lo : (q > hi ? hi : q);   // NaN stays NaN, like torch.clip
    return q;
}

__global__ void k_adam_clip(const float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                            float *__restrict__ v, float *__restrict__ pout, size_t n, float lr, float b1, float b2,
                            float omb1, float omb2, float eps, float wd, float bc1, float bc2, float lo, float hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pout[i] = adam_clip_update(p[i], g[i], m + i, v + i, lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2, lo, hi);
}

// all parameter tensors in one launch: block b works on tensor k with blk0[k] <= b < blk0[k+1]
struct AdamMultiArgs {
    qfa_adam_multi_t t;
    unsigned blk0[QFA_ADAM_MAX + 1];
};
__global__ void k_adam_clip_multi(AdamMultiArgs a, float lr, float b1, float b2, float omb1, float omb2, float eps,
                                  float wd, float bc1, float bc2) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < QFA_ADAM_MAX; ++j)
        if (j < a.t.count && blockIdx.x >= a.blk0[j]) k = j;
    const size_t i = (size_t)(blockIdx.x - a.blk0[k]) * blockDim.x + threadIdx.x;
    if (i >= a.t.n[k]) return;
    a.t.p_out[k][i] = adam_clip_update(a.t.p[k][i], a.t.g[k][i], a.t.m[k] + i, a.t.v[k] + i, lr, b1, b2, omb1, omb2, eps, wd,
                                       bc1, bc2, a.t.lo[k], a.t.hi[k]);
}

// k_finalize + k_adam_clip_multi in ONE launch (the training step never looks at the gradients themselves): block b works on
// parameter tensor k (F, Psi, omega, tau0, c0, beta in this order), forms the normalised gradient of its element from the packed
// buffer exactly as k_finalize does and applies Adam + clip exactly as k_adam_clip_multi does -- the same float32 operations in
// the same order, so the new parameters are bit-identical to the two-launch path.  Block 0 also writes the batch loss.
__global__ void k_finalize_adam(AdamMultiArgs a, const float *__restrict__ accum, int Npix, int Nb, int Nh, float *__restrict__ loss,
                                float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1, float bc2) {
    const float *accF = accum;
    const float *accA = accF + (size_t)Npix * Nh;
    const float *accPsi = accA + Npix;
    const float *accOm = accPsi + Npix;
    const float *accCnt = accOm + Nb;
    const float *accS = accCnt + Npix;
    const int mode = grad_mode(accS);                                     // (k_finalize)
    const float ok = mode == GMODE_MIXED ? __builtin_nanf("") : 1.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss = mode == GMODE_REF ? accS[4] / accS[5] : ok * (accS[4] / accS[5]);
    int k = 0;
#pragma unroll
    for (int j = 1; j < 6; ++j)
        if (blockIdx.x >= a.blk0[j]) k = j;
    const size_t i = (size_t)(blockIdx.x - a.blk0[k]) * blockDim.x + threadIdx.x;
    if (i >= a.t.n[k]) return;
    const float pi = a.t.p[k][i];
    float g;
    if (mode != GMODE_REF) {                                              // exact: the gradient of sum NLL / B
        if (k == 0) g = -accF[i] / accS[5];
        else if (k == 1) g = accPsi[i] / accS[5];
        else if (k == 2) g = accOm[i] / accS[5];
        else g = accS[k - 3] / accS[5];
        g *= ok;
    }
    else if (k == 0) g = (pi * accA[i / Nh] - accF[i]) / accCnt[i / Nh];   // (p[0] is F itself)
    else if (k == 1) g = accPsi[i] / accCnt[i];
    else if (k == 2) g = accOm[i] / accCnt[i];
    else g = accS[k - 3] / accS[3];
    a.t.p_out[k][i] = adam_clip_update(pi, g, a.t.m[k] + i, a.t.v[k] + i, lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2, a.t.lo[k],
                                       a.t.hi[k]);
}

__global__ void k_clip(const float *__restrict__ x, float *__restrict__ y, size_t n, float lo, float hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float q = x[i];
        y[i] = q < lo ? lo : (q > hi ? hi : q);
    }
}

// ------------------------------------------------------------------------------------------------
// k_smooth : edge-aware moving average along axis 0 (QFA/model.py:243-252)
// ------------------------------------------------------------------------------------------------
__global__ void k_smooth(const float *__restrict__ x, float *__restrict__ y, int n, int cols, int half) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * cols) return;
    const int i = (int)(idx / cols), c = (int)(idx % cols);
    const int lo = i - half < 0 ? 0 : i - half;
    const int hi = i + half + 1 > n ? n : i + half + 1;
    float acc = 0.f;
    for (int r = lo; r < hi; ++r) acc += x[(size_t)r * cols + c];
    y[idx] = acc / (float)(hi - lo);
}

// ------------------------------------------------------------------------------------------------
// elementwise optical-depth helpers (QFA/utils.py:57-92, 149-171)
// ------------------------------------------------------------------------------------------------
__global__ void k_tau(const float *__restrict__ z, float *__restrict__ out, size_t n, qfa_tau_t t) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = t.amp * powf((1.0f + z[i]) * t.scale, t.expo) + t.offset;
}
__global__ void k_tauhi(const float *__restrict__ z, const float *tau0, const float *beta, float *__restrict__ out,
                        size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = *tau0 * powf(1.0f + z[i], *beta);
}
__global__ void k_omega_func(const float *__restrict__ z, const float *tau0, const float *beta, const float *c0,
                             float *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float r = 1.0f - *c0 - expf(-(*tau0 * powf(1.0f + z[i], *beta)));
        out[i] = r * r;
    }
}

// ------------------------------------------------------------------------------------------------
// Woodbury utilities for one (n,k) M and (n,) D (QFA/utils.py:12-54): small, generic, fp64 core.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_wood_core(const float *__restrict__ M, const float *__restrict__ D, int n,
                                                    int k, double *__restrict__ core /* k*k + 1 */) {
    extern __shared__ double sh[];   // k*k
    const int t = threadIdx.x;
    if (t < k * k) {
        const int a = t / k, b = t % k;
        double acc = a == b ? 1.0 : 0.0;
        for (int i = 0; i < n; ++i) acc += (double)M[(size_t)i * k + a] * (double)M[(size_t)i * k + b] / (double)D[i];
        sh[t] = acc;
    }
    __syncthreads();
    // sum log D on all threads
    double ld = 0.0;
    for (int i = t; i < n; i += blockDim.x) ld += log((double)D[i]);
    for (int o = 32; o >= 1; o >>= 1) ld += __shfl_xor(ld, o);
    __shared__ double shl[16];
    if ((t & 63) == 0) shl[t >> 6] = ld;
    __syncthreads();
    double logdet = 0.0;
    for (int jj = 0; jj < k; ++jj) {           // in-place Gauss-Jordan, threads over (i, c)
        const double piv = sh[jj * k + jj];
        __syncthreads();
        double nv = 0.0;
        const int i = t / k, c = t % k;
        if (t < k * k) {
            const double ip = 1.0 / piv;
            const double aij = sh[i * k + jj], ajc = sh[jj * k + c];
            if (i == jj) nv = (c == jj) ? ip : ajc * ip;
            else nv = (c == jj) ? -aij * ip : sh[t] - aij * ajc * ip;
        }
        logdet += log(piv);
        __syncthreads();
        if (t < k * k) sh[t] = nv;
        __syncthreads();
    }
    if (t < k * k) core[t] = sh[t];
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += shl[i];
        core[k * k] = s + logdet;
    }
}

__global__ void k_wood_inv(const float *__restrict__ M, const float *__restrict__ D, int n, int k,
                           const double *__restrict__ core, float *__restrict__ inv, float *__restrict__ logdet) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0 && logdet) *logdet = (float)core[k * k];
    if (!inv || idx >= (size_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    double acc = 0.0;
    for (int a = 0; a < k; ++a) {
        double t = 0.0;
        for (int b = 0; b < k; ++b) t += core[a * k + b] * (double)M[(size_t)j * k + b];
        acc += (double)M[(size_t)i * k + a] * t;
    }
    const double di = 1.0 / (double)D[i], dj = 1.0 / (double)D[j];
    inv[idx] = (float)((i == j ? di : 0.0) - di * acc * dj);
}


// ------------------------------------------------------------------------------------------------
// qfa_zabs_factor_f32 (ABI v4): is a caller's zabs (B, Nb) of the form the reference's loader builds,
//   1 + zabs[s][i] = (1 + z_qso[s]) wav_i / 1215.67   (QFA/dataloader.py:102)?
// k_zfactor_derive takes the two factors from row 0 and column 0 (float64 quotient, one rounding each):
//   zq1[s] = 1 + zabs[s][0],   ratio[i] = (1 + zabs[0][i]) / (1 + zabs[0][0])
// k_zfactor_check counts the elements with |(1 + zabs[s][i]) - zq1[s] ratio[i]| > tol (1 + zabs[s][i]); a NaN counts.
// With nbad == 0 the factored-z kernels see every 1 + z within `tol` (a few float32 ulp) of what the zabs kernels would read.
// ------------------------------------------------------------------------------------------------
__global__ void k_zfactor_derive(const float *__restrict__ zabs, int B, int Nb, float *__restrict__ zq1, float *__restrict__ ratio,
                                 unsigned *__restrict__ nbad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *nbad = 0u;
    if (i < B) zq1[i] = 1.0f + zabs[(size_t)i * Nb];
    if (i < Nb) ratio[i] = (float)((1.0 + (double)zabs[i]) / (1.0 + (double)zabs[0]));
}
__global__ __launch_bounds__(256) void k_zfactor_check(const float *__restrict__ zabs, int B, int Nb, const float *__restrict__ zq1,
                                                       const float *__restrict__ ratio, float tol, unsigned *__restrict__ nbad) {
    // block = groups of 8 spectra x a strip of pixels; grid.y is clamped to 65 535, a block takes every gridDim.y-th group
    unsigned bad = 0u;
    for (int s0 = blockIdx.y * 8; s0 < B; s0 += gridDim.y * 8) {
        for (int r = 0; r < 8; ++r) {
            const int s = s0 + r;
            if (s >= B) break;
            const float zq = zq1[s];
            const float *row = zabs + (size_t)s * Nb;
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Nb; i += gridDim.x * blockDim.x) {
                const float a = 1.0f + row[i], d = a - zq * ratio[i];
                if (!(fabsf(d) <= tol * a)) ++bad;
            }
        }
    }
    for (int o = 32; o >= 1; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(nbad, bad);
}
