// qfa_dla.h -- the DLA finder: the table of DLA transmission templates and the likelihood-ratio scan of a batch of spectra over a
// table of templates (include/qfa_hip.h: qfa_dla_profiles_f32, qfa_template_scan_f32 state the rule).  Built in
// qfa_dla.hip.
//
//   k_dla_profiles  one thread per element V[c, k] of the table, float64 (qfa_voigt.h: k_absorber's profile), rounded once
//   k_scan_pf       the pixel image PF[k][16 ntl]: the pair products f_a f_b (a <= b) in 16-column tiles, then the columns f_a;
//                   rows padded to a multiple of 16 pixels (zeros)
//   k_scan_vt       the template table transposed and padded, VT[k][ncp] (pads = 1.0f), so that the 16 candidates of a tile lie
//                   side by side; k_scan_flags: one byte per (candidate tile, 16-pixel block), 0 = every template is 1.0f there
//   k_scan_prep     per spectrum and pixel, float32: A, G = A^2 Psi + omega zd, sigma^2, x, A mu, the three null terms w A^2,
//                   w A delta, w delta^2, G w, ln D and the mask -- eleven rows of Npad floats.  A masked pixel is stored as A = G =
//                   x = A mu = 0, sigma^2 = 1: every term of every candidate is then an exact 0 without a mask in the hot loop
//   k_scan_null     the null moments C0 - I, b0, sum w delta^2, sum ln D, n of a spectrum: float64 sums of the float32 terms in a
//                   fixed order (one workgroup per spectrum);  b0^T y0, log det C0 and NLL0: k_scan_solve's null pass
//   k_template_scan the hot path.  A wave owns 16 candidates x one spectrum; the four waves of a workgroup take four spectra of the
//                   same candidate tile, so its VT and PF lines are fetched once per group and shared in the cache.  Lane (lo, g)
//                   forms the three differences d1, d2, d3 of candidate lo at pixel 4 j + g on the VALU (scan_terms at V minus
//                   scan_terms at 1, which the prep kernel stored: V == 1.0f gives exact zeros) and feeds d1 / d2 as the A operand
//                   of v_mfma_f32_16x16x4_f32 against the PF tiles; d3 is summed per lane in float64.  Blocks of 16 pixels whose
//                   flag is 0 are skipped.  The moments of a candidate leave as one row of MOM
//   k_scan_solve    one wave per (spectrum, candidate): C0 + dC in float64 in LDS (k_em_solve_f's Cholesky), the forward solve, llr
//   k_scan_best     the arg-max of a spectrum's row: a maximum with the lower index on ties, so any order gives the same answer
//   No atomics, no scratch; LDS: 4 x 32 x 33 doubles in k_scan_solve, 2 KiB in k_scan_null and in k_scan_best.
#pragma once
#include "qfa_common.h"
#include "qfa_voigt.h"

namespace qfa_dla {

__host__ __device__ inline int npairs(int Nh) { return Nh * (Nh + 1) / 2; }
__host__ __device__ inline int pair_tiles(int Nh) { return (npairs(Nh) + 15) / 16; }
__host__ __device__ inline int f_tiles(int Nh) { return (Nh + 15) / 16; }
__host__ __device__ inline int pf_cols(int Nh) { return 16 * (pair_tiles(Nh) + f_tiles(Nh)); }
__host__ __device__ inline int mom_cols(int Nh) { return pf_cols(Nh) + 2; }          // + the float64 sum of d3 as two floats
__host__ __device__ inline int null_cols(int Nh) { return pf_cols(Nh) + 3; }         // + sum w delta^2, sum ln D, n

// rows of the per-spectrum record (Npad floats each)
enum { R_A = 0, R_G, R_S2, R_X, R_AM, R_N1, R_N2, R_N3, R_GW, R_LD, R_M, R_ROWS };

// ------------------------------------------------------------------------------------------------
// k_dla_profiles: V[c = i nN + j][k], float64 rounded once
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_dla_profiles(const double *__restrict__ grid, int Npix, double lam_hi, double dv_kms,
                                                             int nz, double logn_lo, double dlogn, int nN, double b_kms, int lyb,
                                                             float *__restrict__ V) {
    using namespace qfa_voigt;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nz * nN * Npix) return;
    const int k = (int)(e % (size_t)Npix), c = (int)(e / (size_t)Npix);
    const int i = c / nN, j = c - i * nN;
    const double lam_i = lam_hi * exp(-(double)i * dv_kms / kC);
    const double lg = logn_lo + (double)j * dlogn;
    const double cb = kC / b_kms, g = grid[k];
    double tau = 0.0;
    for (int l = 0; l < (lyb ? 2 : 1); ++l) {
        const double r = 1.0 / (lam_i * (kLam0[l] / kLam0[0]));                    // 1 / (lam0 (1 + z_a)) of a spectrum at rest
        const double x = cb * fma(g, r, -1.0);
        const double P = x * x, rP = 1.0 / P;
        tau += tau_coef(lg, l, b_kms) * h_full(line_ka(l, b_kms), P, rP);
    }
    V[e] = (float)exp(-tau);
}

// ------------------------------------------------------------------------------------------------
// images of the scan
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_scan_pf(const float *__restrict__ F, int Npix, int Npad, int Nh, float *__restrict__ PF) {
    const int ncol = pf_cols(Nh), np = npairs(Nh), fpos = 16 * pair_tiles(Nh);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Npad * ncol) return;
    const int k = (int)(i / ncol), c = (int)(i % ncol);
    float v = 0.f;
    if (k < Npix) {
        const float *f = F + (size_t)k * Nh;
        if (c < np) {
            int a = 0, q = c;
            while (q >= Nh - a) { q -= Nh - a; ++a; }
            v = __fmul_rn(f[a], f[a + q]);
        } else if (c >= fpos && c < fpos + Nh) {
            v = f[c - fpos];
        }
    }
    PF[i] = v;
}

static __global__ __launch_bounds__(256) void k_scan_vt(const float *__restrict__ V, int nc, int ncp, int Npix, int Npad,
                                                        float *__restrict__ VT) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Npad * ncp) return;
    const int k = (int)(i / ncp), c = (int)(i % ncp);
    VT[i] = (k < Npix && c < nc) ? V[(size_t)c * Npix + k] : 1.0f;
}

static __global__ __launch_bounds__(256) void k_scan_flags(const float *__restrict__ VT, int ncp, int Npad, unsigned char *__restrict__ FLAG) {
    const int nkb = Npad / 16, nct = ncp / 16;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nct * nkb) return;
    const int ct = i / nkb, kb = i - ct * nkb;
    bool any = false;
    for (int k = 0; k < 16; ++k)
        for (int c = 0; c < 16; ++c) any |= !(VT[(size_t)(16 * kb + k) * ncp + 16 * ct + c] == 1.0f);      // (a NaN template counts)
    FLAG[i] = any ? 1 : 0;
}

// The three terms of one pixel under the transmission V: w' A'^2, w' A' delta', w' delta'^2 with A' = V A, D' = V^2 G + sigma^2,
// w' = 1 / D', delta' = x - V (A mu).  Every operation is written out and rounded once, so that the value at V = 1 which the prep
// kernel stores and the value the hot loop forms at V == 1.0f are the same bits and their difference is an exact 0.
struct ScanTerms { float t1, t2, t3; };
// (hipcc's __fmul_rn / __fsub_rn are plain operators, and the backend's fast contraction fuses a product and the subtraction behind
// it into an fma that keeps the product's rounding error whatever the source says: the hot loop pins the three products -- pin(),
// qfa_common.h -- before it subtracts the stored ones, else the difference of equal terms would not be 0)
__device__ __forceinline__ ScanTerms scan_terms(float V, float V2, float A, float G, float S2, float x, float AM) {
    const float Ap = __fmul_rn(V, A);
    const float Dp = __fmaf_rn(V2, G, S2);
    const float wp = fast_rcp(Dp);
    const float dp = __fmaf_rn(-V, AM, x);
    const float u = __fmul_rn(wp, Ap), e = __fmul_rn(wp, dp);
    return ScanTerms{__fmul_rn(u, Ap), __fmul_rn(e, Ap), __fmul_rn(e, dp)};
}

// one thread per (spectrum of the chunk, pixel < Npad).  REC [spectrum][R_ROWS][Npad]
static __global__ __launch_bounds__(256) void k_scan_prep(qfa_params_t p, qfa_batch_t bt, qfa_tau_t tau, const float *__restrict__ mu,
                                                          int s0, int nspec, int Npix, int Npad, int Nb, float *__restrict__ REC) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nspec * Npad) return;
    const int sl = (int)(i / Npad), k = (int)(i % Npad), s = s0 + sl;
    float A = 0.f, G = 0.f, S2 = 1.f, x = 0.f, AM = 0.f, LD = 0.f, m = 0.f;
    if (k < Npix) {
        const unsigned long long row = batch_row(bt, s);
        const unsigned long long off = row * (unsigned long long)bt.row_stride + (unsigned)k;
        if (bt.mask[off] != 0) {
            const float fl = bt.delta[off], sg = bt.error[off];
            float Ak = 1.f, om = 0.f;
            if (k < Nb) {
                const DevConsts kc = load_consts(p, tau);
                const float z = bt.zq1 ? __fmaf_rn(bt.zq1[row], bt.pix_ratio[k], -1.0f) : bt.zabs[row * (unsigned long long)Nb + (unsigned)k];
                const BlueTerms bl = blue_terms(z, kc);
                Ak = bl.A;
                om = __fmul_rn(p.omega[k], bl.zd);
            }
            A = Ak;
            G = __fmaf_rn(__fmul_rn(Ak, Ak), p.Psi[k], om);
            S2 = __fmul_rn(sg, sg);
            AM = __fmul_rn(Ak, mu[k]);
            const bool fin = fl - fl == 0.f && sg - sg == 0.f;                     // a non-finite value in a used pixel poisons the spectrum
            x = fin ? fl : __int_as_float(0x7fc00000);
            if (!fin) S2 = 1.f;
            m = 1.f;
        }
    }
    const ScanTerms n = scan_terms(1.0f, 1.0f, A, G, S2, x, AM);
    const float D = __fmaf_rn(1.0f, G, S2), w = fast_rcp(D);
    if (m != 0.f) LD = fast_log(D);
    float *rec = REC + (size_t)sl * R_ROWS * Npad + k;
    rec[(size_t)R_A * Npad] = A;
    rec[(size_t)R_G * Npad] = G;
    rec[(size_t)R_S2 * Npad] = S2;
    rec[(size_t)R_X * Npad] = x;
    rec[(size_t)R_AM * Npad] = AM;
    rec[(size_t)R_N1 * Npad] = n.t1;
    rec[(size_t)R_N2 * Npad] = n.t2;
    rec[(size_t)R_N3 * Npad] = n.t3;
    rec[(size_t)R_GW * Npad] = __fmul_rn(G, w);
    rec[(size_t)R_LD * Npad] = LD;
    rec[(size_t)R_M * Npad] = m;
}

// ------------------------------------------------------------------------------------------------
// k_scan_null: NULLM[spectrum][null_cols] float64 = [sum n1 PF pairs | sum n2 PF f | sum n3 | sum ln D | n].  One workgroup per
// spectrum: thread (col, part) adds the pixels part, part + P, .. in order; the parts are added in order.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_scan_null(const float *__restrict__ REC, const float *__restrict__ PF, int Npad, int Nh,
                                                          double *__restrict__ NULLM) {
    __shared__ double sh[256];
    const int sl = blockIdx.x, tid = threadIdx.x;
    const int pc = pf_cols(Nh), fpos = 16 * pair_tiles(Nh), ncol = pc + 3;
    const int CW = ncol < 256 ? ncol : 256, P = 256 / CW;
    const float *rec = REC + (size_t)sl * R_ROWS * Npad;
    const int cl = tid % CW, part = tid / CW;
    for (int c0 = 0; c0 < ncol; c0 += CW) {
        const int col = c0 + cl;
        double a = 0.0;
        if (part < P && col < ncol) {
            const float *wrow = rec + (size_t)(col < fpos ? R_N1 : col < pc ? R_N2 : col == pc ? R_N3 : col == pc + 1 ? R_LD : R_M) * Npad;
            for (int k = part; k < Npad; k += P) {
                const double g = col < pc ? (double)PF[(size_t)k * pc + col] : 1.0;
                a = fma((double)wrow[k], g, a);
            }
        }
        __syncthreads();
        sh[tid] = a;
        __syncthreads();
        if (tid < CW && col < ncol) {
            double t = 0.0;
            for (int q = 0; q < P; ++q) t += sh[q * CW + tid];
            NULLM[(size_t)sl * ncol + col] = t;
        }
    }
}

// The float64 Cholesky of one wave (k_em_solve_f's): lane r holds row r of the lower triangle in L (row stride 33); on return
// quad = b^T C^-1 b and logdet = log det C; false = a pivot that is not positive and finite.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ bool chol_quad(double *L, int lane, int Nh, double b, double &quad, double &logdet) {
    const bool row = lane < Nh;
    double ld = 0.0;
    for (int j = 0; j < Nh; ++j) {
        const double piv = L[j * 33 + j];                         // the same address for every lane: wave-uniform
        if (!(piv > 0.0) || !(piv < 1.0e300)) return false;
        const double dj = sqrt(piv), idj = 1.0 / dj;
        ld += log(piv);
        double lij = 0.0;
        if (row && lane > j) lij = L[lane * 33 + j] * idj;
        wave_lds_sync();
        if (row && lane > j) L[lane * 33 + j] = lij;
        if (lane == j) L[j * 33 + j] = dj;
        wave_lds_sync();
        if (row && lane > j)
            for (int c = j + 1; c <= lane; ++c) L[lane * 33 + c] -= lij * L[c * 33 + j];
        wave_lds_sync();
    }
    double x = row ? b : 0.0, q = 0.0;
    for (int j = 0; j < Nh; ++j) {                                // L z = b;  b^T C^-1 b = z^T z
        const double zj = __shfl(x, j) / L[j * 33 + j];
        q = fma(zj, zj, q);
        if (row && lane > j) x -= L[lane * 33 + j] * zj;
    }
    quad = q;
    logdet = ld;
    return true;
}

// ------------------------------------------------------------------------------------------------
// k_template_scan.  grid = (candidate tiles, groups of four spectra of the chunk); wave w owns spectrum 4 blockIdx.y + w.
// NTL: tiles of the accumulator array (>= the shape's ntl = pair_tiles + f_tiles).  MOM [spectrum][ncp][mom_cols].
// ------------------------------------------------------------------------------------------------
template <int NTL>
__global__ __launch_bounds__(256) void k_template_scan(const float *__restrict__ REC, const float *__restrict__ PF,
                                                       const float *__restrict__ VT, const unsigned char *__restrict__ FLAG, int nspec,
                                                       int Npad, int Nh, int ncp, float *__restrict__ MOM) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    const int sl = (int)blockIdx.y * 4 + w, ct = blockIdx.x;
    if (sl >= nspec) return;                                      // (whole wave; no block-level synchronisation below)
    const int npt = pair_tiles(Nh), ntl = npt + f_tiles(Nh), pc = 16 * ntl, nkb = Npad / 16;
    const float *rec = REC + (size_t)sl * R_ROWS * Npad;
    const unsigned char *flag = FLAG + (size_t)ct * nkb;
    const float *vt = VT + 16 * ct + lo;

    f32x4 acc[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    double ds = 0.0;
    for (int kb = 0; kb < nkb; ++kb) {
        if (wave_uniform(flag[kb]) == 0) continue;                // every template of the tile is 1.0f on these 16 pixels: exact zeros
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int k = 16 * kb + 4 * j + g;
            const float V = vt[(size_t)k * ncp];
            const float A = rec[R_A * Npad + k], G = rec[R_G * Npad + k], S2 = rec[R_S2 * Npad + k], x = rec[R_X * Npad + k];
            const float AM = rec[R_AM * Npad + k], n1 = rec[R_N1 * Npad + k], n2 = rec[R_N2 * Npad + k], n3 = rec[R_N3 * Npad + k];
            const float GW = rec[R_GW * Npad + k];
            const float V2 = __fmul_rn(V, V);
            ScanTerms t = scan_terms(V, V2, A, G, S2, x, AM);
            pin(t.t1, t.t2, t.t3);
            const float d1 = __fsub_rn(t.t1, n1), d2 = __fsub_rn(t.t2, n2);
            // ln(D' / D) = ln(1 - (1 - V^2) G / D): an exact 0 at V == 1.0f
            const float q = __fmul_rn(__fmaf_rn(-V, V, 1.0f), GW);
            const float d3 = __fadd_rn(__fsub_rn(t.t3, n3), fast_log(__fsub_rn(1.0f, q)));
            ds += (double)d3;
            const float *pf = PF + (size_t)k * pc + lo;
#pragma unroll
            for (int tt = 0; tt < NTL; ++tt)
                if (tt < ntl) acc[tt] = mfma4(tt < npt ? d1 : d2, pf[16 * tt], acc[tt]);
        }
    }
    // d3 of candidate lo: the four pixel phases g in order
    const double s1 = __shfl(ds, lo + 16), s2 = __shfl(ds, lo + 32), s3 = __shfl(ds, lo + 48);
    const double dsum = ((ds + s1) + s2) + s3;                    // (as lane g = 0 sees it)
    const int mc = pc + 2;
    float *mom = MOM + ((size_t)sl * ncp + 16 * ct) * mc;
    // D layout of the MFMA: lane (g, lo), register r = row (candidate) 4 g + r, column lo
#pragma unroll
    for (int tt = 0; tt < NTL; ++tt) {
        if (tt >= ntl) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) mom[(size_t)(4 * g + r) * mc + 16 * tt + lo] = acc[tt][r];
    }
    if (g == 0) {
        const float hi = (float)dsum;
        mom[(size_t)lo * mc + pc] = hi;
        mom[(size_t)lo * mc + pc + 1] = (float)(dsum - (double)hi);
    }
}

// ------------------------------------------------------------------------------------------------
// k_scan_solve: one wave per (spectrum of the chunk, candidate < nc):
//   llr = (-ds + (b'^T y' - b0^T y0) - (log det C' - log det C0)) / 2.
// null_pass != 0: one wave per spectrum, dC = db = 0; writes NUL0[spectrum] = {b0^T y0, log det C0} and
//   nll0 = (sum w delta^2 - b0^T y0 + n log 2 pi + sum ln D + log det C0) / 2.
// One kernel for both, so that a candidate whose differences are all 0 repeats the null's arithmetic instruction for instruction
// and gets llr = 0 exactly.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_scan_solve(const float *__restrict__ MOM, const double *__restrict__ NULLM,
                                                           double *NUL0, int nspec, int nc, int ncp, int Nh, int null_pass,
                                                           float *__restrict__ out) {
    __shared__ double sL[4][32 * 33];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t item = (size_t)blockIdx.x * 4 + w;
    const size_t per = null_pass ? 1 : (size_t)nc;
    if (item >= (size_t)nspec * per) return;                      // (whole wave; waves synchronise with themselves only)
    const int sl = (int)(item / per), c = (int)(item % per);
    double *L = sL[w];
    const int pc = pf_cols(Nh), fpos = 16 * pair_tiles(Nh), ncol = pc + 3, mc = pc + 2;
    const double *nm = NULLM + (size_t)sl * ncol;
    const float *mom = MOM + ((size_t)sl * ncp + c) * mc;
    if (lane < Nh)
        for (int a = 0; a <= lane; ++a) {
            const int pi = pair_index(a, lane, Nh);
            const double dC = null_pass ? 0.0 : (double)mom[pi];
            L[lane * 33 + a] = (nm[pi] + dC) + (a == lane ? 1.0 : 0.0);
        }
    wave_lds_sync();
    double bl = 0.0;
    if (lane < Nh) bl = nm[fpos + lane] + (null_pass ? 0.0 : (double)mom[fpos + lane]);
    double quad, logdet;
    const bool ok = chol_quad(L, lane, Nh, bl, quad, logdet);
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (null_pass) {
            NUL0[2 * (size_t)sl] = ok ? quad : nan;
            NUL0[2 * (size_t)sl + 1] = ok ? logdet : nan;
            out[sl] = ok ? (float)(0.5 * (nm[pc] - quad + nm[pc + 2] * 1.8378770664093453 + nm[pc + 1] + logdet)) : __int_as_float(0x7fc00000);
        } else {
            const double ds = (double)mom[pc] + (double)mom[pc + 1];
            const double v = 0.5 * (-ds + (quad - NUL0[2 * (size_t)sl]) - (logdet - NUL0[2 * (size_t)sl + 1]));
            out[(size_t)sl * nc + c] = ok ? (float)v : __int_as_float(0x7fc00000);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_scan_best: one workgroup per spectrum.  The largest llr, the lowest c among equals; NaN is never taken; none: -1, NaN.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void best_merge(float &v, int &i, float v2, int i2) {
    if (i2 >= 0 && (i < 0 || v2 > v || (v2 == v && i2 < i))) { v = v2; i = i2; }
}
static __global__ __launch_bounds__(256) void k_scan_best(const float *__restrict__ llr, int nc, int *__restrict__ best_c,
                                                          float *__restrict__ best_llr) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int tid = threadIdx.x;
    const float *row = llr + (size_t)blockIdx.x * nc;
    float v = 0.f;
    int i = -1;
    for (int c = tid; c < nc; c += 256) {
        const float x = row[c];
        if (x == x) best_merge(v, i, x, c);
    }
    sv[tid] = v;
    si[tid] = i;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
            best_merge(v, i, sv[tid + o], si[tid + o]);
            sv[tid] = v;
            si[tid] = i;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (best_c) best_c[blockIdx.x] = i;
        if (best_llr) best_llr[blockIdx.x] = i >= 0 ? v : __int_as_float(0x7fc00000);
    }
}

}  // namespace qfa_dla
