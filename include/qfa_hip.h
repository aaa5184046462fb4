/* qfa_hip.h -- C-ABI of libqfa_hip.so, the MI355X (gfx950) implementation of the QFA hot path.
 *
 * The reference (ZechangSun/QFA) is pure Python and has no FFI: the boundary it offers is the
 * Python method surface of QFA/model.py and QFA/optimizer.py.  qfa_amd keeps that surface in
 * Python and calls the functions below through ctypes (qfa_amd/_lib.py).  Every entry point
 * names the reference interface it replaces (file:line in the reference tree).
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (torch tensors: tensor.data_ptr());
 *     the library allocates nothing, reads no environment variable, keeps no mutable state (but the
 *     per-device compute-unit count, queried once) and is re-entrant across streams and devices;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default);
 *   - arrays are row-major, contiguous, float32; masks are 1 byte per pixel (torch.bool);
 *   - return value: 0 = ok, negative = invalid argument (QFA_E_*), positive = hipError_t;
 *     the library never throws and never calls exit();
 *   - B spectra, Npix = Nb + Nr pixels (blue side first), Nh latent factors (1..32).
 */
#ifndef QFA_HIP_H
#define QFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QFA_ABI_VERSION 4   /* v2: qfa_batch_t carries the factored-z input form; *_ex_f32 entry points with `flags`;
                             * v3: qfa_batch_t carries the resident, indexed input form (rows, row_stride);
                             * v4: qfa_zabs_factor_f32, QFA_E_FLAGS                                                  */

#define QFA_E_NULL      (-1)   /* a required pointer is NULL            */
#define QFA_E_SIZE      (-2)   /* B/Npix/Nb/Nh out of range              */
#define QFA_E_WORKSPACE (-3)   /* workspace smaller than qfa_workspace_bytes */
#define QFA_E_TAU       (-4)   /* unknown tau model                      */
#define QFA_E_FLAGS     (-5)   /* a `flags` bit that does not apply to this shape (QFA_F_S3_FAST at N_h <= 16) */

/* Mean-optical-depth model tau(z) = (amp * ((1+z)*scale)^expo + offset) * series_coeff
 * (reference QFA/utils.py:95-141, 149-171).  qfa_tau_model() fills it for the four built-ins. */
typedef struct {
    float amp;      /* already multiplied by the Lyman-series coefficient */
    float scale;
    float expo;
    float offset;   /* already multiplied by the Lyman-series coefficient */
} qfa_tau_t;

enum { QFA_TAU_BECKER = 0, QFA_TAU_FG = 1, QFA_TAU_KAMBLE = 2, QFA_TAU_MOCK = 3 };

/* Model parameters (reference QFA/model.py:37-55, property `parameters` :297-306). */
typedef struct {
    const float *F;      /* (Npix, Nh) */
    const float *Psi;    /* (Npix,)    */
    const float *omega;  /* (Nb,)      */
    const float *tau0;   /* scalar on device */
    const float *c0;     /* scalar on device */
    const float *beta;   /* scalar on device */
} qfa_params_t;

/* Spectra batch (contract of Dataloader.next_batch, reference QFA/dataloader.py:124-138). */
typedef struct {
    const float   *delta;   /* (B, Npix)  delta = flux - mu*A for training; raw flux for predict */
    const float   *error;   /* (B, Npix)  */
    const float   *zabs;    /* (B, Nb)    */
    const uint8_t *mask;    /* (B, Npix)  1 = pixel is used; masked pixels may hold -999 */
    const float   *A_blue;  /* optional (B, Nb): host-supplied exp(-tau(zabs)) for a custom tau
                               callable (reference QFA/model.py:26,43); NULL = use `tau` */
    /* Factored-z input form (ABI v2).  The reference's loader builds zabs[s][i] = (1 + z_qso[s]) wav[i] / 1215.67 - 1
     * (QFA/dataloader.py:102): 1 + zabs is the product of a per-spectrum and a per-pixel factor.  A caller that has
     * them passes zq1 = 1 + z_qso (B,) and pix_ratio = wav_blue / 1215.67 (Nb,) and may leave zabs NULL: the (B, Nb)
     * array is then never read (4 Nb bytes per spectrum and pass) and (1+z)^beta, tau(z) become products of a
     * per-spectrum and a per-pixel term (three transcendentals per blue element instead of six).  Both NULL = read
     * zabs.  Not combined with A_blue (a custom tau callable is evaluated on zabs by the caller). */
    const float   *zq1;        /* optional (B,)  */
    const float   *pix_ratio;  /* optional (Nb,) */
    /* Resident, indexed input form (ABI v3).  The reference materialises every batch on the host
     * (QFA/dataloader.py:124-138) and shuffles by permuting the whole data set (:154-167).  Here the data set can stay
     * where it is in HBM: spectrum s of the batch is row  r = rows ? rows[s] : s  of delta / error / mask -- rows
     * `row_stride` ELEMENTS apart (4 row_stride bytes for delta and error, row_stride bytes for the mask) -- and of zabs
     * (rows Nb apart) and zq1, so that a batch is B indices into arrays that are built once and a shuffled epoch is one
     * permutation on the device.  row_stride = 0 means Npix (contiguous rows); a loader that pads its rows to a multiple of
     * 32 elements (128 bytes) gives every row the alignment the kernels' 128-byte row segments like (N_pix = 1913, 9243:
     * 4 - 12 % of passes 1 and 2).  Pixels [Npix, row_stride) of a row are never read.  Outputs (nll, ll, hmean, hcov,
     * cont, unc) are in batch order and contiguous.  Not combined with A_blue. */
    const int32_t *rows;       /* optional (B,) device array of row indices, each >= 0 */
    int64_t        row_stride; /* 0 = Npix; else >= Npix */
} qfa_batch_t;

/* `flags` of the *_ex_f32 entry points (0 = the defaults; A/B timing and the cross-checks in tests/). */
#define QFA_F_PASS2_F32    0x1u  /* N_h <= 16: pass 2 in its float32-MFMA form (k_grads; never the default there)    */
#define QFA_F_PASS2_XDL    0x2u  /* N_h <= 16: pass 2 in its two-role all-XDL form (k_grads_x: 64 spectra per workgroup
                                  * walk the pixel axis)                                                         */
#define QFA_F_S3_FAST      0x4u  /* N_h = 17..32: stage 3 of pass 2 (k_grads_s3) with three bf16 piece products (operands
                                    carried to ~17 bits, <= 1.1e-5 per product).  Kept for callers that set it; since
                                    round 5 the default form runs three FLOAT16 piece products at float32 grade and is
                                    as fast.  At N_h <= 16 there is no such form: the call returns QFA_E_FLAGS        */
#define QFA_F_PREDICT_F32  0x8u  /* posterior writer in its float32-MFMA form (k_predict_out)                   */
#define QFA_F_SYNC         0x20u /* debugging: synchronise `stream` before returning, so that an asynchronous fault of
                                    THIS call's kernels is returned by THIS call (positive hipError_t) instead of
                                    surfacing at the caller's next synchronisation without context               */
#define QFA_F_PASS2_PIXRES 0x40u /* N_h <= 16: pass 2 in its pixel-resident all-XDL form (k_grads_t: a wave owns 16 pixels
                                  * and walks the spectra; the per-spectrum operands stream through LDS).  Without any
                                  * QFA_F_PASS2_* flag the library picks between k_grads_x (small batches) and this form
                                  * (from 96 spectra per CU on; N_h <= 8 and N_pix >= 1024: from 36 per CU on) --
                                  * qfa_host.h, pass2_use_pixres                                                      */
#define QFA_F_ZERO_ACCUM   0x80u /* qfa_nll_grad_*: the library zeroes `accum` itself before it adds to it (inside the first
                                  * kernel of the call: one launch less than a caller-side fill -- the step of a small
                                  * batch is a chain of dependent launches a few microseconds long)                  */
#define QFA_F_EXACT_GRAD   0x100u /* qfa_nll_grad_*: exact gradients of the reported loss instead of the reference's formulas
                                  * (opt-in; the default keeps the reference bit for bit).  The reference (QFA/model.py:137-144)
                                  * multiplies the F term by diag(A) once too often, uses 1 - tau0 (1+z)^beta - c0 with an extra
                                  * zd factor in the tau0 / c0 / beta terms, and divides every element by its own count.  In this
                                  * mode, with zd = r^2, r = 1 - c0 - exp(-t), t = tau0 (1+z)^beta, e' = dG omega 2 r (blue pixels):
                                  *   accF  = -dNLL/dF   (k_solve writes Z = -C^-1 and p = y, so pass 2 runs unchanged;
                                  *                       the reference's gF_i = wD A^3 f_i - wD A^2 f_i Z - A u p, Z = C^-1 T)
                                  *   g_tau0 =  sum e' exp(-t) (1+z)^beta      (reference: -sum e (1+z)^beta, e = dG omega zd^2 2 root)
                                  *   g_beta =  sum e' exp(-t) t ln(1+z)       (reference: -sum e tau0 (1+z)^beta ln(1+z))
                                  *   g_c0   = -sum e'                         (reference: -sum e)
                                  *   gPsi, gOmega, NLL: unchanged (already exact)
                                  * and scalar slot 6 of `accum` gets +B, the way slot 5 counts spectra: the buffer carries
                                  * its mode through an all-reduce, and qfa_finalize_grads_f32 / qfa_finalize_adam_clip_f32
                                  * read it there (see qfa_accum_floats).                                            */
/* (0x10: the one-wave-per-SIMD form k_grads_w of round 3, removed from the library in round 4 -- same results, 5.4 against
 *  2.15 ms at c3; the measurement is kept in profiles/r3_ablation_pass2.txt) */

int qfa_abi_version(void);

/* fills `out` for which in QFA_TAU_*, series 1..30 (reference QFA/utils.py:149-171,
 * coefficients QFA/Lyman_series.csv:2-31). */
int qfa_tau_model(int which, int series, qfa_tau_t *out);

/* bytes of scratch needed by qfa_nll_grad_f32 / qfa_predict_f32 for this shape */
size_t qfa_workspace_bytes(int B, int Npix, int Nh);

/* number of floats in the packed accumulation buffer used by qfa_nll_grad_f32 and
 * qfa_finalize_grads_f32:  [accF Npix*Nh | sumA Npix | gPsi Npix | gOmega Nb | cnt Npix | 8 scalars]
 * scalars = {g_tau0, g_c0, g_beta, n_spectra_with_blue, sum_nll, n_spectra, n_spectra_exact, 0}.
 * This is the buffer a data-parallel job all-reduces (sum) across ranks once per step.
 * n_spectra_exact (slot 6) counts the spectra of QFA_F_EXACT_GRAD launches and selects what the finalize calls compute:
 *   slot 6 = 0        the reference's semantics (every gradient sum / count, 0/0 = NaN);
 *   slot 6 = slot 5   exact semantics: gF = -accF, every gradient divided by n_spectra (normalize = 0: raw sums), so
 *                     the step's gradient is that of loss = sum NLL / B; an element no spectrum observes gets 0;
 *   otherwise         launches of both modes were added into one buffer (e.g. ranks that disagree): NaN in the loss
 *                     and in every gradient. */
size_t qfa_accum_floats(int Npix, int Nb, int Nh);

/* Replaces the loop body of QFA.forward (reference QFA/model.py:98-103) and
 * QFA.loglikelihood_and_gradient_for_single_spectra (:107-158) together with MatrixInverse /
 * MatrixLogDet (QFA/utils.py:12-54) for a whole batch.
 *   nll   (B,)  per-spectrum negative log-likelihood (out, may be NULL)
 *   accum qfa_accum_floats() floats, ADDED to (caller zeroes it once per step).
 * The per-spectrum sums are raw (not normalised): see qfa_finalize_grads_f32.
 * Limit: the counts in `accum` (cnt per pixel, n_spectra, n_spectra_with_blue) are float32 sums of ones, exact up to
 * 2^24: B > 16 777 216 returns QFA_E_SIZE, and a caller that adds several launches (or ranks) into one buffer must
 * finalise before the total number of spectra passes 2^24. */
int qfa_nll_grad_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau,
                     int B, int Npix, int Nb, int Nh,
                     float *nll, float *accum, void *workspace, size_t workspace_bytes,
                     void *stream);

/* Same call with stage timing for benchmarks: `events` is NULL or an array of 5 hipEvent_t
 * (entries may be NULL) recorded on `stream` at {start, after the parameter-image build, after pass 1
 * (moments), after the k x k solve, after pass 2 (gradients)}. */
int qfa_nll_grad_events_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau,
                            int B, int Npix, int Nb, int Nh,
                            float *nll, float *accum, void *workspace, size_t workspace_bytes,
                            void *stream, void *const *events);

/* Deterministic accumulation (SURVEY.md section 7 hard part 5, 8(e)).  By default the tiles of a block of 64 spectra
 * are added to `accum` with float32 atomics, whose arrival order -- and so the last bits of the sums -- changes
 * from run to run.  With a slab of qfa_det_slab_bytes() bytes every block writes its tile partials to its own
 * row of the slab (plain stores) and a reducer adds the rows to `accum` in block order: two runs on the same
 * inputs (and the same B, which fixes the work plan) are bit-identical.  slab == NULL is qfa_nll_grad_events_f32.
 * (Where pass 2 runs in its pixel-resident form -- from 96 spectra per CU on, 36 at N_h <= 8, or QFA_F_PASS2_PIXRES --
 * the per-range sums always leave through such rows, inside the workspace when slab == NULL: no float atomics
 * there in either mode.) */
size_t qfa_det_slab_bytes(int B, int Npix, int Nb, int Nh);
/* The split of the pixel-resident pass 2 (N_h <= 16) on this device: `ranges` ranges of `range_groups` groups of 16 spectra each
 * (the last range takes what is left; range_groups is even at N_h = 9..16, where the pass contracts pairs of groups).
 * deterministic != 0: the plan of a call with a slab.  Host only. */
int qfa_pixres_plan(int B, int Npix, int Nh, int deterministic, int *ranges, int *range_groups);
int qfa_nll_grad_det_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau,
                         int B, int Npix, int Nb, int Nh,
                         float *nll, float *accum, void *workspace, size_t workspace_bytes,
                         void *slab, size_t slab_bytes, void *stream, void *const *events);

/* The general form of the three calls above: slab may be NULL (then slab_bytes is ignored), events may be NULL,
 * flags = QFA_F_* (0 = defaults). */
int qfa_nll_grad_ex_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau,
                        int B, int Npix, int Nb, int Nh,
                        float *nll, float *accum, void *workspace, size_t workspace_bytes,
                        void *slab, size_t slab_bytes, unsigned flags, void *stream, void *const *events);

/* Replaces the normalisation of QFA.forward (reference QFA/model.py:104): elementwise
 * grad = sum / count (0/0 = NaN), loss = sum_nll / n_spectra (model.py:100); exact semantics when the buffer's slot 6
 * says so (QFA_F_EXACT_GRAD, qfa_accum_floats).  Reads `accum`
 * (after the optional all-reduce) and writes gradients with the reference's shapes.
 * normalize = 0 returns the raw sums instead (the per-spectrum gradient of
 * loglikelihood_and_gradient_for_single_spectra when accum holds one spectrum). */
int qfa_finalize_grads_f32(const float *accum, const float *F, int Npix, int Nb, int Nh,
                           int normalize, float *gF, float *gPsi, float *gOmega, float *gTau0,
                           float *gC0, float *gBeta, float *loss, void *stream);

/* Replaces QFA.prediction_for_single_spectra (reference QFA/model.py:160-180) for a batch:
 * b->delta holds the raw flux.  Outputs: ll (B,), hmean (B,Nh), hcov (B,Nh,Nh), cont (B,Npix),
 * unc (B,Npix): contiguous, any 4-byte alignment.  (The writer is fastest when the rows of cont / unc start on
 * 64-byte boundaries; at N_h <= 8 it stores whole aligned lines for any N_pix as long as cont and unc are
 * congruent modulo 128 bytes, as two allocations are.) */
int qfa_predict_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b,
                    const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh,
                    float *ll, float *hmean, float *hcov, float *cont, float *unc,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Same call with stage timing for benchmarks: `events` is NULL or an array of 4 hipEvent_t (entries
 * may be NULL) recorded on `stream` at {start, after the parameter images + pass 1 (moments),
 * after the k x k solve (ll, hmean, hcov written), after the continuum / uncertainty writer}. */
int qfa_predict_events_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b,
                           const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh,
                           float *ll, float *hmean, float *hcov, float *cont, float *unc,
                           void *workspace, size_t workspace_bytes, void *stream, void *const *events);

int qfa_predict_ex_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b,
                       const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh,
                       float *ll, float *hmean, float *hcov, float *cont, float *unc,
                       void *workspace, size_t workspace_bytes, unsigned flags, void *stream, void *const *events);

/* Posterior draws (additive to ABI v4).  The reference stops at the posterior moments: nb/predict.ipynb cell 11 plots
 * cont +- k uncertainty, and nb/generate_mock_continuum.ipynb cell 7 forms continua as `F@posterior_samples[idx]+mu`, one
 * vector at a time in numpy.  These calls draw latent vectors from N(hmean, hcov) and write the continua on the device.
 *
 * The draw contract.  For spectrum b of a call, r = row0 + b is its global row (int64); for sample s (0 <= s < S) and
 * latent component j (0 <= j < Nh):
 *   generator  Philox4x32-10 (the constants and rounds of Random123's philox4x32_10),
 *              key = (seed & 0xffffffff, seed >> 32), counter = (j >> 2, s, r & 0xffffffff, r >> 32) -> words x0..x3;
 *   uniforms   u_i = (x_i + 0.5) 2^-32 in float64 (in (0, 1): the log below is always finite);
 *   normals    Box-Muller in float64, each rounded once to float32:  z[4q+0] = sqrt(-2 ln u0) cos(2 pi u1),
 *              z[4q+1] = sqrt(-2 ln u0) sin(2 pi u1), z[4q+2], z[4q+3] the same of (u2, u3), q = j >> 2;
 *   latent     h[b,s,:] = hmean[b] + C_b z[b,s,:] in float64, rounded once, where C_b is the lower Cholesky factor of the
 *              LOWER triangle of hcov[b] (float32, as qfa_predict_f32 writes it) computed in float64.  A pivot <= 0 zeroes
 *              its column (the defined result for the near-singular hcov of high-S/N spectra); a NaN or Inf anywhere in
 *              hcov[b] or hmean[b] makes every value of that spectrum's draws NaN and touches no other spectrum;
 *   continuum  cont[r, p] = mu[p] + sum_j F[p, j] h[r, j] on ALL pixels (the `cont` of qfa_predict_f32), a float32 fma chain
 *              from mu in order of j.
 * Consequences: draws depend only on (seed, r, s, j) -- not on how a data set is split into calls, the launch shape or Nh
 * (the draws at Nh = 8 are a prefix of those at Nh = 16); hmean = 0, hcov = I draws from the prior, h = z.  A captured
 * graph replays the seed it was captured with: the same draws on every replay.
 * Neither call synchronises or allocates (graph-capturable). */

/* h (B, S, Nh) float32, contiguous: S draws of every spectrum of hmean (B, Nh), hcov (B, Nh, Nh).  row0 >= 0.
 * Returns QFA_E_NULL, or QFA_E_SIZE for B < 0, S < 1, Nh outside 1..32, row0 < 0; B = 0 does nothing. */
int qfa_sample_latent_f32(const float *hmean, const float *hcov, int B, int Nh, int S, uint64_t seed, int64_t row0,
                          float *h, void *stream);

/* bytes of scratch of qfa_continua_f32 (an image of F and mu, (Nh + 1) rows padded to 256 pixels); 0 = unsupported shape */
size_t qfa_continua_workspace_bytes(int Npix, int Nh);

/* out (R, Npix) = mu + F h for R latent rows h (R, Nh) -- the mock-continuum notebook's `F@h+mu` for a whole batch
 * (h of qfa_sample_latent_f32 is R = B S rows).  F (Npix, Nh), mu (Npix,); out contiguous at any 4-byte alignment; 64-bit
 * indices (R Npix may pass 2^31).  Returns QFA_E_NULL, QFA_E_SIZE (R < 0, Npix < 1, Nh outside 1..32) or QFA_E_WORKSPACE;
 * R = 0 does nothing. */
int qfa_continua_f32(const float *F, const float *mu, const float *h, int64_t R, int Npix, int Nh, float *out,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Mock spectra and posterior-predictive replicates (additive to ABI v4).  The model is generative -- reference README.md:46-54,
 *   flux = A (mu + F h + sqrt(Psi) e1) + sqrt(omega zdep) e2 + sigma e3,
 * with the noise terms of QFA/model.py:125-131 -- but the reference only ever draws continua, one vector at a time in numpy
 * (nb/generate_mock_continuum.ipynb cell 7).  This call draws whole spectra on the device, under each spectrum's own noise and mask.
 *
 * The draw contract.  For spectrum b of a call, r = row0 + b is its global row (int64); for replicate s (0 <= s < S) and pixel p:
 *   latent     h[b,s,:] is an INPUT, (B, S, Nh) float32: qfa_sample_latent_f32's output.  With hmean = 0, hcov = I that call draws
 *              from the prior (mock data); with the posterior of qfa_predict_f32 the result is a posterior-predictive replicate;
 *   noise      the three noise terms are independent Gaussians and are drawn as ONE normal of variance
 *              D = A^2 Psi + omega zdep + sigma^2   (sigma = b->error; SURVEY App. A step 3, the D of the likelihood kernels);
 *   normal     e[r,s,p] = z[p & 3] of the Philox4x32-10 / float64 Box-Muller normals above, key = (seed & 0xffffffff, seed >> 32),
 *              counter = (0x80000000 | (p >> 2), s, r & 0xffffffff, r >> 32): four consecutive pixels share one Philox call.  The
 *              latent stream's first counter word is 0..7, so bit 31 keeps the two streams disjoint under one seed;
 *   value      c = mu[p] + sum_j F[p,j] h[b,s,j], the float32 fma chain of qfa_continua_f32 in order of j;
 *              flux = fma(sqrt(D), e, A c) in float32, A c and sqrt(D) each rounded once.  A and zdep are evaluated the way the
 *              likelihood kernels evaluate them (the `tau` model; zabs, or the factored zq1 / pix_ratio form, or A_blue for a
 *              custom tau, which is read in batch order and needs zabs for zdep); on red pixels A = 1, zdep = 0;
 *   masks      b->mask == NULL: every pixel is used.  A masked pixel gets exactly -999.0f (the loader's sentinel) in every output;
 *              what `error` holds under the mask (-999, NaN, inf) reaches no output (a select, not a product);
 *   outputs    flux (B, S, Npix) and delta = flux - fl(mu A) (B, S, Npix) with the same float32 A; either may be NULL, not both;
 *              contiguous at any 4-byte alignment (rows that start on 16-byte boundaries are stored as whole dwordx4), 64-bit
 *              indices (B S Npix may pass 2^31).
 * Consequences: a value depends only on (seed, r, s, p), the parameters and the inputs of its own spectrum -- not on how a data
 * set is cut into calls, the launch shape or the number of ranks that share the rows; a non-finite h[b,s,:] makes the unmasked
 * pixels of replicate (b, s) non-finite and touches nothing else.  The call neither synchronises nor allocates (graph-capturable;
 * a captured graph replays the seed and row0 it was captured with).
 *
 * qfa_batch_t: error, mask (may be NULL), zabs | zq1 + pix_ratio | zabs + A_blue, rows / row_stride (the resident form: replicates
 * of a resident data set need no gather; h and the outputs are in batch order).  b->delta is not read.
 * workspace: qfa_mock_workspace_bytes (an image of F, mu, Psi, omega and the per-pixel factors of the factored-z form; 0 =
 * unsupported shape).  Returns QFA_E_NULL for a missing required pointer, QFA_E_SIZE for B < 0, S < 1, Nh outside 1..32, row0 < 0,
 * Npix < 1, Nb outside 0..Npix or 0 < row_stride < Npix, QFA_E_WORKSPACE; B = 0 does nothing. */
size_t qfa_mock_workspace_bytes(int Npix, int Nh);
int qfa_mock_spectra_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *h,
                         int B, int S, int Npix, int Nb, int Nh, uint64_t seed, int64_t row0, float *flux, float *delta,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Closed-form EM update of the factor loadings F (additive to ABI v4).  The reference moves every parameter with Adam
 * (QFA/model.py:212-214); F is the one group whose M-step has a closed form.  Per batch, at the current parameters, with the
 * posterior of the latent h of every spectrum s (y_s = C_s^-1 b_s as in qfa_predict_f32's hmean, E_s = C_s^-1 + y_s y_s^T):
 *   S2_i  = sum_s wD_si A_si^2 E_s           (Nh x Nh, symmetric)         wD = mask / D, a masked pixel contributes an exact 0
 *   S1_i  = sum_s wD_si A_si delta_si y_s    (Nh)                         whatever delta / error hold under the mask
 *   cnt_i = sum_s mask_si
 *   F_i  <- F_i + damping ((S2_i + ridge I)^-1 S1_i - F_i)
 * S2_i f_i - S1_i is the QFA_F_EXACT_GRAD gradient d(sum_s NLL_s)/df_i: the update's fixed point is that mode's stationary
 * point.  Psi, omega, tau0, beta, c0 are held fixed (a conditional M-step: with damping = 1, ridge = 0 the update cannot raise
 * sum_s NLL_s of the batch the statistics were taken on).
 *
 * qfa_em_floats: number of floats of the packed statistics  [S2 Npix Nh Nh | S1 Npix Nh | cnt Npix | sum NLL, n_spectra, 0, 0]
 * (sums only: the buffer a data-parallel job all-reduces); 0 = unsupported shape.  S2 is the full symmetric array, both triangles
 * bit-equal.  qfa_em_workspace_bytes: scratch of qfa_em_stats_f32 (it contains qfa_workspace_bytes); 0 = unsupported shape.
 *
 * qfa_em_stats_f32 ADDS the statistics of the batch into `stats` (QFA_F_ZERO_ACCUM: overwrites instead; QFA_F_SYNC as above;
 * any other flag: QFA_E_FLAGS) and writes the per-spectrum NLL at the parameters used to `nll` ((B,), may be NULL).  Every input
 * form of qfa_batch_t.  The sums over the batch leave through rows of the workspace and a fixed-order reducer -- no float
 * atomics: two calls on the same inputs give the same bits.  The same limit of 2^24 spectra per buffer as qfa_nll_grad_f32.
 *
 * qfa_em_update_f_f32 solves the Npix systems in float64 (Cholesky) and writes float32 F_out (Npix, Nh), which may alias F.
 * A row with cnt_i = 0, a pivot <= 0 or a non-finite solution is copied from F unchanged; *n_skipped (device memory, zeroed by
 * the call; may be NULL) counts such rows.  ridge >= 0.
 * Neither call synchronises or allocates (graph-capturable). */
size_t qfa_em_floats(int Npix, int Nh);
size_t qfa_em_workspace_bytes(int B, int Npix, int Nh);
int qfa_em_stats_f32(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh,
                     float *stats, float *nll, void *workspace, size_t workspace_bytes, unsigned flags, void *stream);
int qfa_em_update_f_f32(const float *stats, const float *F, int Npix, int Nh, double ridge, double damping, float *F_out,
                        unsigned *n_skipped, void *stream);

/* Lyman-alpha forest transmission and its redshift-binned stack (additive to ABI v4).  The reference presents QFA as a continuum
 * predictor FOR the forest (README.md, the paper's abstract): its users divide the observed flux by the continuum on the blue side,
 * T = flux / continuum, and stack T in redshift bins for the mean transmission and tau_eff(z) = -ln <T>; the reference itself stops
 * at the continuum (QFA/model.py:160-180).  This call forms T and its inverse variance for every draw of the latent and adds the
 * weighted sums of the stack, without ever writing a continuum.
 *
 * The contract.  For spectrum b of a call (row r = rows ? rows[b] : b of the input arrays), draw s (0 <= s < S) and blue pixel
 * p (0 <= p < Nb):
 *   inputs     b->delta holds the RAW FLUX (as for qfa_predict_f32), b->error the pipeline error sigma, b->mask may be NULL (every
 *              pixel is used); redshift from b->zabs, or from the factored zq1 + pix_ratio form; rows / row_stride: the resident
 *              form.  A_blue is ignored; the call uses neither a tau model nor Psi, omega, tau0, beta, c0.
 *              h (B, S, Nh) float32 in batch order: hmean with S = 1 (the posterior-mean continuum) or qfa_sample_latent_f32's draws.
 *              unc (B, Npix) in batch order as qfa_predict_f32 writes it, or NULL: the continuum's 1 sigma, meant for S = 1;
 *   redshift   z = zabs[r, p], or in the factored form z = fma(zq1[r], pix_ratio[p], -1) (one rounding);
 *   continuum  c = mu[p] + sum_j F[p,j] h[b,s,j], the float32 fma chain of qfa_continua_f32 in order of j;
 *   values     every operation rounded once, no contraction:  T = flux / c;  den = (T T) u2 + sigma sigma with u2 = unc unc or 0
 *              (a product, a product and an add);  iv = (c c) / den;
 *   use        mask != 0 && c > cont_min && isfinite(T) && isfinite(iv) (a NaN c fails the comparison).  What flux or error hold
 *              under the mask (-999, NaN, inf) reaches no output: selects, not products;
 *   outputs    trans, ivar (B, S, Nb) float32 in batch order, contiguous at any 4-byte alignment, 64-bit indices; either or both
 *              may be NULL.  An unused pixel gets exactly 0.0f in both;
 *   stack      (S, 4, nbin) float64 = [sum w | sum w T | sum w T^2 | n] per draw, or NULL (but not all three outputs NULL);
 *              w = (double)iv, or 1 with QFA_F_FOREST_UNIT_W; the terms are w, w T and w (T T) in float64, each product rounded
 *              once.  The sums run over the used pixels with p_lo <= p < p_hi whose bin k = floorf((z - z0) inv_dz) satisfies
 *              0 <= k < nbin: inv_dz = 1.0f / dz is formed once on the host in float32, the subtraction and the product are each
 *              rounded once, and the range test is done on the float (a NaN z is not stacked).  The call ADDS to `stack`;
 *              QFA_F_ZERO_ACCUM overwrites instead;
 *   sums       sums only -- the buffer a data-parallel job all-reduces.  No float atomics anywhere: every wave adds its pixels to a
 *              table of its own in a fixed order, the tables leave through rows of the workspace and a fixed-order reducer adds
 *              the rows to `stack`: two calls on the same inputs give the same bits.  z need not be monotone in p (it is for the
 *              reference's loader, which is the fast case: a wave's 256 pixels then fall into a few consecutive bins).
 * qfa_forest_stack_doubles: S 4 nbin, 0 = unsupported (S < 1, nbin outside 1..4096).  qfa_forest_workspace_bytes: the scratch (an
 * image of F and mu on the blue side and the rows of partial sums); 0 = unsupported shape.
 * Returns QFA_E_NULL for a missing required pointer; QFA_E_SIZE for B < 0, S < 1, Npix < 1, Nb outside 0..Npix, Nh outside 1..32,
 * bad bins (dz <= 0 or not finite, z0 not finite, nbin outside 1..4096, not 0 <= p_lo <= p_hi <= Nb) or 0 < row_stride < Npix;
 * QFA_E_FLAGS for any flag other than QFA_F_ZERO_ACCUM, QFA_F_SYNC, QFA_F_FOREST_UNIT_W; QFA_E_WORKSPACE.  B = 0 or Nb = 0 does
 * nothing to trans / ivar and, under QFA_F_ZERO_ACCUM, still zeroes `stack`.  Argument checks return before any device work.  The
 * call neither synchronises nor allocates (graph-capturable). */
typedef struct { float z0, dz; int nbin; int p_lo, p_hi; } qfa_forest_bins_t;   /* dz > 0, 1 <= nbin <= 4096, 0 <= p_lo <= p_hi <= Nb */
#define QFA_F_FOREST_UNIT_W 0x200u   /* qfa_forest_f32: stack with w = 1 instead of w = ivar */

size_t qfa_forest_stack_doubles(int S, int nbin);
size_t qfa_forest_workspace_bytes(int B, int S, int Npix, int Nb, int Nh, int nbin);
int qfa_forest_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, const float *unc,
                   int B, int S, int Npix, int Nb, int Nh, const qfa_forest_bins_t *bins, float cont_min,
                   unsigned flags, float *trans, float *ivar, double *stack,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The line-of-sight flux power spectrum of forest segments (P1D) and its stack in (k, z) (additive to ABI v4).  The statistic forest
 * users compute from the transmission: delta_F = T / <T>(z) - 1 on segments of the forest, a Fourier transform per segment, the noise
 * power subtracted, |delta~(k)|^2 stacked in redshift bins.  The reference stops at the continuum (QFA/model.py:160-180); this call
 * takes what qfa_forest_f32 writes (trans, ivar) and a mean transmission (the `mean` of qfa_forest_f32's stack) and runs the rest,
 * per posterior draw of the continuum, without ever writing delta_F.  The rest-frame grid is uniform in log lambda, so pixels are
 * uniform in velocity and a plain DFT per segment is the estimator; it runs as a float32 matrix product on the matrix pipe, exact
 * for every segment length.
 *
 * The contract.  Row r = b S + s (spectrum b of the call, draw s) of trans / ivar, segment g (0 <= g < nseg) of L = seg_len pixels
 * p = p_lo + g L + j, 0 <= j < L; M = L / 2 (integer division) modes:
 *   inputs     trans, ivar (B, S, Nb) float32 exactly as qfa_forest_f32 writes them: an unused pixel has ivar == 0.  Pixels outside
 *              the segments are not read.  `b` is read for redshift only -- zabs (rows Nb apart), or zq1 + pix_ratio with
 *              z = fma(zq1[r'], pix_ratio[p], -1) (one rounding), r' = rows ? rows[b] : b; delta, error, mask, A_blue are not read.
 *              tbar (St, nT) float32, St = 1 (one mean transmission for every draw) or St = S (row s serves draw s), over the bins
 *              (zT0, dzT, nT): kT = floorf((z - zT0) inv_dzT), qfa_forest_f32's rule (inv_dzT = 1.0f / dzT formed once on the host
 *              in float32, subtraction and product each rounded once, the range test on the float, a NaN z is in no bin);
 *   per pixel  used = ivar > 0 && 0 <= kT < nT && tb > 0 with tb = tbar[s or 0][kT] (a NaN tb fails the comparison).  A used
 *              pixel has d = T / tb - 1 (a division and a subtraction) and v = 1 / (ivar (tb tb)), every operation rounded once,
 *              no contraction; an unused pixel has d = 0 and v = 0 by selects, not products: a NaN under the mask reaches nothing;
 *   segment    n_used = the number of used pixels;  N = (sum_j v_j) / L (the sum and the quotient in float64, rounded to float32
 *              once);  X_m = sum_j d_j (cos(2 pi j m / L) - i sin(2 pi j m / L)) and P_m = (Re^2 + Im^2) / L for m = 1 .. M (mode 0
 *              is not computed).  Every twiddle is formed from the exact integer (j m) mod L, evaluated in float64 and rounded to
 *              float32 once; the sums over j are float32 fma chains in order of j (v_mfma_f32_16x16x4_f32); the two squares, their
 *              sum and the division by L are float32, each rounded once.  The segment is valid when n_used >= min_used;
 *              zc = z[r', p_lo + g L + L / 2] and kz = floorf((zc - z0) inv_dz) by the same rule;
 *   outputs    power (B S, nseg, M) and noise (B S, nseg) float32: an invalid segment gets exactly 0 in both;
 *              stack (S, nz, 2 + 2 M) float64 = [n | sum N | sum P_1..M | sum P^2_1..M] per draw and z-bin, over the valid segments
 *              with 0 <= kz < nz; the terms are formed in float64 from the float32 P and N, each product rounded once.  The call ADDS
 *              to `stack`; QFA_F_ZERO_ACCUM overwrites instead.  Any of the three may be NULL, but not all;
 *   sums       no float atomics anywhere: the per-segment rows leave through the workspace (or through `power` / `noise`), and a
 *              fixed-order reducer adds them, segment by segment in order of (b, g), onto what `stack` holds: two calls on the same
 *              inputs give the same bits, and draw s of a call of S draws gets the bits of a call of that draw alone.
 * qfa_p1d_stack_doubles: S nz (2 + 2 (L / 2)); 0 = unsupported (S < 1, nz outside 1..4096, L outside 1..4096).
 * qfa_p1d_workspace_bytes(R = B S, ...): the scratch (the twiddle table and the per-segment rows of one launch); 0 = unsupported
 * shape (R < 0, S < 1, R not a multiple of S, L outside 1..4096, nseg < 1, nseg L > Nb, nz outside 1..4096).
 * Returns QFA_E_NULL for a missing required pointer (trans, ivar, b, tbar, p, workspace, all three outputs, zabs without the
 * factored pair, half of the pair); QFA_E_SIZE for B < 0, S < 1, Nb < 1, seg_len outside 1..4096, nseg < 1, p_lo < 0,
 * p_lo + nseg seg_len > Nb, min_used < 1, bad bins of either kind (dz <= 0 or not finite, z0 not finite, count outside 1..4096),
 * St other than 1 or S, 0 < row_stride < Nb; QFA_E_FLAGS for any flag other than QFA_F_ZERO_ACCUM, QFA_F_SYNC; QFA_E_WORKSPACE.
 * B = 0 does nothing, except zeroing `stack` under QFA_F_ZERO_ACCUM.  Argument checks return before any device work.  The call
 * neither synchronises nor allocates (graph-capturable). */
typedef struct {
    float zT0, dzT; int nT, St;                 /* bins and rows of tbar: dzT > 0, 1 <= nT <= 4096, St = 1 or S */
    int p_lo, seg_len, nseg, min_used;          /* 1 <= seg_len <= 4096, nseg >= 1, p_lo + nseg seg_len <= Nb, min_used >= 1 */
    float z0, dz; int nz;                       /* bins of the stack: dz > 0, 1 <= nz <= 4096 */
} qfa_p1d_t;

size_t qfa_p1d_stack_doubles(int S, int nz, int L);
size_t qfa_p1d_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz);
int qfa_p1d_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                const qfa_p1d_t *p, unsigned flags, float *power, float *noise, double *stack,
                void *workspace, size_t workspace_bytes, void *stream);

/* Band powers of the forest's P1D and the covariance matrix between the bands, per posterior draw and z-bin (additive to ABI v4).
 * qfa_p1d_f32's stack holds a mean and a variance per Fourier mode and nothing between modes; a measurement is reported in
 * k-bands with the covariance between them, which masks, the window and the continuum make non-diagonal.  This call runs
 * qfa_p1d_f32's kernels unchanged into the workspace and reduces their rows to bands and to sums of outer products.
 *
 * The contract.  trans, ivar, b, tbar, B, S, Nb and p are qfa_p1d_f32's: the per-pixel rule, segment validity and the z-bin kz of a
 * segment are those of that call, and the P_m and N this call works from have the bits qfa_p1d_f32 writes to `power` / `noise` for
 * the same inputs.  M = seg_len / 2.
 *   bands      band (M,) int32 on the device: entry m - 1 is the band of mode m; a value outside 0 .. nband - 1 puts the mode in no
 *              band.  weight (M,) float32 on the device or NULL (every w_m = 1): the caller folds dv, 1 / n_a and 1 / W^2(k_m) in;
 *   segment    for a valid segment Q_a = sum_{m : band[m] = a} (double)w_m ((double)P_m - s (double)N), s = subtract_noise: float64,
 *              the product s N, the difference, the product with w_m and the sum each rounded once, no contraction, the sum in
 *              order of m from 0; a band without modes has Q_a = 0.  An invalid segment has P = N = 0 and gets exactly 0 in every
 *              band (finite weights) and adds to nothing;
 *   outputs    bandpower (B S, nseg, nband) float64; stack (S, nz, 1 + nband + nband^2) float64 = [n | sum Q_a | sum Q_a Q_b,
 *              row-major, full] per draw and z-bin over the valid segments with 0 <= kz < nz; each product Q_a Q_b rounded once;
 *              entries (a, b) and (b, a) hold the same bits.  The call ADDS to `stack`; QFA_F_ZERO_ACCUM overwrites.  Either
 *              output may be NULL, not both;
 *   sums       no float atomics.  The segments of a draw, in order of (b, g) over the whole call, are cut into chunks of
 *              qfa_p1d_band_chunk_segments() segments -- a constant of the library, not of the grid or the device.  A chunk's sums
 *              start from 0 and add its segments in order; they leave through the workspace, and a second kernel adds them in
 *              chunk order onto what `stack` holds.  The host cuts B into launches on chunk boundaries, so the result does not
 *              depend on the cut: two calls on the same inputs give the same bits, and draw s of a call of S draws gets the bits
 *              of a call on that draw alone.
 * qfa_p1d_band_stack_doubles: S nz (1 + nband + nband^2); 0 = unsupported (S < 1, nz outside 1..4096, nband outside 1..64).
 * qfa_p1d_band_workspace_bytes(R = B S, ...): qfa_p1d_workspace_bytes' shapes, and nband outside 1..64, give 0.  The rows and the
 * chunk partials of one launch aim at the cap of qfa_p1d_f32's rows; the least a launch holds is the fewest spectra whose segments
 * fill whole chunks (chunk / gcd(chunk, nseg)).
 * Returns every code of qfa_p1d_f32 for the arguments they share; QFA_E_NULL also for q, q->band or both outputs missing;
 * QFA_E_SIZE also for nband outside 1..64 or subtract_noise outside {0, 1}.  Argument checks return before any device work.  B = 0
 * does nothing, except zeroing `stack` under QFA_F_ZERO_ACCUM.  The call neither synchronises nor allocates. */
typedef struct {
    int nband;              /* 1 .. 64 */
    const int   *band;      /* device (M,) int32 */
    const float *weight;    /* device (M,) float32, or NULL = all 1 */
    int subtract_noise;     /* 0 or 1 */
} qfa_p1d_band_t;

size_t qfa_p1d_band_stack_doubles(int S, int nz, int nband);
size_t qfa_p1d_band_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nband);
int qfa_p1d_band_chunk_segments(void);
int qfa_p1d_band_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_p1d_band_t *q, unsigned flags, double *bandpower, double *stack,
                     void *workspace, size_t workspace_bytes, void *stream);

/* The pair-weighted correlation function of the forest along the line of sight, xi(l), and its (lag, z) stack, per posterior draw
 * (additive to ABI v4).  Every estimator above is a Fourier one: a masked pixel enters it as d = 0, and the power it reports is
 * convolved with the mask's window.  The statistic without a window is xi(l) = sum_j w_j w_{j+l} d_j d_{j+l} / sum_j w_j w_{j+l}: a
 * masked pixel has w = 0 and leaves the numerator and the normaliser alike.  It is the real-space partner of P1D, where metal lines
 * show as bumps at their velocity separation (SiIII at 2271 km/s), and its scatter over the draws is the continuum's error bar on it.
 * This call takes qfa_p1d_f32's inputs and writes the pair sums of every segment and their stack, without ever writing delta_F.
 *
 * The contract.  trans, ivar, b, tbar, B, S, Nb and p are qfa_p1d_f32's, bit for bit: `used`, d and v of a pixel, n_used, validity
 * (n_used >= min_used) and the z-bin kz of a segment (at its central pixel p_lo + g L + L / 2) are those of that call, with its rules
 * on the redshift forms and on NaN under the mask.  L = seg_len, lags l = 0 .. nlag - 1:
 *   per pixel  float32, every operation rounded once, no contraction:  wv = 1 / (v + sigma2_lss) (an addition and a division);
 *              w = used && isfinite(wv) ? wv : 0, or with QFA_F_XI_UNIT_W w = used ? 1 : 0, by selects;  x = w d;
 *   segment    for a valid segment W_l = sum_j w_j w_{j+l}, A_l = sum_j x_j x_{j+l} over j = 0 .. L - 1 - l -- pairs never cross a
 *              segment edge -- and N0 = sum_j (w_j w_j) v_j, the noise that sits in A_0.  float32 sums (fma chains); their order is
 *              a function of (L, nlag) alone, never of the grid, B or S;
 *   outputs    pairs (B S, nseg, 2, nlag) float32 = [W_l | A_l]; noise0 (B S, nseg) float32; an invalid segment gets exactly 0
 *              everywhere.  stack (S, nz, 2 + 5 nlag) float64 = [n | sum N0 | sum W_l | sum A_l | sum W_l^2 | sum A_l W_l |
 *              sum A_l^2] per draw and z-bin over the valid segments with 0 <= kz < nz; the three products are formed in float64
 *              from the float32 rows, each rounded once.  xi_l = sum A_l / sum W_l (sum N0 taken off lag 0), and the last three
 *              sums give the ratio's error from the scatter of the segments.  The call ADDS to `stack`; QFA_F_ZERO_ACCUM
 *              overwrites.  Any of the three may be NULL, but not all;
 *   sums       qfa_p1d_band_f32's: no float atomics; the segments of a draw, in order of (b, g) over the whole call, are cut into
 *              chunks of qfa_p1d_band_chunk_segments(); a chunk's sums start from 0 and add its segments in order, leave through
 *              the workspace, and a second kernel adds them in chunk order onto what `stack` holds.  The host cuts B on chunk
 *              boundaries: two calls on the same inputs give the same bits, and draw s of a call of S draws gets the bits of a
 *              call on that draw alone.
 * qfa_xi_stack_doubles: S nz (2 + 5 nlag); 0 = unsupported (S < 1, nz outside 1..4096, nlag outside 1..4096).
 * qfa_xi_workspace_bytes(R = B S, ...): qfa_p1d_workspace_bytes' shapes, and nlag outside 1..L, give 0.  The rows and the chunk
 * partials of one launch aim at the cap of qfa_p1d_f32's rows; the least a launch holds is the fewest spectra whose segments fill
 * whole chunks.
 * Returns every code of qfa_p1d_f32 for the arguments they share; QFA_E_NULL also for x or all three outputs missing; QFA_E_SIZE
 * also for nlag outside 1..seg_len or sigma2_lss negative or not finite; QFA_E_FLAGS for any flag other than QFA_F_ZERO_ACCUM,
 * QFA_F_SYNC, QFA_F_XI_UNIT_W.  Argument checks return before any device work.  B = 0 does nothing, except zeroing `stack` under
 * QFA_F_ZERO_ACCUM.  The call neither synchronises nor allocates. */
typedef struct { int nlag; float sigma2_lss; } qfa_xi_t;      /* 1 <= nlag <= seg_len; sigma2_lss >= 0, finite */
#define QFA_F_XI_UNIT_W 0x400u   /* qfa_xi_f32: w = 1 on a used pixel instead of 1 / (v + sigma2_lss) */

size_t qfa_xi_stack_doubles(int S, int nz, int nlag);
size_t qfa_xi_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nlag);
int qfa_xi_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
               const qfa_p1d_t *p, const qfa_xi_t *x, unsigned flags, float *pairs, float *noise0, double *stack,
               void *workspace, size_t workspace_bytes, void *stream);

/* The probability distribution of the transmitted flux, P(F), of forest segments and the stack its covariance matrix comes from, per
 * posterior draw and z-bin (additive to ABI v4).  The one-point statistic reported beside P1D and xi, and the one most sensitive to
 * the continuum: a continuum placed 2 % low moves the whole F ~ 1 end of the PDF, which is what the scatter over the draws measures.
 * This call takes qfa_p1d_f32's inputs and counts the pixels of every segment into flux bins; the sums of the counts and of their
 * outer products per z-bin give the PDF and, with segments as the independent units, the covariance between its bins.
 *
 * The contract.  trans, ivar, b, tbar, B, S, Nb and p are qfa_p1d_f32's, bit for bit: `used` of a pixel (ivar > 0 && 0 <= kT < nT &&
 * tb > 0), n_used, validity of a segment (n_used >= min_used) and its z-bin kz (at the central pixel p_lo + g L + L / 2) are those of
 * that call, with its rules on the three redshift forms and on NaN under the mask: the PDF is measured on exactly the pixels and
 * segments of the P1D.  nt flux bins [t0 + a dt, t0 + (a + 1) dt), a = 0 .. nt - 1:
 *   per pixel  float32, every operation rounded once, no contraction:  x = T, or with QFA_F_PDF_RELATIVE x = T / tb (one division);
 *              counted = used && ivar >= ivar_min;  fa = floorf((x - t0) inv_dt), a subtraction and a product, inv_dt = 1.0f / dt
 *              formed once on the host in float32; the range test is on the float, qfa_forest_f32's bin rule: an edge belongs to the
 *              bin above it.  Without QFA_F_PDF_CLAMP a pixel with fa outside [0, nt) is in no bin; with it fa < 0 goes to bin 0
 *              and fa >= nt (x = +inf included) to bin nt - 1.  A NaN x is in no bin either way.  Everything is done by selects:
 *              nothing under the mask reaches an output;
 *   segment    h_a = the number of counted pixels of bin a; n_cnt = the number of counted pixels, in a bin or not.  An invalid
 *              segment has h = 0 and n_cnt = 0 and adds to nothing;
 *   outputs    hist (B S, nseg, nt) int32; stack (S, nz, 2 + nt + nt^2) float64 = [n_seg | sum n_cnt | sum h_a | sum h_a h_b,
 *              row-major, full] per draw and z-bin over the valid segments with 0 <= kz < nz; entries (a, b) and (b, a) are equal.
 *              The call ADDS to `stack`; QFA_F_ZERO_ACCUM overwrites.  Either output may be NULL, not both;
 *   sums       every term is an integer, h_a h_b <= L^2 <= 2^24, so every entry of `stack` is exact while it stays below 2^53 --
 *              that takes more than 5 10^8 segments in one (draw, z-bin).  The result therefore does not depend on the order of
 *              addition, on how the host cuts B into launches, on B, S or on how a caller splits its spectra over calls that add
 *              into one stack; draw s of a call of S draws equals a call on that draw alone.  No atomics all the same: a chunk of
 *              qfa_p1d_band_chunk_segments() segments leaves its int32 sums through the workspace and a second kernel adds them
 *              onto what `stack` holds.
 * qfa_flux_pdf_stack_doubles: S nz (2 + nt + nt^2); 0 = unsupported (S < 1, nz outside 1..4096, nt outside 1..64).
 * qfa_flux_pdf_workspace_bytes(R = B S, ...): qfa_p1d_workspace_bytes' shapes, and nt outside 1..64, give 0.  The workspace holds the
 * chunk partials of one launch alone (hist is written directly), aimed at the cap of qfa_p1d_f32's rows, one chunk at the least.
 * Returns every code of qfa_p1d_f32 for the arguments they share; QFA_E_NULL also for q or both outputs missing; QFA_E_SIZE also for
 * nt outside 1..64, dt <= 0 or not finite, t0 not finite, ivar_min negative or not finite; QFA_E_FLAGS for any flag other than
 * QFA_F_ZERO_ACCUM, QFA_F_SYNC, QFA_F_PDF_RELATIVE, QFA_F_PDF_CLAMP.  Argument checks return before any device work.  B = 0 does
 * nothing, except zeroing `stack` under QFA_F_ZERO_ACCUM.  The call neither synchronises nor allocates. */
typedef struct { float t0, dt; int nt; float ivar_min; } qfa_pdf_t;   /* dt > 0 finite, t0 finite, 1 <= nt <= 64, ivar_min >= 0 finite */
#define QFA_F_PDF_RELATIVE 0x800u    /* qfa_flux_pdf_f32: bin x = T / tbar(z) instead of x = T */
#define QFA_F_PDF_CLAMP    0x1000u   /* qfa_flux_pdf_f32: x below the range counts in bin 0, above it in bin nt - 1 (the convention of the published PDFs) */

size_t qfa_flux_pdf_stack_doubles(int S, int nz, int nt);
size_t qfa_flux_pdf_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nt);
int qfa_flux_pdf_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_pdf_t *q, unsigned flags, int *hist, double *stack,
                     void *workspace, size_t workspace_bytes, void *stream);

/* The variance function of the forest: the moments of delta_F in bins of the pipeline's noise variance v and of redshift, per
 * posterior draw (additive to ABI v4).  qfa_xi_f32 weights a pixel by 1 / (v + sigma2_lss) and qfa_p1d_f32 subtracts a noise level
 * made of v: both rest on v being right and on a number, sigma2_lss, that nothing above produces.  The standard answer of the Lya
 * pipelines is to measure var(delta_F) in bins of v and z and to fit var = eta v + sigma2_lss (+ eps / v): eta corrects the
 * pipeline's noise, sigma2_lss is the intrinsic variance of the forest, and the scatter of the fit over the draws is the continuum's
 * error bar on both.  This call takes qfa_p1d_f32's inputs and writes the five sums per bin the fit needs, without ever writing
 * delta_F; the fit itself is a closed form on the stack (qfa_amd.stacks.VarianceStack.fit).
 *
 * The contract.  trans, ivar, b, tbar, B, S, Nb and p are qfa_p1d_f32's, bit for bit: `used`, d and v of a pixel, n_used, validity
 * (n_used >= min_used) and the z-bin kz of a segment (at its central pixel p_lo + g L + L / 2) are those of that call, with its rules
 * on the redshift forms and on NaN under the mask.  nv = n_oct << sub variance bins, 2^sub per octave from 2^e_lo on:
 *   bin rule   on bits, no logarithm: with u the int32 bit pattern of the float32 v, c = (u >> (23 - sub)) - ((e_lo + 127) << sub)
 *              (an arithmetic shift).  Bin c covers 2^(e_lo + (c >> sub)) [1 + m / 2^sub, 1 + (m + 1) / 2^sub), m = c & (2^sub - 1):
 *              an edge belongs to the bin above it.  Zero, denormal, negative, inf and NaN v have c outside [0, nv) by construction;
 *   per pixel  counted = used && the segment is valid && 0 <= c < nv && fabsf(d) <= d_max (false for a NaN d; d_max = FLT_MAX cuts
 *              the non-finite d alone).  Its terms in float64: (double)v, (double)d, d2 = (double)d (double)d (exact) and d4 = d2 d2
 *              (rounded once); no contraction.  Everything is done by selects: nothing under the mask reaches an output;
 *   segment    moments (B S, nseg, 5, nv) float64 = [n_a | sum v | sum d | sum d^2 | sum d^4] over the counted pixels of bin a.  The
 *              order of the additions is a fixed function of the segment's data and of (L, nv): never of the grid, of B, S or of
 *              how a batch is cut.  An invalid segment gets exactly 0 everywhere;
 *   outputs    stack (S, nz, 2 + 5 nv) float64 = [n_seg | n_used | n_a | sum v_a | sum d_a | sum d^2_a | sum d^4_a] per draw and
 *              z-bin over the valid segments with 0 <= kz < nz; n_used = the used pixels of those segments, so that n_used - sum_a
 *              n_a is what fell outside the bins or the cut.  The call ADDS to `stack`; QFA_F_ZERO_ACCUM overwrites.  Either output
 *              may be NULL, not both;
 *   sums       qfa_xi_f32's: no atomics; the segments of a draw, in order of (b, g) over the whole call, are cut into chunks of
 *              qfa_p1d_band_chunk_segments(); a chunk's sums start from 0 and add its segments in order, leave through the
 *              workspace, and a second kernel adds them in chunk order onto what `stack` holds.  The host cuts B on chunk
 *              boundaries: two calls on the same inputs give the same bits, and draw s of a call of S draws gets the bits of a
 *              call on that draw alone.
 * qfa_variance_stack_doubles: S nz (2 + 5 nv); 0 = unsupported (S < 1, nz outside 1..4096, nv outside 1..64).
 * qfa_variance_workspace_bytes(R = B S, ...): qfa_p1d_workspace_bytes' shapes, and nv outside 1..64, give 0.  The rows
 * (segment, 1 + 5 nv) float64 and the chunk partials of one launch aim at the cap of qfa_p1d_f32's rows; the least a launch holds
 * is the fewest spectra whose segments fill whole chunks.
 * Returns every code of qfa_p1d_f32 for the arguments they share; QFA_E_NULL also for q or both outputs missing; QFA_E_SIZE also
 * for sub outside 0..4, n_oct < 1, n_oct << sub above 64, e_lo < -126, e_lo + n_oct > 127, d_max <= 0 or NaN; QFA_E_FLAGS for any
 * flag other than QFA_F_ZERO_ACCUM, QFA_F_SYNC.  Argument checks return before any device work.  B = 0 does nothing, except zeroing
 * `stack` under QFA_F_ZERO_ACCUM.  The call neither synchronises nor allocates. */
typedef struct { int e_lo, n_oct, sub; float d_max; } qfa_var_t;   /* 0 <= sub <= 4, 1 <= n_oct << sub <= 64, -126 <= e_lo, e_lo + n_oct <= 127, d_max > 0 */

size_t qfa_variance_stack_doubles(int S, int nz, int nv);
size_t qfa_variance_workspace_bytes(int R, int S, int Nb, int L, int nseg, int nz, int nv);
int qfa_variance_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                     const qfa_p1d_t *p, const qfa_var_t *q, unsigned flags, double *moments, double *stack,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Observed-frame spectra onto the common rest-frame grid: rebin, normalise, S/N and the catalogue's counts (additive to ABI v4).
 * Every other entry point assumes the reference's contract -- "all spectra should have same wavelength grid", "spectra are
 * preprocessed as in the paper" (reference QFA/dataloader.py:21-24): rest frame, the common log-lambda grid, normalised at 1280 A,
 * -999 sentinels, and a catalogue whose `snr` and `num_mask` columns exist (QFA/dataloader.py:49).  The reference ships no such step.
 * This call takes spectra as a survey delivers them and writes the two (N, Npix) float32 arrays the loaders accept, and the
 * catalogue's columns.
 *
 * The contract.  N spectra, ragged: spectrum i owns the input pixels offsets[i] .. offsets[i + 1] - 1 (n of them) of
 *   inputs     wave (float64, observed-frame pixel centres in Angstrom, strictly increasing inside a spectrum), flux (float32),
 *              ivar (float32), bad (uint8, or NULL), offsets (int64, N + 1, non-decreasing, every n <= max_n_in: the CALLER checks
 *              these, the arrays live on the device), zqso (float64, N).  Input pixel j is usable when ivar_j > 0 and finite,
 *              flux_j is finite and bad_j == 0 (NULL: every bad_j = 0);  u_j = ivar_j if usable, else 0.  What an unusable pixel
 *              holds in flux (NaN, inf) reaches no sum: selects, not products.
 *              out_edges (float64, Npix + 1, rest frame, increasing: the caller checks) and wav_grid (float64, Npix, the pixel
 *              centres the windows below are tested on) come from the host, so both sides of every comparison share their bits;
 *   geometry   all in float64.  Input edges (n >= 2):  e_j = 0.5 (w_{j-1} + w_j) for 0 < j < n,  e_0 = w_0 - (e_1 - w_0),
 *              e_n = w_{n-1} + (w_{n-1} - e_{n-1}) -- additions, subtractions and halvings only, which no fused contraction can
 *              change.  Output edges in the observed frame E_k = out_edges[k] (1 + z) (one product, 1 + z one addition);
 *              width(k) = E_{k+1} - E_k;  overlap(j, k) = max(0, min(e_{j+1}, E_{k+1}) - max(e_j, E_k)).  A spectrum with n < 2, or
 *              whose 1 + z is not a positive finite number, covers nothing;
 *   rebin      per output pixel k, float64, every operation rounded once, no contraction, the sums in input-pixel order:
 *                c_jk = overlap(j, k) / width(k)              W = sum_j c_jk u_j              coverage_k = sum_{j usable} c_jk
 *                flux_k = (sum_j (c_jk u_j) f_j) / W          ivar_k = (W W) / sum_j c_jk (c_jk u_j)
 *              ivar_k is the inverse variance of that weighted mean for independent input pixels.  Pixel k is VALID iff
 *              coverage_k >= min_coverage and W > 0;
 *   norm       norm = (sum_k ivar_k flux_k) / (sum_k ivar_k) over the valid pixels with norm_lo <= wav_grid[k] < norm_hi, of the
 *              unrounded flux_k ("normalized at rest-frame wavelength 1280 A", reference nb/predict.ipynb).  The spectrum is OK
 *              iff that window holds at least norm_min_pixels valid pixels and norm > 0 and finite;
 *   outputs    flux_out[i, k] = float32(flux_k / norm), error_out[i, k] = float32(1 / (sqrt(ivar_k) norm)); exactly -999.0f in both
 *              for an invalid pixel and for EVERY pixel of a spectrum that is not ok -- the reference's sentinels: the mask is
 *              (flux != -999) & (error != -999) as everywhere else.  (N, Npix) contiguous, written once, 64-bit indices;
 *   record     per spectrum, whether ok or not, from the valid flags of the rebin, in two arrays: record_f64 (N, 2) = [norm | snr],
 *              record_i32 (N, 5) = [n_valid | n_lead | n_trail | num_mask | ok].  snr = the mean of
 *              flux_k sqrt(ivar_k) over the valid pixels with snr_lo <= wav_grid[k] < snr_hi, NaN if there are none;  n_valid;
 *              n_lead / n_trail = the length of the invalid run that touches the blue / red end (Npix in both when nothing is
 *              valid);  num_mask = the number of maximal runs of invalid pixels that touch neither end, the catalogue's "masked
 *              regions" (reference main.py:33) -- a leading run is what the spectrograph's blue limit leaves at low z: reported,
 *              but no masked region;  ok (0 / 1).  The five integers are int32 and exact;
 *   sums       float64 in one fixed order (per thread in order of k, a butterfly over the wave, the waves in order), no atomics.  A
 *              spectrum's outputs depend on that spectrum alone -- not on N, on how a data set is cut into calls, or on the number
 *              of ranks that share it -- and two calls on the same inputs give the same bits.
 * qfa_preprocess_workspace_bytes: the scratch (one byte per output pixel: its window flags); 0 = unsupported shape (N < 0, Npix
 * outside 1..16 384, max_n_in outside 0..32 768).
 * Returns QFA_E_NULL for q == NULL; QFA_E_SIZE for N < 0, Npix outside 1..16 384, max_n_in outside 0..32 768, min_coverage not in
 * (0, 1], a window that is empty (lo >= hi) or not finite, norm_min_pixels < 1; then N = 0 does nothing and returns 0; QFA_E_NULL
 * for any other missing pointer (bad may be NULL; wave, flux, ivar may be NULL when max_n_in = 0); QFA_E_WORKSPACE.  Argument checks
 * return before any device work.  The call neither synchronises nor allocates (graph-capturable). */
typedef struct {
    double min_coverage;        /* in (0, 1] */
    double norm_lo, norm_hi;    /* rest-frame Angstrom, lo < hi */
    double snr_lo, snr_hi;
    int norm_min_pixels;        /* >= 1 */
} qfa_preprocess_t;

size_t qfa_preprocess_workspace_bytes(int N, int Npix, int max_n_in);
int qfa_preprocess_f32(const double *wave, const float *flux, const float *ivar, const uint8_t *bad, const int64_t *offsets,
                       const double *zqso, int N, int max_n_in, const double *out_edges, const double *wav_grid, int Npix,
                       const qfa_preprocess_t *q, float *flux_out, float *error_out, double *record_f64,
                       int32_t *record_i32, void *workspace, size_t workspace_bytes, void *stream);

/* Catalogued absorbers and bad wavelengths: mask and correct (additive to ABI v4).  A damped Lyman-alpha system wipes out tens of
 * Angstrom of forest and its Lorentzian wings depress hundreds more; sky lines and Galactic Ca H&K spoil the same observed
 * wavelengths of every spectrum; a BAL trough spoils rest-frame intervals of one.  This call applies catalogues of the three to the
 * (N, Npix) rest-frame arrays every loader accepts -- qfa_preprocess_f32's output or data already in the reference's file format --
 * between preprocessing and everything after it: a spoiled pixel becomes the -999 sentinel, which every kernel of the package
 * treats as weight zero, the rest is divided by the absorbers' Voigt profile.  The reference ships no such step.
 *
 * The contract.
 *   inputs     flux, error (N, Npix) float32 with -999 sentinels; zqso (float64, N); wav_grid (float64, Npix, rest-frame pixel
 *              centres).  Absorbers as a CSR list: spectrum i owns entries abs_offsets[i] .. abs_offsets[i + 1] - 1 of abs_z (the
 *              absorber's redshift, 1 + z_a > 0) and abs_lognhi (log10 of the column density in cm^-2), both float64;
 *              abs_offsets (int64, N + 1) NULL = no absorbers.  obs_intervals (n_obs, 2) float64 [lo, hi) in observed-frame
 *              Angstrom, the same for every spectrum (NULL with n_obs = 0).  rest_offsets (int64, N + 1, NULL = none) /
 *              rest_intervals (., 2) float64 [lo, hi) in rest-frame Angstrom per spectrum.  Everything lives on the device; the
 *              CALLER checks that the offsets are non-decreasing and every list entry is finite, lo < hi, 1 + z_a > 0.
 *   profile    all in float64.  lam_obs = wav_grid[k] (1 + z_i)  (one addition, one product).  tau = 0; for each absorber j of
 *              the spectrum in list order, and for each of its lines in the order Ly-alpha (lam0 = 1215.67, f = 0.4164,
 *              Gamma = 6.265e8), then under QFA_ABS_LYB Ly-beta (1025.72, 0.07912, 1.897e8):
 *                x = (c / b) (lam_obs / (lam0 (1 + z_a)) - 1),  c = 299792.458,  b = b_kms;      P = x x
 *                a = Gamma lam0 1e-13 / (4 pi b)            ka = a / sqrt(pi)
 *                tau += 1.497e-15 10^logNHI f lam0 / b  H(a, x)
 *              H is the approximation of Tepper-Garcia (2006), with H0 = exp(-P), Q = 1.5 / P:
 *                1/16 <= P <= 750   H = H0 - (ka / P) [H0 H0 (4 P P + 7 P + 4 + Q) - Q - 1]
 *                P > 750            H = (ka / P) (1 + Q)    -- the same value: exp(-P) is 0 in float64 from P = 746 on
 *                P < 1/16           H = H0 - ka (g_0 + g_1 P + .. + g_9 P^9), the Taylor series of [..] / P, which the form above loses to
 *                                   cancellation (its 1.5 / P terms) and to 0 / 0 at P = 0:  g_k = 4 E_{k-1} + 7 E_k + 4 E_{k+1} +
 *                                   1.5 E_{k+2},  E_n = (-2)^n / n!, E_{-1} = 0:
 *                                   2, -4, 5/3, 14/15, -8/5, 352/315, -169/315, 38/189, -884/14175, 2584/155925
 *                                   (the next term is below 4e-15 ka at the switch; H(a, 0) = 1 - 2 ka, the Voigt function's value
 *                                   to first order in a)
 *              T = exp(-tau); no absorbers: T = 1 exactly.  The approximation is first order in a: against the Faddeeva function T
 *              is good to float32 grade for damped systems and worse for weaker ones at large b (profiles/absorber_accuracy.txt).
 *   pixels     an input pixel is valid iff flux != -999 and error != -999.  A valid pixel is MASKED iff T < t_min, or T is not
 *              finite (absorber-masked), or lam_obs lies in any [lo, hi) of obs_intervals, or wav_grid[k] in any [lo, hi) of the
 *              spectrum's rest intervals (interval-masked; a pixel masked for both reasons counts as absorber-masked).
 *   outputs    a masked or invalid pixel: exactly -999.0f in flux_out and error_out (what an invalid pixel holds -- NaN, inf --
 *              reaches nothing: selects, not products).  A kept pixel: flux_out = float32(double(flux) / T), error_out =
 *              float32(double(error) / T) under QFA_ABS_CORRECT, else the input's bits.  trans_out (N, Npix) float32 = T of every
 *              pixel, valid or not; may be NULL.  flux_out == flux and error_out == error (in place) is allowed.
 *   record     per spectrum, from the OUTPUT arrays, with qfa_preprocess_f32's definitions:  record_i32 (N, 6) = [n_valid |
 *              n_lead | n_trail | num_mask | n_absorber_masked | n_interval_masked],  record_f64 (N, 1) = [snr], the mean of
 *              double(flux_out) / double(error_out) over the kept pixels with snr_lo <= wav_grid[k] < snr_hi, NaN if none.
 *   sums       float64 in one fixed order (per thread in order of k, a butterfly over the wave, the waves in order), no atomics.  A
 *              spectrum's outputs depend on that spectrum alone -- not on N or on how a set is cut into calls -- and two calls on
 *              the same inputs give the same bits.
 * qfa_absorber_workspace_bytes: 0 = unsupported shape (N < 0, Npix outside 1..16 384); nothing is held between kernels, the size
 * of a supported shape is a token 16 bytes.
 * Returns QFA_E_NULL for q == NULL; QFA_E_SIZE for an unsupported shape, n_obs < 0, t_min outside [0, 1), b_kms not positive and
 * finite, an snr window that is empty or not finite; QFA_E_FLAGS for an unknown flag; then N = 0 does nothing and returns 0;
 * QFA_E_NULL for any other missing pointer (trans_out may be NULL; abs_offsets NULL = no absorbers, else abs_z and abs_lognhi are
 * required; obs_intervals is required when n_obs > 0; rest_offsets NULL = none, else rest_intervals is required);
 * QFA_E_WORKSPACE.  Argument checks return before any device work.  The call neither synchronises nor allocates (graph-capturable). */
enum { QFA_ABS_LYB = 0x1, QFA_ABS_CORRECT = 0x2 };
typedef struct {
    double t_min;               /* in [0, 1); 0.8 is the usual choice */
    double b_kms;               /* Doppler parameter of every absorber, km/s, > 0; 30 */
    double snr_lo, snr_hi;      /* rest-frame Angstrom, lo < hi */
    unsigned flags;             /* QFA_ABS_LYB | QFA_ABS_CORRECT */
} qfa_absorber_t;

size_t qfa_absorber_workspace_bytes(int N, int Npix);
int qfa_absorber_mask_f32(const float *flux, const float *error, const double *zqso, const double *wav_grid, int N, int Npix,
                          const int64_t *abs_offsets, const double *abs_z, const double *abs_lognhi,
                          const double *obs_intervals, int n_obs, const int64_t *rest_offsets, const double *rest_intervals,
                          const qfa_absorber_t *q, float *flux_out, float *error_out, float *trans_out, double *record_f64,
                          int32_t *record_i32, void *workspace, size_t workspace_bytes, void *stream);

/* The DLA finder: a likelihood-ratio scan of every spectrum over a table of transmission templates (additive to ABI v4).
 * qfa_absorber_mask_f32 applies a catalogue of damped Lyman-alpha systems; these calls produce one.  The method is the
 * Gaussian-process finder of Garnett et al. (2017) and Ho, Bird & Garnett (2020) on this package's model: for every spectrum and
 * every candidate (absorber redshift, column density) the model is multiplied by the candidate's Voigt profile, and the gain in
 * log-likelihood is the statistic.  The reference ships no such step.
 *
 * The rule.  A template is a per-pixel transmission V[c, k] (candidate c, pixel k of the model's rest-frame grid), (nc, Npix)
 * float32.  With the quantities of qfa_predict_f32 -- x = b->delta the RAW FLUX, sigma = b->error, A = exp(-tau(z)) and
 * zd = (1 - c0 - exp(-tau0 (1 + z)^beta))^2 on the blue side (A = 1, zd = 0 on the red side) -- candidate c models the spectrum as
 *   A' = V A        G = A^2 Psi + omega zd        D' = V^2 G + sigma^2        w' = mask / D'
 *   delta' = x - A' mu      C' = I + sum_k w' A'^2 f f^T      b' = sum_k w' A' delta' f      y' = C'^-1 b'
 *   NLL'(c) = ( sum_k w' delta'^2 - b'^T y' + n log 2 pi + sum_mask log D' + log det C' ) / 2
 * (the model's absorption variance omega zd lies behind the absorber too: hence V^2 G).  V = 1 gives NLL0, qfa_predict_f32's ll;
 * n, the number of used pixels, is the same for every candidate, and the output is
 *   llr[s, c] = NLL0[s] - NLL'[s, c].
 *   redshift   z = zabs[r, k], or in the factored form z = fma(zq1[r], pix_ratio[k], -1) (one rounding), r = rows ? rows[s] : s:
 *              one arithmetic behind both, so a zabs array that holds those z gives the factored form's bits; rows / row_stride
 *              as everywhere.  A_blue (a custom tau callable) is refused: QFA_E_NULL;
 *   arithmetic the per-pixel terms in float32, in DIFFERENCE form against V = 1:  w' A'^2 - w A^2,  w' A' delta' - w A delta,
 *              w' delta'^2 - w delta^2 + ln(1 - (1 - V^2) G / D).  Both members of a difference are formed by the same operations,
 *              so a pixel with V == 1.0f contributes exact zeros (and blocks of pixels where a whole tile of templates is 1.0f are
 *              skipped without changing a bit), and the error of llr scales with llr, not with NLL.  The sums over the pixels of
 *              the first two run on the matrix pipe (v_mfma_f32_16x16x4_f32, float32 accumulators, pixels in order), the third
 *              and every null sum in float64; C' = C0 + dC is factored in float64 (Cholesky) per candidate:
 *              llr = ( -ds + (b'^T y' - b0^T y0) - (log det C' - log det C0) ) / 2, rounded to float32 once;
 *   masks      a masked pixel (mask == 0) may hold NaN, inf or -999 in delta and error: they are not read.  A spectrum with no
 *              used pixel has nll0 = 0 and llr = 0 for every c.  A non-finite delta or error in a USED pixel makes that spectrum's
 *              nll0, llr and best_llr NaN and its best_c -1, and touches no other spectrum;
 *   outputs    llr (B, nc) and nll0 (B,) float32;  best_c (B,) int32 = the c of the largest llr of the row, the lowest c among
 *              equals, NaN never taken, -1 if every llr is NaN;  best_llr (B,) = that llr (NaN with -1).  best_c and best_llr may
 *              each be NULL;
 *   sums       no float atomics; two calls on the same inputs give the same bits.  A spectrum's row depends on that spectrum
 *              (and the table) alone, bit for bit: not on B, on the spectra beside it or on how the batch is cut into chunks.
 * qfa_template_scan_workspace_bytes: the images of F and of the table and the rows of one chunk of spectra (the batch is walked in
 * chunks whose rows stay below 256 MiB, four spectra at least); 0 = unsupported shape (B outside 1..2^24, Npix < 1, Nh outside
 * 1..32, nc outside 1..262 144).
 * Returns QFA_E_NULL for a missing pointer (p and its members, mu, b and its members as qfa_predict_f32 needs them, tau, V, llr,
 * nll0, workspace) or a non-NULL A_blue; QFA_E_SIZE for an unsupported shape, Nb outside 0..Npix or 0 < row_stride < Npix;
 * QFA_E_FLAGS for any flag but QFA_F_SYNC; QFA_E_WORKSPACE.  Argument checks return before any device work.  The call neither
 * synchronises nor allocates (graph-capturable).
 *
 * DLA templates.  qfa_dla_profiles_f32 fills the table of a grid of candidates that is the same in every quasar's rest frame:
 * Ly-alpha centres lam_i = lam_hi exp(-i dv_kms / c), i = 0 .. nz - 1, column densities logN_j = logn_lo + j dlogn, j = 0 .. nN - 1,
 * c = i nN + j, V_out (nz nN, Npix).  In spectrum s candidate i is an absorber at z_a = (1 + z_qso[s]) lam_i / 1215.67 - 1, and
 * lam_obs / (lam0 (1 + z_a)) = wav_grid[k] / (lam_i lam0 / 1215.67) does not depend on s.  tau and H(a, x) are those of
 * qfa_absorber_mask_f32's "profile", with x = (c / b) (wav_grid[k] / (lam_i lam0 / 1215.67) - 1): the same constants and three
 * ranges of P, Ly-alpha and under `lyb` Ly-beta, the same b_kms; float64 throughout, V = exp(-tau) rounded to float32 once.
 * Returns QFA_E_NULL; QFA_E_SIZE unless Npix >= 1, 1 <= nz <= 4096, 1 <= nN <= 64, lam_hi > 0, dv_kms >= 0, b_kms > 0, all finite,
 * and wav_grid[0] <= lam_i <= wav_grid[Npix - 1] for every i.  The last check reads the two ends of wav_grid on the host: this call
 * synchronises `stream` once (it is made once per grid, not per batch). */
int qfa_dla_profiles_f32(const double *wav_grid, int Npix, double lam_hi, double dv_kms, int nz, double logn_lo, double dlogn, int nN,
                         double b_kms, int lyb, float *V_out, void *stream);
size_t qfa_template_scan_workspace_bytes(int B, int Npix, int Nh, int nc);
int qfa_template_scan_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *V, int nc,
                          int B, int Npix, int Nb, int Nh, float *llr, float *nll0, int32_t *best_c, float *best_llr,
                          void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* The quasar-redshift finder: the likelihood of every spectrum under the model at 2 m + 1 integer pixel shifts (additive to ABI v4).
 * Every other call takes the catalogue redshift as exact; this one measures it.  On a rest-frame grid that is uniform in log
 * wavelength (step Delta in log10) a change of the redshift by one grid step is an integer shift between data and model pixels: no
 * interpolation, and the rule is exact.  The reference ships no such step.
 *
 * The rule.  Inputs per spectrum: x = b->delta the RAW FLUX, sigma = b->error, w = b->mask, zq1 = b->zq1 = 1 + z_cat (required when
 * Nb > 0: a (B, Nb) zabs cannot give z beyond Nb); shared: the model, mu, tau, pix_ratio_full[p] = wav_grid[p] / 1215.67 for ALL
 * Npix pixels, max_shift = m >= 0.  Candidates s = -m .. m (n_s = 2 m + 1, column c = s + m): candidate s says that data pixel p is
 * model pixel q = p + s, i.e. 1 + z_s = (1 + z_cat) 10^(-s Delta).
 *   window     the data pixels p in [m, Npix - m), the same for every candidate: every candidate explains the same data, n is
 *              common to all and the ratio is a likelihood ratio.  Pixels outside the window have weight 0;
 *   per pixel  z_p = fma(zq1[r], pix_ratio_full[p], -1) (one rounding, r = rows ? rows[s] : s) does not depend on s.  The pixel is
 *              blue iff q < Nb: there A = exp(-tau(z_p)), zd = (1 - c0 - exp(-tau0 (1 + z_p)^beta))^2; else A = 1, zd = 0.
 *              D = A^2 Psi_q + omega_q zd + sigma_p^2,  delta = x_p - A mu_q,  the factor row f_q;
 *   candidate  C = I + sum w/D A^2 f_q f_q^T,  b = sum w/D A delta f_q,
 *              NLL_s = ( sum w/D delta^2 - b^T C^-1 b + n log 2 pi + sum w log D + log det C ) / 2;
 *   arithmetic the per-pixel terms in float32; the sums of C and b on the matrix pipe (v_mfma_f32_16x16x4_f32) with float32
 *              accumulators over a block of 16 pixels, the blocks added in float64 in pixel order; sum w/D delta^2, sum w log D
 *              and n in float64 / integers; C factored in float64 (Cholesky) and NLL_s kept as a double;
 *   outputs    llr (B, n_s) float32 = NLL_0 - NLL_s, the difference taken in float64 before the one rounding: llr[:, m] == 0
 *              exactly;  nll0 (B,) float32 = NLL_0 (with m = 0 the window is the whole spectrum and nll0 is qfa_predict_f32's ll);
 *              best_s (B,) int32 = the s of the largest llr, among equals the lowest |s|, then the lowest s, NaN never taken;
 *              best_llr (B,) = that llr;  off, sig (B,) float64: with y-, y0, y+ the float32 llr at best_s - 1, best_s, best_s + 1
 *              and cv = (y- - y0) + (y+ - y0):  off = (y- - y+) / (2 cv), the vertex of the parabola in pixels relative to best_s,
 *              sig = 1 / sqrt(-cv);  both NaN where best_s = +-m or cv is not negative.  best_s, best_llr, off, sig may be NULL;
 *   masks      a masked pixel may hold NaN, inf or -999 in delta and error: they are not read.  A spectrum with no used pixel in
 *              the window has nll0 = 0, llr = 0, best_s = 0.  A non-finite delta or error in a USED pixel of the window makes that
 *              spectrum's nll0, llr and best_llr NaN and its best_s 0, and touches no other spectrum;
 *   sums       no atomics; two calls give the same bits, and a spectrum's row depends on that spectrum alone, bit for bit: not on B,
 *              on the spectra beside it or on how the batch is cut into chunks.
 * qfa_zscan_workspace_bytes: the images of F and of the model and the rows of one chunk of spectra (chunks whose rows stay below
 * 64 MiB, four spectra at least); 0 = unsupported shape (B outside 1..2^24, Nh outside 1..32, max_shift outside 0..4096,
 * Npix < 2 max_shift + 1).
 * Returns QFA_E_NULL for a missing pointer (p and its members, mu, b and its members as qfa_predict_f32 needs them, zq1 when Nb > 0,
 * tau, pix_ratio_full, llr, nll0, workspace) or a non-NULL A_blue; QFA_E_SIZE for an unsupported shape, Nb outside 0..Npix or
 * 0 < row_stride < Npix; QFA_E_FLAGS for any flag but QFA_F_SYNC; QFA_E_WORKSPACE.  Argument checks return before any device work.
 * The call neither synchronises nor allocates (graph-capturable). */
size_t qfa_zscan_workspace_bytes(int B, int Npix, int Nh, int max_shift);
int qfa_redshift_scan_f32(const qfa_params_t *p, const float *mu, const qfa_batch_t *b, const qfa_tau_t *tau, const float *pix_ratio_full,
                          int max_shift, int B, int Npix, int Nb, int Nh, float *llr, float *nll0, int32_t *best_s, float *best_llr,
                          double *off, double *sig, void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* The sightline bootstrap of the segment statistics (additive to ABI v4). The five calls above take their error bars from the scatter
 * of segments, but the segments of one quasar share a continuum, a noise model and a large-scale mode, and nothing but the band stack
 * gives a covariance between modes, lags, flux bins or z-bins.  The published measurements resample quasars.  These calls do that on
 * the per-segment rows the statistics already write (power, pairs, hist, bandpower, moments): R Poisson-bootstrap replicates of the
 * sums of the rows per draw and z-bin, from which qfa_amd.stacks.BootstrapStack forms the estimates and their covariance.
 *
 * qfa_segment_codes_f32 writes codes (B S, nseg) int32: entry (b S + s, g) is the z-bin kz of segment g of draw s of spectrum b when
 * the segment is valid and 0 <= kz < nz, else -1.  trans, ivar, b, tbar, B, S, Nb and p are qfa_p1d_f32's, bit for bit: `used` of a
 * pixel, n_used, validity (n_used >= min_used) and the z-bin (at the central pixel p_lo + g L + L / 2) are those of that call -- the
 * same device functions -- with its rules on the redshift forms and on NaN under the mask.  Returns every code of qfa_p1d_f32 for the
 * arguments they share (QFA_E_NULL also for codes, QFA_E_SIZE also for B S nseg above 2^31 - 1); checks return before any device work; B = 0 does nothing.
 *
 * The weight (the contract every port must reproduce).  Replicate r (0 <= r < R) gives the spectrum of global row g = row_offset + b
 * (int64) the weight w(seed, g, r) ~ Poisson(1), the same for all its segments and draws:
 *   generator  Philox4x32-10 as above, key = (seed & 0xffffffff, seed >> 32),
 *              counter = (0x40000000 | (r >> 2), 0, g & 0xffffffff, g >> 32) -> words x0..x3.  Bit 30 is set and bit 31 clear: disjoint
 *              from the latent stream (first word 0..7) and the mock stream (bit 31 set) under one seed;
 *   word       u = x[r & 3]: four consecutive replicates share one Philox call;
 *   weight     w = the number of thresholds T_k <= u, T_k = floor(2^32 sum_{i <= k} e^-1 / i!), k = 0 .. 12:
 *              0x5e2d58d8 0xbc5ab1b1 0xeb715e1d 0xfb239797 0xff1025f5 0xffd90f3b 0xfffa8b71 0xffff540c 0xffffed1f 0xfffffe21
 *              0xffffffd4 0xfffffffc 0xffffffff  (w <= 13).  Integer arithmetic only: identical on every device and in numpy.
 * The weight depends on (seed, g, r) alone -- not on the cut of a data set into calls, on the draw s, on R or on the rank.
 *
 * qfa_bootstrap_f64.  rows (B S, nseg, W) of row_type QFA_ROW_F32 / QFA_ROW_F64 / QFA_ROW_I32 -- row (b S + s, g) is segment g of draw s
 * of spectrum b, as the statistics write them; codes (B S, nseg) as qfa_segment_codes_f32 writes them (any value outside 0 .. nz - 1
 * puts the segment in no bin: its row is never read, NaN or inf in it reach nothing).
 *   output     boot (S, R, nz, 1 + W) float64 = [sum w | sum w x_0 .. x_{W-1}] over the segments of draw s with code kz.  The call ADDS
 *              to `boot`; QFA_F_ZERO_ACCUM overwrites instead;
 *   sums       x is converted to float64 (exact) and every term enters as fma(w, x, sum): w x is never rounded on its own (for
 *              float32 and int32 rows it is exact anyway, w <= 13), so the only roundings are those of the float64 additions --
 *              n_terms 2^-52 sum w |x| bounds the distance to the sum in any order.  Every element of boot is ONE chain of additions in order of (b, g) that starts from what `boot` holds
 *              (qfa_p1d_f32's rule: chunks of one segment): no atomics, two runs give the same bits, and calls on consecutive
 *              pieces of a batch -- the later ones adding, row_offset advanced -- give the bits of one call.  Replicate r does not
 *              depend on R, draw s not on S.  Sums over pieces added in another order (ranks, an all-reduce) differ by the rounding
 *              of float64 sums; int32 rows give integers, exact below 2^53 in any order.
 * qfa_bootstrap_workspace_bytes(n_spectra = B, ...): 0 = unsupported shape (B < 0, S < 1, nseg < 1, W or nz outside 1..4096, R outside
 * 1..65 536, B S nseg or S nz ceil((1 + W) / 4) above 2^31 - 1).  Nothing is held between kernels: the size of a supported shape is a
 * token 16 bytes.
 * Returns QFA_E_NULL for boot or ws missing; QFA_E_SIZE for an unsupported shape, row_offset < 0 or an unknown row_type; QFA_E_FLAGS
 * for any flag other than QFA_F_ZERO_ACCUM, QFA_F_SYNC; QFA_E_WORKSPACE; then QFA_E_NULL for rows or codes missing when B > 0.  B = 0
 * does nothing, except zeroing `boot` under QFA_F_ZERO_ACCUM.  Argument checks return before any device work.  Neither call
 * synchronises or allocates (graph-capturable). */
enum { QFA_ROW_F32 = 0, QFA_ROW_F64 = 1, QFA_ROW_I32 = 2 };

int qfa_segment_codes_f32(const float *trans, const float *ivar, const qfa_batch_t *b, const float *tbar, int B, int S, int Nb,
                          const qfa_p1d_t *p, int32_t *codes, void *stream);
size_t qfa_bootstrap_workspace_bytes(int n_spectra, int S, int nseg, int W, int nz, int R);
int qfa_bootstrap_f64(const void *rows, int row_type, const int32_t *codes, int B, int S, int nseg, int W, int nz, int R, uint64_t seed,
                      int64_t row_offset, unsigned flags, double *boot, void *ws, size_t ws_bytes, void *stream);

/* The observed-frame residual stack and the calibration it gives (additive to ABI v4).  Sky-line residuals, Galactic Ca H&K and the
 * spectrograph's flux-calibration residual spoil the same OBSERVED wavelengths of every spectrum, whatever its redshift.  Forest
 * analyses measure them from their own data: r = flux / continuum of every spectrum is stacked in bins of observed wavelength; the
 * stack's mean is the calibration vector, and bins whose scatter or mean stand out are the lines to mask (the intervals that
 * qfa_absorber_mask_f32 takes as obs_intervals).  qfa_forest_f32 stacks the blue side in at most 4096 float32 redshift bins; this
 * call stacks any pixel range -- the red side is where the calibration is measured -- in up to 32768 float64 bins, of which a
 * spectrum touches a contiguous run.
 *
 * The contract of qfa_obs_stack_f32.  For spectrum b of a call (row r = rows ? rows[b] : b of the input arrays), draw s (0 <= s < S)
 * and pixel p (p_lo <= p < p_hi, anywhere in 0 .. Npix):
 *   inputs     F, mu, b, h, unc exactly as qfa_forest_f32 reads them: b->delta holds the RAW FLUX, b->error the pipeline sigma,
 *              b->mask may be NULL (every pixel is used), rows / row_stride: the resident form; h (B, S, Nh) and unc (B, Npix) or NULL
 *              in batch order.  zabs, zq1, pix_ratio and A_blue are ignored.  pix_u (Npix,) float64, finite and NON-DECREASING
 *              (the caller checks; a run of a bin is found by bisection on it); spec_u (B,) float64 in batch order;
 *   coordinate float64, every operation rounded once, no contraction:  QFA_OBS_LOG  u = pix_u[p] + spec_u[b]  (the host passes
 *              log10(wav_grid) and log10(1 + z): both sides of every comparison share their bits);  QFA_OBS_LINEAR  u = pix_u[p]
 *              spec_u[b]  (the host passes wav_grid and 1 + z);  x = (u - u0) inv_du with inv_du = 1.0 / du formed once on the host;
 *              k = floor(x).  The pixel is stacked iff 0 <= x < nbin, tested on the double: an edge belongs to the bin above it.  A
 *              spectrum whose spec_u is not finite stacks nothing (a negative or zero linear spec_u is a coordinate like any other);
 *   values     those of qfa_forest_f32, verbatim, so that its bounds carry over:  c = mu[p] + sum_j F[p,j] h[b,s,j], the float32 fma
 *              chain in order of j;  r = flux / c;  den = (r r) u2 + sigma sigma with u2 = unc unc or 0;  iv = (c c) / den; every
 *              operation rounded once;
 *   use        mask != 0 && c > cont_min && isfinite(r) && isfinite(iv).  Selects, not products: what flux or error hold under the
 *              mask (-999, NaN, inf) reaches nothing.  NO transmission model is applied: on blue pixels the stack holds
 *              <T> x calibration, on red pixels the calibration alone;
 *   stack      (S, 4, nbin) float64 = [sum w | sum w r | sum w r^2 | n] per draw over the used, stacked pixels; w = (double)iv, or 1
 *              with QFA_F_OBS_UNIT_W; the terms are w, w r and w (r r) in float64, each product rounded once.  The call ADDS to
 *              `stack`; QFA_F_ZERO_ACCUM overwrites instead.  Nothing per pixel is written (qfa_forest_f32 writes the blue pixels);
 *   sums       no float atomics: a thread owns a bin and adds the pixels of its run spectrum by spectrum, in pixel order; chunks of
 *              spectra leave through rows of the workspace and a fixed-order reducer adds the rows to `stack`.  The cut is a function
 *              of the shape alone: two calls on the same inputs give the same bits.
 * qfa_obs_stack_doubles: S 4 nbin, 0 = unsupported (S < 1, nbin outside 1..32768).  qfa_obs_stack_workspace_bytes: the rows of partial
 * sums; 0 = unsupported shape.
 * Returns QFA_E_NULL for a missing required pointer (unc and b->mask may be NULL); QFA_E_SIZE for B < 0, S < 1, Npix < 1, Nh outside
 * 1..32, bad bins (du <= 0 or not finite, 1 / du or u0 not finite, nbin outside 1..32768, not 0 <= p_lo <= p_hi <= Npix, an unknown
 * mode) or 0 < row_stride < Npix; QFA_E_FLAGS for any flag other than QFA_F_ZERO_ACCUM, QFA_F_SYNC, QFA_F_OBS_UNIT_W;
 * QFA_E_WORKSPACE.  B = 0 or p_lo == p_hi adds nothing and, under QFA_F_ZERO_ACCUM, still zeroes `stack`.  Argument checks return
 * before any device work.  The call neither synchronises nor allocates (graph-capturable).
 *
 * The contract of qfa_calibrate_f32: divide spectra by a calibration table.  flux, error (N, Npix) float32 with the -999 sentinels (a
 * pixel is valid iff flux != -999 and error != -999, as for qfa_absorber_mask_f32); pix_u, spec_u (N,), mode, u0, du as above;
 * cal (ncal >= 2) float64 at the bin CENTRES u0 + (j + 0.5) du; c_min > 0.  Per pixel, in float64, every operation rounded once:
 *   x = (u - u0) inv_du - 0.5;  j = min(floor(x), ncal - 2);  f = x - j;  c = fma(f, cal[j + 1] - cal[j], cal[j]).
 * A pixel is calibrated iff it is valid, 0 <= x <= ncal - 1 and c is finite and >= c_min; it gets flux_out = (float)((double)flux / c)
 * and error_out = (float)((double)error / c).  Every other pixel keeps its input bits, sentinels included.  n_uncal (N,) int32 = the
 * number of VALID pixels left uncalibrated.  flux_out == flux and error_out == error (in place) is allowed; a spectrum's output
 * depends on that spectrum alone.  Returns QFA_E_SIZE for N < 0, Npix < 1, ncal < 2, du <= 0 or not finite, 1 / du or u0 not finite,
 * c_min <= 0 or not finite, an unknown mode; then N = 0 does nothing and returns 0; QFA_E_NULL for a missing pointer.  Argument
 * checks return before any device work.  The call neither synchronises nor allocates (graph-capturable). */
typedef struct { double u0, du; int nbin; int p_lo, p_hi; unsigned mode; } qfa_obs_bins_t;   /* du > 0, 1 <= nbin <= 32768, 0 <= p_lo <= p_hi <= Npix */
enum { QFA_OBS_LOG = 0, QFA_OBS_LINEAR = 1 };
#define QFA_F_OBS_UNIT_W 0x2000u   /* qfa_obs_stack_f32: stack with w = 1 instead of w = ivar */

size_t qfa_obs_stack_doubles(int S, int nbin);
size_t qfa_obs_stack_workspace_bytes(int B, int S, int Npix, int Nh, int nbin);
int qfa_obs_stack_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, const float *unc, const double *pix_u,
                      const double *spec_u, int B, int S, int Npix, int Nh, const qfa_obs_bins_t *bins, float cont_min,
                      unsigned flags, double *stack, void *workspace, size_t workspace_bytes, void *stream);
int qfa_calibrate_f32(const float *flux, const float *error, const double *pix_u, const double *spec_u, int N, int Npix,
                      const double *cal, int ncal, double u0, double du, unsigned mode, double c_min, float *flux_out,
                      float *error_out, int32_t *n_uncal, void *stream);

/* The BAL finder (additive to ABI v4): balnicity-type indices of r = flux / continuum in velocity windows blueward of emission lines
 * (BI: Weymann et al. 1991; AI: Hall et al. 2002, Trump et al. 2006), the list of trough velocities, and the mask made from them.
 * The continuum is the model's posterior continuum mu + F h on the RED side, per draw; no transmission model is applied, so a window
 * must lie at p_lo >= Nb.  qfa_amd.absorbers.bal_intervals turns the trough velocities back into rest-frame intervals.
 *
 * The contract of qfa_bal_scan_f32.  For spectrum b (row r = rows ? rows[b] : b of the input arrays), draw s, line l < n_lines:
 *   inputs     F, mu, b, h and cont_min exactly as qfa_obs_stack_f32 reads them (b->delta: RAW FLUX, b->error: the pipeline sigma,
 *              b->mask may be NULL, rows / row_stride: the resident form; h (B, S, Nh) in batch order).  No redshift is read.
 *   window     the pixels [p_lo[l], p_hi[l]), at most QFA_BAL_MAX_WIN of them, Nb <= p_lo <= p_hi <= Npix; n_win = p_hi - p_lo.  Window
 *              pixel i (0 = the lowest outflow velocity) is pixel p = p_hi - 1 - i and spans [vedge[i], vedge[i + 1]] km/s of
 *              v = c (1 - lambda / lambda_line), c = 299792.458.  vedge[l] (n_win + 1) float64 in DEVICE memory is the host's table,
 *              non-decreasing (the caller checks): centre velocities formed in float64, edges halfway between centres, extrapolated
 *              at the ends.  The kernel never forms a velocity: every width decision below is subtractions, one addition and min /
 *              max of float64 numbers of this table and of the index, the same operations on both sides of any comparison;
 *   pixel      c = mu[p] + sum_j F[p,j] h[b,s,j], the float32 fma chain in order of j;  r = flux / c;  iv = (c c) / (sigma sigma)
 *              (qfa_obs_stack_f32's with unc = NULL, except where r r overflows while r is finite: that call forms (r r) 0 = NaN and
 *              drops the pixel, this one keeps it);  used = mask != 0 && c > cont_min && isfinite(r) && isfinite(iv): selects, not
 *              products -- what flux or error hold under the mask reaches nothing;
 *   boxcar     `smooth` odd, 1..15, hw = smooth / 2:  r~_i = (sum of r_j over the USED j of [i - hw, i + hw] clipped to [0, n_win),
 *              float32, added in ascending j from 0) / (float)n_i, n_i the number of those j; defined where i itself is used.
 *              smooth = 1: r~ = r;
 *   below      used_i && (double)r~_i < thr;
 *   index      x < n_indices: {v_lo, v_hi, w_min, mode}.  Pixel i is IN THE DOMAIN iff min(vedge[i+1], v_hi) - max(vedge[i], v_lo) > 0.
 *              A BRIDGED pixel: max_gap (0..16) > 0, the pixel is unused and in the domain, and the maximal stretch of consecutive
 *              unused in-domain pixels it lies in has at most max_gap pixels and an in-domain `below` pixel directly on BOTH sides.
 *              A RUN is a maximal stretch of consecutive pixels that are in-domain-and-below or bridged (it starts and ends on a
 *              below pixel); any other pixel ends it.  first / last: its ends;  e0 = max(vedge[first], v_lo),
 *              e1 = min(vedge[last + 1], v_hi).
 *              QFA_BAL_WHOLE: the run qualifies iff e1 - e0 >= w_min; every below pixel of it contributes
 *                             width_i = min(vedge[i+1], v_hi) - max(vedge[i], v_lo).
 *              QFA_BAL_AFTER: a below pixel contributes width_i = max(0, min(vedge[i+1], v_hi) - max(vedge[i], e0 + w_min)); the
 *                             run qualifies iff some pixel contributes a positive width (equivalently, its last one does).
 *              Bridged pixels lengthen the run and contribute nothing;
 *   outputs    per (b, s, l, x):  value = sum_i (1 - (double)r~_i / thr) width_i over the pixels with width_i > 0, float64, each
 *              operation rounded once;  var = (sum_q (sigma_q / c_q)^2 a_q^2) / (thr thr), the exact noise variance of `value` under
 *              the pipeline sigma:  a_q = sum of width_i / (double)n_i over the used i of [q - hw, q + hw] with width_i > 0, in
 *              ascending i (a_q = width_q at smooth = 1), sigma_q / c_q the float32 quotient, squared in float64, over the used q
 *              with a_q > 0;  counts (B, S, n_lines, n_indices, 3) int32 = [n_pix: pixels with width_i > 0 | n_runs: qualifying
 *              runs | n_bridged: bridged pixels of qualifying runs].  value, var (B, S, n_lines, n_indices).
 *              per (b, s, l):  line_counts (B, S, n_lines, 2) int32 = [n_used: used pixels of the window | n_troughs: the TRUE
 *              number of qualifying runs of index `trough_index`];  troughs (B, S, n_lines, QFA_BAL_MAX_TROUGHS, 2) float64 = [e0, e1]
 *              of the first QFA_BAL_MAX_TROUGHS of them in order of velocity, NaN where unfilled;
 *   sums       float64, no atomics.  Lane m of the one wave that owns (b, l) adds the terms of its pixels i = m, m + 64, .. in ascending
 *              i; the 64 partial sums are added in the tree (m, m ^ 32), (m, m ^ 16), .., (m, m ^ 1).  The order is a function of the
 *              window alone: two calls give the same bits, draw s does not depend on S nor on how a call cuts the draws into groups,
 *              a spectrum's rows depend on that spectrum alone, and the resident form equals the gathered batch bit for bit.
 * There is no workspace.  Returns QFA_E_NULL for b == NULL or q == NULL or a missing vedge; QFA_E_SIZE for B < 0, S < 1, Npix < 1, Nb
 * outside 0..Npix, Nh outside 1..32, n_lines or n_indices outside 1..4, trough_index outside the indices, smooth even or outside 1..15,
 * max_gap outside 0..16, thr not positive and finite, a window with p_lo < Nb, p_lo > p_hi, p_hi > Npix or more than QFA_BAL_MAX_WIN
 * pixels, an index with v_lo >= v_hi, w_min < 0, anything not finite or an unknown mode, 0 < row_stride < Npix, B S n_lines above 2^30;
 * QFA_E_FLAGS for any flag other than QFA_F_SYNC; then B = 0 does nothing and returns 0; QFA_E_NULL for any other missing pointer
 * (b->mask may be NULL).  An empty window writes zeros and NaN troughs.  Argument checks
 * return before any device work.  The call neither synchronises nor allocates (graph-capturable).
 *
 * The contract of qfa_bal_mask_f32: the mask of the next predict -> find -> mask iteration, made on the device.  mask_in (B, Npix)
 * bytes (NULL: all set), wav (Npix,) float64 rest-frame wavelengths, troughs as qfa_bal_scan_f32 wrote them for S draws and n_lines
 * lines, mask_lines (n_mask_lines <= 4) float64 in HOST memory.  mask_out[b, p] = mask_in[b, p] && !inside, where inside holds iff
 *   lam (1 - (v_max + pad) / c) <= wav[p] < lam (1 - (v_min - pad) / c)
 * for some filled trough [v_min, v_max] of draw s_ref of spectrum b (any of its lines) and some lam of mask_lines: float64, the sum or
 * difference with pad, the division, the subtraction and the product each rounded once, never contracted -- the operations of
 * bal_intervals(v_min - pad, v_max + pad), so the result equals bal_intervals -> qfa_absorber_mask_f32's rest intervals.  n_masked
 * (B,) int32 = the pixels of mask_in that the call cleared.  mask_out == mask_in (in place) is allowed.  Returns QFA_E_SIZE for B < 0,
 * S < 1, Npix < 1, n_lines or n_mask_lines outside 1..4, s_ref outside 0..S-1, pad_kms negative or not finite, a line not positive and
 * finite; QFA_E_NULL for mask_lines == NULL; then B = 0 does nothing and returns 0; QFA_E_NULL for any other missing pointer.  Argument
 * checks return before any device work.  The call neither synchronises nor allocates (graph-capturable). */
#define QFA_BAL_MAX_LINES 4
#define QFA_BAL_MAX_INDICES 4
#define QFA_BAL_MAX_TROUGHS 8
#define QFA_BAL_MAX_WIN 2048
enum { QFA_BAL_WHOLE = 0, QFA_BAL_AFTER = 1 };
typedef struct { double v_lo, v_hi, w_min; unsigned mode; } qfa_bal_index_t;   /* BI = {3000, 25000, 2000, AFTER}, AI = {0, 25000, 450, WHOLE} */
typedef struct {
    int n_lines, n_indices;
    int p_lo[QFA_BAL_MAX_LINES], p_hi[QFA_BAL_MAX_LINES];
    const double *vedge[QFA_BAL_MAX_LINES];      /* device, (p_hi - p_lo + 1) each */
    qfa_bal_index_t index[QFA_BAL_MAX_INDICES];
    double thr;
    int smooth, max_gap, trough_index;
} qfa_bal_t;

int qfa_bal_scan_f32(const float *F, const float *mu, const qfa_batch_t *b, const float *h, int B, int S, int Npix, int Nb, int Nh,
                     const qfa_bal_t *q, float cont_min, unsigned flags, double *value, double *var, int32_t *counts,
                     int32_t *line_counts, double *troughs, void *stream);
int qfa_bal_mask_f32(const unsigned char *mask_in, const double *wav, const double *troughs, int B, int S, int n_lines, int s_ref,
                     int Npix, const double *mask_lines, int n_mask_lines, double pad_kms, unsigned char *mask_out, int32_t *n_masked,
                     void *stream);

/* Replaces Adam.update(reference QFA/optimizer.py:37-52) followed by the clamp of QFA.clip
 * (QFA/model.py:233-241) for ONE tensor of n elements:
 *   g' = g + wd*p; m = (1-b1) g' + b1 m; v = (1-b2) g'^2 + b2 v;
 *   p_out = clamp(p - lr * (m/bc1) / (sqrt(v/bc2) + eps), lo, hi),  bc = 1 - b^(i+1),
 * with i = Adam.i (advanced by Adam.step(), once per epoch in QFA.train).  The hyper-parameters
 * are doubles because the reference holds them as Python floats and rounds (1-b), b^(i+1) etc.
 * to float32 only when they meet a tensor.  m and v are updated in place; pass lo > hi to skip
 * the clamp.  NaN propagates as in torch.  One departure from the reference's float32: where v/bc2 overflows although v is
 * finite (|g| beyond ~1e18 while bc2 is small) the root is formed as sqrt(v)/sqrt(bc2), so the element still moves by about
 * lr as in exact arithmetic; the reference's inf leaves it where it is.  n = 0 does nothing and returns 0. */
int qfa_adam_clip_f32(const float *p, const float *g, float *m, float *v, float *p_out, size_t n,
                      double lr, double b1, double b2, double eps, double wd, int i,
                      float lo, float hi, void *stream);

/* Adam.update + clip for up to QFA_ADAM_MAX tensors in ONE launch (reference QFA/optimizer.py:37-52 loops over the
 * parameter dict, QFA/model.py:233-241 clips each entry): same arithmetic as qfa_adam_clip_f32 per tensor.
 * lo[k] > hi[k] disables the clip of tensor k; p_out[k] may equal p[k] (in place). */
#define QFA_ADAM_MAX 8
typedef struct {
    const float *p[QFA_ADAM_MAX];
    const float *g[QFA_ADAM_MAX];
    float *m[QFA_ADAM_MAX];
    float *v[QFA_ADAM_MAX];
    float *p_out[QFA_ADAM_MAX];
    size_t n[QFA_ADAM_MAX];
    float lo[QFA_ADAM_MAX], hi[QFA_ADAM_MAX];
    int count;
} qfa_adam_multi_t;
int qfa_adam_clip_multi_f32(const qfa_adam_multi_t *t, double lr, double b1, double b2, double eps, double wd, int i,
                            void *stream);

/* qfa_finalize_grads_f32 (normalised) followed by qfa_adam_clip_multi_f32 for the six parameter tensors in ONE launch -- the
 * reference's `loss, grad = self.forward(...); self.parameters = optimizer.update(self.parameters, grad)` (QFA/model.py:212-214)
 * without the gradients in between.  `t` holds the tensors in the order F, Psi, omega, tau0, c0, beta (count = 6; its `g`
 * pointers are not read); the gradient of every element is formed from `accum` with k_finalize's arithmetic and fed to
 * qfa_adam_clip_multi_f32's: the new parameters are bit-identical to the two calls.  loss (1 float) = sum NLL / n_spectra. */
int qfa_finalize_adam_clip_f32(const float *accum, int Npix, int Nb, int Nh, const qfa_adam_multi_t *t, double lr, double b1,
                               double b2, double eps, double wd, int i, float *loss, void *stream);

/* Replaces QFA.clip for one tensor (reference QFA/model.py:233-241): y = clamp(x, lo, hi), NaN kept. */
int qfa_clip_f32(const float *x, float *y, size_t n, float lo, float hi, void *stream);

/* Replaces QFA.smooth (reference QFA/model.py:243-252): edge-aware moving average of
 * (2*half+1) rows along axis 0 of an (n, cols) array, divisor = in-range sample count. */
int qfa_smooth_f32(const float *x, float *y, int n, int cols, int half, void *stream);

/* Replace tau(), tauHI(), omega_func() (reference QFA/utils.py:57-92, 149-171), elementwise on n.
 * For every elementwise entry point (these three, qfa_clip_f32, qfa_smooth_f32, qfa_adam_clip_f32) n = 0 does nothing and
 * returns 0 whatever the pointers are: an empty torch tensor (N_b = 0) has a NULL data pointer. */
int qfa_tau_f32(const float *z, float *out, size_t n, const qfa_tau_t *tau, void *stream);
int qfa_tauhi_f32(const float *z, const float *tau0, const float *beta, float *out, size_t n,
                  void *stream);
int qfa_omega_func_f32(const float *z, const float *tau0, const float *beta, const float *c0,
                       float *out, size_t n, void *stream);

/* Device-side batch builder.  Replaces what Dataloader.next_batch / __init__ do
 * on the host with numpy (reference QFA/dataloader.py:29,102,124-138 and tau_total, QFA/utils.py:174-203):
 * for row r of the batch, spectrum s = idx ? idx[r] : r of the resident flux/error arrays (N rows, row_stride elements
 * apart; 0 = Npix),
 *   zabs  = (1+zqso) wav_blue / 1215.67 - 1,  delta = flux - mu * exp(-tau_total) (blue) | flux - mu (red),
 *   mask  = (flux != -999) & (error != -999),  error_out = error[s].
 * float64 arithmetic like numpy, outputs (contiguous, batch order) rounded to float32 once.  wav0 = wav[0] (host copy). */
int qfa_build_batch_f32(const float *flux, const float *error, const double *zqso, const int *idx,
                        const double *wav, double wav0, const double *mu, int which, int nrow, int Npix,
                        int Nb, int64_t row_stride, float *delta, float *error_out, float *zabs, uint8_t *mask,
                        void *stream);

/* The resident form of a whole data set, built ONCE per loader instead of once per batch (ABI v3; the reference
 * recomputes delta for every batch, QFA/dataloader.py:135-136, although it depends on mu and tau only): for every
 * row r < nrow of flux / error (rows row_stride >= Npix elements apart)
 *   delta[r] = flux - mu * exp(-tau_total) (blue) | flux - mu (red),  mask[r] = (flux != -999) & (error != -999),
 * written with the SAME row stride (pad pixels: 0 / masked), and zq1[r] = (float)(1 + zqso[r]).  The same arithmetic as
 * qfa_build_batch_f32: a batch of the resident form -- qfa_batch_t{delta, error, mask, zq1, pix_ratio, rows, row_stride} --
 * holds bit for bit the numbers the materialised batch of the same rows holds. */
int qfa_build_resident_f32(const float *flux, const float *error, const double *zqso, const double *wav, double wav0,
                           const double *mu, int which, int64_t nrow, int Npix, int Nb, int64_t row_stride,
                           float *delta, uint8_t *mask, float *zq1, void *stream);

/* ABI v4.  Does a caller's zabs (B, Nb) have the structure the reference's loader gives it -- 1 + zabs[s][i] =
 * (1 + z_qso[s]) wav_i / 1215.67 (reference QFA/dataloader.py:102) -- so that the factored-z input form (qfa_batch_t::zq1 /
 * pix_ratio above) may stand in for it?  Writes zq1[s] = 1 + zabs[s][0] (B floats) and pix_ratio[i] = (1 + zabs[0][i]) /
 * (1 + zabs[0][0]) (Nb floats; the quotient in float64, rounded once) and counts in *nbad (device memory, zeroed by the call)
 * the elements with |(1 + zabs[s][i]) - zq1[s] pix_ratio[i]| > tol (1 + zabs[s][i]) (a NaN counts).  nbad == 0: every 1 + z the
 * factored kernels form is within tol (relative) of the one the zabs kernels read -- at tol = 4e-7 (three float32 roundings) the
 * results agree as the two forms of one loader's batch do (tests/test_hip_parity.py).  One pass over zabs: B Nb 4 bytes read.
 * Asynchronous like every entry point: the caller reads *nbad behind the stream. */
int qfa_zabs_factor_f32(const float *zabs, int B, int Nb, float tol, float *zq1, float *pix_ratio, unsigned *nbad,
                        void *stream);

/* Replaces the continuum-mean estimate of Dataloader.__init__ (reference QFA/dataloader.py:110-112):
 * mu_raw = sum_s flux exp(+tau_total) mask / #(flux != -999); mu_smooth = reflect-padded boxcar of
 * window_len (QFA/utils.py:206-219; may be NULL).  scratch: 2*Npix doubles.  flux / error rows row_stride elements apart
 * (0 = Npix). */
int qfa_mu_estimate_f64(const float *flux, const float *error, const double *zqso, const double *wav,
                        double wav0, int which, int B, int Npix, int Nb, int64_t row_stride, int window_len,
                        double *scratch, double *mu_raw, double *mu_smooth, void *stream);

/* The two halves of qfa_mu_estimate_f64 for a data-parallel loader (each rank holds a shard of the
 * spectra): qfa_mu_sums_f64 ADDS this shard's per-pixel sums to scratch = [num Npix | den Npix]
 * (caller zeroes it), the caller all-reduces scratch over the ranks, qfa_mu_finish_f64 divides and
 * smooths.  Same arithmetic as the one-call form. */
int qfa_mu_sums_f64(const float *flux, const float *error, const double *zqso, const double *wav,
                    double wav0, int which, int B, int Npix, int Nb, int64_t row_stride, double *scratch,
                    void *stream);
int qfa_mu_finish_f64(const double *scratch, int Npix, int window_len, double *mu_raw, double *mu_smooth,
                      void *stream);

/* Replace MatrixInverse / MatrixLogDet (reference QFA/utils.py:12-54) for one (n,k) M and (n,) D:
 * inv (n,n) dense, logdet scalar (Cholesky-free Gauss-Jordan on the k x k core, finite where the
 * reference's float32 det overflows). workspace: qfa_workspace_bytes(1, n, k). */
int qfa_woodbury_f32(const float *M, const float *D, int n, int k, float *inv, float *logdet,
                     void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QFA_HIP_H */
