"""Float64 closed form of the EM update of the factor loadings F (QFA.em_statistics / em_update_F, include/qfa_hip.h
qfa_em_stats_f32 / qfa_em_update_f_f32), in the notation of DESIGN.md sections 2 and 14.

Per spectrum s at the current parameters: wD = mask / D, C = I + sum_i wD A^2 f f^T, y = C^-1 b, E_s = C^-1 + y y^T.  Then
    S2_i = sum_s wD_si A_si^2 E_s      S1_i = sum_s wD_si A_si delta_si y_s      cnt_i = sum_s mask_si
    F_i <- F_i + damping ((S2_i + ridge I)^-1 S1_i - F_i)        rows with cnt_i = 0 stay as they are
and S2_i f_i - S1_i is the exact-mode gradient d(sum_s NLL_s)/df_i (tests/_exact_ref.py).

The element judge of tests/test_em_elements.py lives here as well (a whole-tensor norm does not see one
wrong element, least of all at a pixel whose weights wD = mask / D are small): ``em_terms`` restates the statistics as matrix
products over the spectra and returns the sums of |terms| next to them, ``stat_units`` reads an element's error in units of its
own sum of |terms|, ``solve_rows`` is the M-step row by row on GIVEN float32 statistics with the kernel's skip rule and the
derived bar of ``solve_bar``.  The inputs and the case table of the GPU tests are here too, so that tools/em_bars.py (which
measures the statistics' bars, profiles/em_accuracy.txt) and the CPU tests see exactly what the GPU tests see.
"""
from __future__ import annotations

import numpy as np

from oracle import qfa_oracle as orc


def em_statistics(params, delta, error, zabs, mask, tau_which="becker", A_blue=None, tau_series=1):
    """Batch sums: dict S2 (Npix, Nh, Nh), S1 (Npix, Nh), cnt (Npix,), nll_sum, n, nll (B,)."""
    p = orc._as_params(params, np.float64)
    F = p["F"]
    npix, nh = F.shape
    S2 = np.zeros((npix, nh, nh))
    S1 = np.zeros((npix, nh))
    cnt = np.zeros(npix)
    nlls = np.zeros(len(delta))
    for s in range(len(delta)):
        w = np.asarray(mask[s], dtype=bool)
        A, _, D = orc.pixel_terms(params, error[s], zabs[s], tau_which, tau_series, np.float64,
                                  None if A_blue is None else A_blue[s])
        wD, d, _, C, y, _, nll = orc._lowrank_core(F, A, D, w, np.asarray(delta[s], dtype=np.float64))
        E = np.linalg.inv(C) + np.outer(y, y)
        S2 += (wD * A * A)[:, None, None] * E[None, :, :]
        S1 += (wD * A * d)[:, None] * y[None, :]
        cnt += w
        nlls[s] = nll
    return {"S2": S2, "S1": S1, "cnt": cnt, "nll_sum": float(nlls.sum()), "n": float(len(delta)), "nll": nlls}


def em_update(F, st, ridge=0.0, damping=1.0):
    """(new F, number of rows skipped): rows with cnt = 0 or a system that is not positive definite are kept."""
    F = np.asarray(F, dtype=np.float64)
    out = F.copy()
    nh = F.shape[1]
    skipped = 0
    for i in range(F.shape[0]):
        if not st["cnt"][i] > 0:
            skipped += 1
            continue
        try:
            L = np.linalg.cholesky(st["S2"][i] + ridge * np.eye(nh))
        except np.linalg.LinAlgError:
            skipped += 1
            continue
        x = np.linalg.solve(L.T, np.linalg.solve(L, st["S1"][i]))
        out[i] = F[i] + damping * (x - F[i])
    return out, skipped


def em_step(params, delta, error, zabs, mask, ridge=0.0, damping=1.0, tau_which="becker", tau_series=1):
    """(mean NLL at `params`, params with the updated F, statistics, rows skipped)"""
    st = em_statistics(params, delta, error, zabs, mask, tau_which, tau_series=tau_series)
    newF, skipped = em_update(params["F"], st, ridge, damping)
    q = dict(params)
    q["F"] = newF
    return st["nll_sum"] / st["n"], q, st, skipped


# ----------------------------------------------------------------------------------------------------------------------
# the element judge of the statistics
# ----------------------------------------------------------------------------------------------------------------------
def pair_indices(nh):
    """(a, b) of the packed upper triangle, row-major"""
    return np.triu_indices(nh)


def em_terms(params, delta, error, zabs, mask, tau_which="becker", A_blue=None, dtype=np.float64, tau_series=1):
    """``em_statistics`` restated as two matrix products over the spectra, after the per-spectrum E-step of the oracle:
    S2 = W2^T (Npix x B) @ E (B x pairs of N_h), S1 = W1^T @ Y with W2 = wD A^2, W1 = wD A delta -- and the same products of the
    absolute values: absS2[i, a, b] = sum_s |beta_si E_s[a, b]|, absS1[i, a] = sum_s |gamma_si y_s[a]|, the scale an element's
    error is read in (``stat_units``).  ``dtype=np.float32``: the whole restatement in float32 (E-step, weights, products),
    which is what the bars are measured with.  dict S2, S1, absS2, absS1 (``dtype``), cnt, nll (B,), nll_sum, n."""
    dtype = np.dtype(dtype).type
    p = orc._as_params(params, dtype)
    F = p["F"]
    npix, nh = F.shape
    B = len(delta)
    ia, ib = pair_indices(nh)
    W2 = np.zeros((B, npix), dtype)
    W1 = np.zeros((B, npix), dtype)
    EP = np.zeros((B, len(ia)), dtype)
    Y = np.zeros((B, nh), dtype)
    nlls = np.zeros(B)
    cnt = np.zeros(npix)
    for s in range(B):
        w = np.asarray(mask[s], dtype=bool)
        A, _, D = orc.pixel_terms(params, error[s], zabs[s], tau_which, tau_series, dtype, None if A_blue is None else A_blue[s])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):      # (junk under the mask: selected away)
            wD, d, _, C, y, _, nll = orc._lowrank_core(F, A, D, w, np.asarray(delta[s], dtype=dtype))
        E = np.linalg.inv(C) + np.outer(y, y)
        W2[s] = wD * A * A
        W1[s] = wD * A * d
        EP[s] = E[ia, ib]
        Y[s] = y
        nlls[s] = nll
        cnt += w
    def unpack(P):
        out = np.zeros((npix, nh, nh), dtype)
        out[:, ia, ib] = P
        out[:, ib, ia] = P
        return out
    return {"S2": unpack(W2.T @ EP), "S1": W1.T @ Y, "absS2": unpack(np.abs(W2).T @ np.abs(EP)),
            "absS1": np.abs(W1).T @ np.abs(Y), "cnt": cnt, "nll": nlls, "nll_sum": float(nlls.sum()), "n": float(B)}


def stat_units(ours, ref, abssum):
    """|ours - ref| / abssum per element.  An element without a term (abssum 0) must be exactly 0 in ``ours``: it reads 0 then,
    inf otherwise; NaN or inf on one side only reads inf (the convention of ``_elementwise_ref.grad_error_units``)."""
    ours, ref = np.asarray(ours, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    abssum = np.asarray(abssum, dtype=np.float64)
    assert ours.shape == ref.shape == abssum.shape, (ours.shape, ref.shape, abssum.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.abs(ours - ref) / abssum
    empty = abssum == 0
    u[empty] = np.where(ours[empty] == 0, 0.0, np.inf)
    u[np.isfinite(ours) != np.isfinite(ref)] = np.inf
    return u


def worst_element(units):
    """(index tuple, value) of the largest entry; NaN reads as the largest of all"""
    u = np.where(np.isnan(units), np.inf, units)
    idx = np.unravel_index(int(np.argmax(u)), u.shape)
    return tuple(int(i) for i in idx), float(u[idx])


# The bars of S2 and S1 in units of an element's sum of |terms| (profiles/em_accuracy.txt): 8 x the worst value of the float32
# restatement ``em_terms(dtype=np.float32)`` against the float64 one over exactly ELEMENT_CASES below, which
# tools/em_bars.py prints.  The margin of 8 is that of tests/_elementwise_ref.py: the kernels sum in another order, use
# fast_rcp and the hardware's exp / log, and take E_s from split-16-bit products.
#
# (pixels that two and more spectra see, pixels that ONE spectrum sees).  A single term beta E_s[a, b] is itself a sum that
# cancels -- E_s = C_s^-1 + y_s y_s^T, y_s = C_s^-1 b_s -- and sum|terms| does not see a cancellation INSIDE a term: where many
# terms are summed the few cancelled ones weigh little next to sum|terms|, where one is, nothing does.  The float32 restatement
# reads 1.1e-4 there against 1.9e-6, so, as in _elementwise_ref.GRADIENT_BARS, the one-term pixels get a bar of their own and
# the dense ones keep the 60 x tighter one.
STAT_BARS = {"S2": (8 * 1.85e-6, 8 * 1.14e-4), "S1": (8 * 8.22e-7, 8 * 9.39e-5)}


def class_worst(units, cnt):
    """((worst units, element) over the pixels with cnt >= 2 -- and cnt 0, which must be exact zeros --, the same over the
    pixels with cnt = 1)"""
    single = np.asarray(cnt) == 1
    out = []
    for cls in (~single, single):
        sel = np.broadcast_to(cls.reshape((-1,) + (1,) * (units.ndim - 1)), units.shape)
        if not sel.any():
            out.append((0.0, ()))
            continue
        idx, w = worst_element(np.where(sel, units, -1.0))
        out.append((w, idx))
    return tuple(out)


def check_stat_elements(S2, S1, cnt, ref, what="", bars=None):
    """Every element of S2 and S1 under its bar, cnt exact.  ``ref``: ``em_terms`` in float64, or the sum of several batches'
    (S2, S1, absS2, absS1, cnt).  Returns {"S2": ((worst units, element) of the dense pixels, the same of the one-term pixels),
    "S1": ...}; raises AssertionError naming the element."""
    bars = STAT_BARS if bars is None else bars
    cnt = np.asarray(cnt, dtype=np.float64)
    bad = np.flatnonzero(cnt != ref["cnt"])
    assert bad.size == 0, f"{what}: cnt of pixel {bad[0]} is {cnt[bad[0]]:.0f}, the reference counts {ref['cnt'][bad[0]]:.0f}"
    out = {}
    for k, ours in (("S2", S2), ("S1", S1)):
        ours = np.asarray(ours, dtype=np.float64)
        out[k] = class_worst(stat_units(ours, ref[k], ref["abs" + k]), ref["cnt"])
        for (w, idx), bar in zip(out[k], bars[k]):
            assert w <= bar, f"{k} {what}: element {idx} is {w:.3e} of its sum of |terms| from float64 (bar {bar:.2e}); " \
                             f"cnt {ref['cnt'][idx[0]]:.0f}, ours {ours[idx]!r}, float64 {ref[k][idx]!r}"
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the M-step, row by row
# ----------------------------------------------------------------------------------------------------------------------
def split_stats(buf, npix, nh):
    """(S2, S1, cnt) views of a flat statistics buffer [S2 | S1 | cnt | tail of 4]"""
    buf = np.asarray(buf)
    n2, n1 = npix * nh * nh, npix * nh
    return buf[:n2].reshape(npix, nh, nh), buf[n2:n2 + n1].reshape(npix, nh), buf[n2 + n1:n2 + n1 + npix]


def solve_rows(stats_f32, F, ridge, damping):
    """The M-step of qfa_em_update_f_f32 in float64 on GIVEN float32 statistics (``stats_f32``: (S2, S1, cnt)), so that nothing
    but the solve separates it from the kernel: per row numpy.linalg.cholesky of S2_i + ridge I (the lower triangle, which is
    all the kernel reads either), two triangular solves, F_i + damping (x_i - F_i).  The skip rule is the kernel's: cnt not > 0,
    a pivot not > 0 (numpy's LinAlgError, a non-finite factor), a pivot not < 1e300, a solution that is not finite.
    Returns (new F float64 with skipped rows = F, skipped (Npix,) bool, cond_2(S2_i + ridge I) per row -- NaN where skipped --,
    x (Npix, Nh): the solutions before the damping)."""
    S2, S1, cnt = (np.asarray(a) for a in stats_f32)
    assert S2.dtype == np.float32 and S1.dtype == np.float32
    F = np.asarray(F, dtype=np.float64)
    npix, nh = F.shape
    out, skipped = F.copy(), np.zeros(npix, bool)
    cond, xs = np.full(npix, np.nan), np.full((npix, nh), np.nan)
    for i in range(npix):
        skipped[i] = True
        if not cnt[i] > 0:
            continue
        A = np.tril(S2[i].astype(np.float64)) + ridge * np.eye(nh)
        A = A + np.tril(A, -1).T
        if not np.isfinite(A).all():                     # reaches a pivot as NaN or -inf; +inf on the diagonal: not < 1e300
            continue
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        piv = np.diag(L) ** 2
        if not (np.all(piv > 0) and np.all(piv < 1e300)):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            z = _tri_solve(L, S1[i].astype(np.float64), lower=True)
            x = _tri_solve(L.T, z, lower=False)
        if not np.isfinite(x).all():
            continue
        skipped[i] = False
        xs[i] = x
        cond[i] = np.linalg.cond(A, 2)
        out[i] = F[i] + damping * (x - F[i])
    return out, skipped, cond, xs


def _tri_solve(T, b, lower):
    n = len(b)
    x = np.array(b, dtype=np.float64)
    order = range(n) if lower else range(n - 1, -1, -1)
    for j in order:
        x[j] = x[j] / T[j, j]
        if lower:
            x[j + 1:] -= T[j + 1:, j] * x[j]
        else:
            x[:j] -= T[:j, j] * x[j]
    return x


def solve_bar(F_ref, x, cond, nh, damping):
    """The bar of |F_gpu - F_ref| per element, derived -- no measured number in it:

        2^-24 |F_ref|  +  |damping| c N_h cond_i 2^-53 ||x_i||_inf          c = 2 (3 N_h + 2) sqrt(N_h)

    First term: the kernel rounds its float64 result to float32 once (half an ulp).  Second term: both sides solve
    A x = b, A = S2_i + ridge I, by Cholesky and two triangular solves in float64 (u = 2^-53).  The computed solution of that
    algorithm solves (A + dA) x^ = b exactly with |dA| <= gamma_(3n+1) |R^T| |R| (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., theorem 10.4); the kernel scales a column by the reciprocal of its pivot's root, one more rounding per
    element of the factor: gamma_(3n+2), and gamma_k = k u / (1 - k u).  With || |R^T| |R| ||_2 <= n ||A||_2 (ibid. (10.7)) the
    backward error is ||dA||_2 <= n (3n + 2) u ||A||_2 and the forward error
    ||x^ - x||_2 <= cond_2(A) n (3n + 2) u ||x||_2 to first order.  An element's error is at most the 2-norm, and
    ||x||_2 <= sqrt(n) ||x||_inf: |x^_k - x_k| <= n (3n + 2) sqrt(n) cond_2(A) u ||x||_inf -- for EACH of the two sides, hence
    the 2 in c.  The update F + damping (x - F) carries the difference of the two solutions over times |damping|; its own
    float64 roundings are the same expression on both sides."""
    c = 2.0 * (3 * nh + 2) * np.sqrt(nh)
    xinf = np.max(np.abs(x), axis=1)
    return 2.0 ** -24 * np.abs(F_ref) + (abs(damping) * c * nh * cond * 2.0 ** -53 * xinf)[:, None]


SOLVE_NH = (1, 2, 5, 16, 17, 31, 32)
SOLVE_NPIX = (1, 3, 5, 64, 130)
SOLVE_RIDGE_DAMPING = ((0.0, 1.0), (0.3, 1.0), (0.0, 0.4), (2.0, 0.7), (0.0, 0.0), (0.0, 1.5), (0.0, -0.5))
# rows planted among good ones where the pixel axis has room (N_pix >= 64), one per position inside a block of four rows
PLANTED = {"cnt0": 5, "negated": 10, "rank": 19, "nan": 28, "inf": 33}


def solve_case(npix, nh, seed=None):
    """Hand-built float32 statistics and F of the solve test: (S2, S1, cnt, F, planted {name: row}).  S2_i = Q diag(lambda) Q^T
    with cond log-uniform in [1, 1e6] per row, rounded to float32 and symmetrised; random S1 and F.  Planted rows (``PLANTED``;
    on a short pixel axis only a cnt = 0 row at the end of N_pix = 5 and a NaN row in the middle of N_pix = 3): cnt = 0; S2_i
    negated; a zero pivot at the last column only -- S2_i = L L^T of small integers with L[-1, -1] = 0, every operation of the
    factorisation exact in float32 and float64 --; a NaN off the diagonal; +inf in S1_i (every pivot positive, the solution
    is not finite)."""
    rng = np.random.default_rng(1000 * npix + nh if seed is None else seed)
    S2 = np.empty((npix, nh, nh), np.float32)
    for i in range(npix):
        Q, _ = np.linalg.qr(rng.standard_normal((nh, nh)))
        lam = np.ones(nh)
        if nh > 1:
            c = 10.0 ** rng.uniform(0.0, 6.0)                            # the row's condition number
            lam = c ** -rng.uniform(0.0, 1.0, size=nh)
            lam[0], lam[-1] = 1.0, 1.0 / c
        lam = lam * 10.0 ** rng.uniform(-1.0, 2.0)                       # and its scale
        M = ((Q * lam) @ Q.T).astype(np.float32)
        S2[i] = np.tril(M) + np.tril(M, -1).T
    S1 = rng.standard_normal((npix, nh)).astype(np.float32)
    cnt = rng.integers(1, 50, size=npix).astype(np.float32)
    F = rng.uniform(-0.5, 0.5, size=(npix, nh)).astype(np.float32)
    planted = {}
    if npix >= 64:
        planted = dict(PLANTED)
        if npix % 4:
            planted["cnt0_last"] = npix - 1              # in the ragged last block
    elif npix == 5:
        planted = {"cnt0_last": 4}
    elif npix == 3:
        planted = {"nan": 1}
    for name, i in planted.items():
        if name.startswith("cnt0"):
            cnt[i] = 0.0
        elif name == "negated":
            S2[i] = -S2[i]
        elif name == "rank":
            L = np.tril(rng.integers(-2, 3, size=(nh, nh))).astype(np.float64)
            L[np.arange(nh), np.arange(nh)] = rng.choice([1.0, 2.0], size=nh)
            L[-1, -1] = 0.0
            S2[i] = (L @ L.T).astype(np.float32)
            assert np.array_equal(S2[i].astype(np.float64), L @ L.T)
        elif name == "nan":
            if nh > 1:
                S2[i, nh - 1, 0] = S2[i, 0, nh - 1] = np.nan
            else:
                S2[i, 0, 0] = np.nan                       # (N_h = 1 has no off-diagonal)
        elif name == "inf":
            S1[i, nh // 2] = np.inf
    return S2, S1, cnt, F, planted


# ----------------------------------------------------------------------------------------------------------------------
# the inputs and the cases of the GPU tests
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [  # (npix, nh, B): every N_h class, ragged pixel axes (N_pix = 1 included), B from 1 to 4 096
    (1, 1, 5), (37, 1, 1), (203, 4, 70), (333, 8, 257), (97, 8, 4096), (501, 16, 130), (75, 16, 1030), (211, 17, 33),
    (130, 32, 300), (45, 5, 2), (1030, 12, 64),
]


def em_inputs(npix, nh, B, seed, random_F=True, junk=True, batch_seed=None, plant=None):
    """(p, b, dead, wav, nb, zfac) in numpy: masks on, one red-only spectrum, one pixel range masked in every spectrum, NaN / inf /
    -999 under the masks; F ~ U(-0.5, 0.5) like random_init_func.  ``batch_seed``: another batch at the same parameters
    (default seed + 1).  ``plant(mask)`` may clear further elements of the mask before the junk goes under it.  ``zfac``: the
    float32 factors (1 + z_qso, lambda / Ly-alpha) of the factored-z input form."""
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    bseed = seed + 1 if batch_seed is None else batch_seed
    dead = (npix // 3, min(npix, npix // 3 + 3)) if npix >= 8 else None
    # (a pixel axis shorter than a mask run would be masked whole: such shapes get the per-pixel 1 % masks only below)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=bseed, masks=npix >= 32,
                                   red_only=(0,) if (B > 2 and 0 < nb < npix) else (), dead_range=dead)
    if npix < 32 and B > 1:
        b["mask"][1::3, ::2] = False
        for k in ("flux", "error"):
            b[k] = np.where(b["mask"], b[k], np.float32(-999.0))
    if plant is not None:
        was = b["mask"].copy()
        plant(b["mask"])
        assert not (b["mask"] & ~was).any()              # (planting only clears: no pixel without data is switched on)
        for k in ("flux", "error", "delta"):
            b[k] = np.where(b["mask"], b[k], np.float32(-999.0))
    if random_F:
        p = dict(p)
        p["F"] = np.random.default_rng(seed + 2).uniform(-0.5, 0.5, size=(npix, nh)).astype(np.float32)
    if junk:
        rng = np.random.default_rng(bseed + 2)
        hole = ~b["mask"]
        fill = rng.choice(np.array([np.nan, np.inf, -np.inf, -999.0], dtype=np.float32), size=hole.sum())
        b["delta"] = b["delta"].copy(); b["error"] = b["error"].copy()
        b["delta"][hole] = fill
        b["error"][hole] = fill[::-1]
    zfac = ((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), (wav[:nb] / synthetic.LYA).astype(np.float32))
    return p, b, dead, wav, nb, zfac


def zabs_of(zfac, dtype=np.float64):
    """what the factored-z kernels take for zabs: the product of the two float32 factors - 1, in ``dtype``"""
    return np.outer(zfac[0].astype(dtype), zfac[1].astype(dtype)) - dtype(1.0)


def a_blue_of(zabs_f32):
    """the host-supplied A_blue as a caller with the Becker tau would form it: float32 exp(-tau(zabs)) (numpy; the GPU test hands
    the kernels this very array through its tau callable's tensor)"""
    from qfa_amd import synthetic
    return np.exp(-synthetic._tau_becker(zabs_f32.astype(np.float64))).astype(np.float32)


# ---- past the fold of k_em_stats (qfa_em.h: kFlush = 64 MFMA steps = 256 spectra) ----
# em_plan (qfa_em.hip) at B = 4101, N_pix = 4040: nblk = 64, R = min(16, ceil(4101 / 256) = 17, by_mem) = 16, per = ceil(4101 / 16) =
# 257 -> 260, ranges 0..14 of 260 spectra and a last range of 4101 - 15 * 260 = 201, which is no multiple of 4.
FOLD_B, FOLD_NPIX, FOLD_PER, FOLD_R = 4101, 4040, 260, 16
FOLD_CASES = [  # (nh, form): launch_stats<2>; <4>; <10> at t0 = 0 and 10 (2 of 10 tiles); four passes, the last with 5 tiles
    (4, "factored"), (8, "a_blue"), (17, "zabs"), (32, "factored"),
]
# planted pixel columns: seen ONLY by spectra of in-range index >= 256 (its whole value passes through the final tot += acc);
# only by spectra of in-range index < 256 (folded once, zeros after); by one spectrum of the last, short range (its last)
FOLD_COLUMNS = {"late": 777, "early": 2500, "single": FOLD_NPIX - 1}


def fold_plant(mask):
    B, npix = mask.shape
    j = np.arange(B) % FOLD_PER
    mask[j < 256, FOLD_COLUMNS["late"]] = False
    mask[j >= 256, FOLD_COLUMNS["early"]] = False
    mask[np.arange(B) != B - 1, FOLD_COLUMNS["single"]] = False


def plan_from_bytes(em_bytes, step_bytes, B, npix, nh):
    """(R, per, length of the last range) of em_plan, recovered from qfa_em_workspace_bytes and qfa_workspace_bytes alone: the
    workspace is [step ws | REC B ncp | SLAB R N_pix ncp | CNT R N_pix] floats, each part rounded up to 256 bytes."""
    up = lambda x: (x + 255) // 256 * 256
    ncp = 16 * ((nh * (nh + 1) // 2 + 15) // 16 + (nh + 15) // 16)
    rest = em_bytes - up(step_bytes) - up(4 * B * ncp)
    Rs = [R for R in range(1, B + 1) if up(4 * R * npix * ncp) + up(4 * R * npix) == rest]
    assert len(Rs) == 1, (em_bytes, step_bytes, Rs)
    R = Rs[0]
    per = ((B + R - 1) // R + 3) // 4 * 4
    assert (B + per - 1) // per == R, (B, R, per)
    return R, per, B - (R - 1) * per


ACCUM_CASES = [(203, 8, 96, 11), (333, 17, 300, 12)]         # (npix, nh, B, seed): one range; two ranges

# every case the statistics' bars are measured over: (kind, npix, nh, B, form, seed)
ELEMENT_CASES = (
    [("shape", n, k, B, f, n + 5 * k) for n, k, B in SHAPES for f in ("zabs", "factored")] + [("shape", 203, 8, 70, "a_blue", 13)]
    + [("fold", FOLD_NPIX, k, FOLD_B, f, 100 + k) for k, f in FOLD_CASES]
    + [("accum", n, k, B, "zabs", s) for n, k, B, s in ACCUM_CASES]
)


def case_reference_inputs(kind, npix, nh, B, form, seed, batch_seed=None):
    """(p, b, dead, zfac, zabs the float64 reference takes, A_blue it takes or None) of a case of ELEMENT_CASES"""
    p, b, dead, wav, nb, zfac = em_inputs(npix, nh, B, seed, batch_seed=batch_seed, plant=fold_plant if kind == "fold" else None)
    zabs = zabs_of(zfac) if form == "factored" else b["zabs"]
    return p, b, dead, zfac, zabs, a_blue_of(b["zabs"]) if form == "a_blue" else None


def case_terms(case, dtype=np.float64):
    """``em_terms`` of a case (the accumulation cases: the list of both batches' terms)"""
    kind, npix, nh, B, form, seed = case
    out = []
    for bs in ((None, seed + 50) if kind == "accum" else (None,)):
        p, b, dead, zfac, zabs, ab = case_reference_inputs(kind, npix, nh, B, form, seed, batch_seed=bs)
        if dtype == np.float32 and form == "factored":
            zabs = zabs_of(zfac, np.float32)
        out.append(em_terms(p, b["delta"], b["error"], zabs, b["mask"], A_blue=ab, dtype=dtype))
    return out if kind == "accum" else out[0]
