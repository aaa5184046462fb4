"""numpy float64 restatement of the redshift finder's rule (include/qfa_hip.h, qfa_redshift_scan_f32), built from the oracle's pixel
terms and Woodbury core on index-shifted parameter rows; plus the data the two test files share: a model whose mean has emission
lines, so that a shift is identifiable, and spectra drawn from it at a known integer shift."""
import numpy as np

from oracle import qfa_oracle as O

LYA = 1215.67
C_KMS = 299792.458
NLL_BAR = 5e-6                  # the project's per-spectrum NLL bar (relative)
BAR = 1e-5                      # |llr - llr_f64| <= BAR max(|NLL_0|, |NLL_s|): its double on a difference of two (tests/_dla_ref.BAR)
LINES = ((1034.0, 8.0, 0.4), (1215.67, 12.0, 1.5), (1400.0, 12.0, 0.3), (1549.0, 14.0, 0.8))     # centre, sigma (Angstrom), height


def grid(npix, lam_lo=1030.0, lam_hi=1600.0):
    """(wav (npix,), dloglam): exactly log-uniform, as the reference's 10**arange(log10 LAMMIN, log10 LAMMAX, LOGLAM_DELTA)"""
    d = np.log10(lam_hi / lam_lo) / npix
    return 10.0 ** (np.log10(lam_lo) + d * np.arange(npix)), d


def model(npix, nb, nh, seed=0):
    """(params, mu, wav, dloglam).  mu: a power-law continuum with four emission lines; F: smooth random loadings whose summed
    standard deviation is 0.08 whatever nh; Psi about 0.04^2, omega about 0.05.  nb is free (the tests put the blue/red boundary
    at 0, at the scan's edge and at the last pixel): z comes from wav / 1215.67 whatever it is."""
    rng = np.random.default_rng(seed)
    wav, d = grid(npix)
    mu = (wav / 1280.0) ** -1.5
    for c, s, a in LINES:
        mu = mu + a * np.exp(-0.5 * ((wav - c) / s) ** 2)
    kw = max(3, (npix // 8) | 1)
    ker = np.hanning(kw + 2)[1:-1]
    ker /= np.sqrt(np.sum(ker ** 2))
    F = np.stack([np.convolve(rng.standard_normal(npix + kw - 1), ker, mode="valid") for _ in range(nh)], axis=1) * (0.08 / np.sqrt(nh))
    params = {"F": F.astype(np.float32), "Psi": (0.04 ** 2 * (0.5 + rng.random(npix))).astype(np.float32),
              "omega": (0.05 * (0.5 + rng.random(nb))).astype(np.float32), "tau0": np.float32(0.146), "beta": np.float32(1.333),
              "c0": np.float32(0.239)}
    return params, mu.astype(np.float32), wav, d


def z_pixels(zqso, wav):
    """(B, Npix) float32: z_p = fma(zq1, pix_ratio_full[p], -1) of float32 factors, as the prep kernel forms it"""
    zq1 = (1.0 + np.asarray(zqso, dtype=np.float64)).astype(np.float32).astype(np.float64)
    ratio = (np.asarray(wav, dtype=np.float64) / LYA).astype(np.float32).astype(np.float64)
    return (zq1[:, None] * ratio[None, :] - 1.0).astype(np.float32)


def nll_one(params, mu, x, sg, w, z, m, s, tau_which="becker", tau_series=1):
    """NLL of one spectrum under candidate s (data pixel p is model pixel p + s) over the window [m, N - m), float64: the oracle's
    pixel terms and Woodbury core on the parameter rows p + s"""
    n = len(x)
    nb = np.asarray(params["omega"]).shape[0]
    lo, hi = m, n - m
    nbs = int(np.clip(nb - s - lo, 0, hi - lo))                    # window pixels with p + s < nb
    ps = {"F": np.asarray(params["F"], dtype=np.float64)[lo + s:hi + s], "Psi": np.asarray(params["Psi"], dtype=np.float64)[lo + s:hi + s],
          "omega": np.asarray(params["omega"], dtype=np.float64)[lo + s:lo + s + nbs], "tau0": params["tau0"], "c0": params["c0"],
          "beta": params["beta"]}
    ww = np.asarray(w, dtype=bool)[lo:hi]
    xx = np.where(ww, np.asarray(x, dtype=np.float64)[lo:hi], 0.0)
    ss = np.where(ww, np.asarray(sg, dtype=np.float64)[lo:hi], 1.0)
    A, _, D = O.pixel_terms(ps, ss, np.asarray(z)[lo:lo + nbs], tau_which, tau_series)
    return O._lowrank_core(ps["F"], A, D, ww, xx - A * np.asarray(mu, dtype=np.float64)[lo + s:hi + s])[-1]


def scan(params, mu, flux, error, mask, zqso, wav, m, tau_which="becker", tau_series=1):
    """(llr (B, 2 m + 1), nll0 (B,), nll (B, 2 m + 1)) in float64"""
    z = z_pixels(zqso, wav)
    nll = np.array([[nll_one(params, mu, flux[b], error[b], mask[b], z[b], m, s, tau_which, tau_series) for s in range(-m, m + 1)]
                    for b in range(len(flux))])
    return nll[:, m:m + 1] - nll, nll[:, m].copy(), nll


def argbest(llr):
    """the rule's arg-max: the largest value, among equals the lowest |s|, then the lowest s; as s"""
    llr = np.asarray(llr)
    m = (llr.shape[1] - 1) // 2
    s = np.arange(-m, m + 1)
    order = np.lexsort((s, np.abs(s)))                            # candidates by (|s|, s)
    return np.array([s[order[int(np.argmax(row[order]))]] for row in llr])


def parabola(llr, best_s):
    """(off, sig) float64 of the parabola through the three values around best_s; NaN at the edges and for a curvature >= 0"""
    llr = np.asarray(llr, dtype=np.float64)
    m = (llr.shape[1] - 1) // 2
    off, sig = np.full(len(llr), np.nan), np.full(len(llr), np.nan)
    for b, s in enumerate(best_s):
        c = int(s) + m
        if 0 < c < llr.shape[1] - 1:
            cv = (llr[b, c - 1] - llr[b, c]) + (llr[b, c + 1] - llr[b, c])
            if cv < 0.0:
                off[b], sig[b] = 0.5 * (llr[b, c - 1] - llr[b, c + 1]) / cv, 1.0 / np.sqrt(-cv)
    return off, sig


def draw(params, mu, wav, B, seed, shifts, snr=(20.0, 100.0), zq=(2.2, 3.4), masks=True, tau_which="becker", tau_series=1):
    """B spectra drawn from the model at the integer shifts `shifts` (B,): data pixel p is drawn from model pixel p + t, with the
    absorption of its own observed-frame redshift z_p.  Pixels whose p + t falls off the grid hold the mean of the nearest model
    pixel (they lie outside every window with m >= |t|).  2 % random masks and one masked run; masked pixels hold -999.
    Returns dict(flux, error float32; mask bool; zqso float64; shift int)."""
    rng = np.random.default_rng(seed)
    n = len(wav)
    F, Psi, om = (np.asarray(params[k], dtype=np.float64) for k in ("F", "Psi", "omega"))
    nb = len(om)
    mu = np.asarray(mu, dtype=np.float64)
    zqso = rng.uniform(zq[0], zq[1], size=B)
    z = z_pixels(zqso, wav).astype(np.float64)
    shifts = np.broadcast_to(np.asarray(shifts, dtype=np.int64), (B,))
    s2n = np.exp(rng.uniform(np.log(snr[0]), np.log(snr[1]), size=B))
    flux, sigma = np.empty((B, n)), np.empty((B, n))
    for b in range(B):
        q = np.clip(np.arange(n) + shifts[b], 0, n - 1)
        blue = q < nb
        A = np.where(blue, np.exp(-O.tau_eff(z[b], tau_which, tau_series)), 1.0)
        zd = np.where(blue, O.omega_zdep(z[b], float(params["tau0"]), float(params["beta"]), float(params["c0"])), 0.0)
        omq = np.where(blue, om[np.minimum(q, max(nb - 1, 0))] if nb > 0 else 0.0, 0.0)
        sigma[b] = np.abs(mu[q]) / s2n[b] * (0.8 + 0.4 * rng.random(n))
        flux[b] = A * (mu[q] + F[q] @ rng.standard_normal(F.shape[1]) + np.sqrt(Psi[q]) * rng.standard_normal(n)) \
            + np.sqrt(omq * zd) * rng.standard_normal(n) + sigma[b] * rng.standard_normal(n)
    mask = np.ones((B, n), dtype=bool)
    if masks:
        for b in range(B):
            st = int(rng.integers(0, n))
            mask[b, st:st + max(2, n // 40)] = False
        mask &= rng.random((B, n)) >= 0.02
    return dict(flux=np.where(mask, flux, -999.0).astype(np.float32), error=np.where(mask, sigma, -999.0).astype(np.float32),
                mask=mask, zqso=zqso, shift=shifts.copy())


def chunk_size(ws_bytes, npix, nh, m, limit=64):
    """the number of spectra that one chunk of the scan's batch walk holds, read off the library's own size function
    (`ws_bytes(B, Npix, Nh, max_shift)`: qfa_zscan_workspace_bytes), as tests/_dla_ref.chunk_size reads the DLA scan's"""
    ws = [int(ws_bytes(b, npix, nh, m)) for b in range(1, limit + 2)]
    assert all(v > 0 for v in ws)
    flat = [i for i in range(limit) if ws[i + 1] == ws[i]]
    assert flat, "the workspace still grows at B = %d" % limit
    bc = flat[0] + 1
    assert all(ws[i + 1] > ws[i] for i in range(bc - 1)) and all(v == ws[bc - 1] for v in ws[bc - 1:])
    return bc


# the three recovery data sets: (N_pix, N_b, N_h, m, B, S/N range, seed)
RECOVERY = ((160, 64, 4, 6, 48, (20.0, 100.0), 101), (96, 38, 9, 17, 32, (20.0, 100.0), 102), (200, 80, 16, 8, 32, (5.0, 20.0), 103))
# the chunked case: the records and moments of a spectrum at N_h = 32 and 501 candidates pass 1 MiB, so a chunk holds fewer than 64
CHUNK_SHAPE = (512, 200, 32, 250)

_recovery = {}


def recovery_case(i):
    """the i-th recovery data set, its model and the restatement's scan (made once): shifts drawn uniformly from -m .. m"""
    if i not in _recovery:
        npix, nb, nh, m, B, snr, seed = RECOVERY[i]
        params, mu, wav, d = model(npix, nb, nh, seed)
        t = np.random.default_rng(seed + 1).integers(-m, m + 1, size=B)
        data = draw(params, mu, wav, B, seed + 2, t, snr=snr)
        llr, nll0, nll = scan(params, mu, data["flux"], data["error"], data["mask"], data["zqso"], wav, m)
        _recovery[i] = dict(params=params, mu=mu, wav=wav, dloglam=d, nb=nb, nh=nh, m=m, llr=llr, nll0=nll0, nll=nll, **data)
    return _recovery[i]
