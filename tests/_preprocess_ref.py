"""numpy float64 restatement of the observed-frame preprocessing rule (include/qfa_hip.h, qfa_preprocess_f32).

Plain loops over (spectrum, output pixel, input pixel): for an output pixel the overlap with EVERY input pixel of the spectrum
is formed -- no search, no assumption on where the overlapping pixels sit -- and the sums run over the input pixels in order.
(The overlaps of one output pixel are formed as one numpy expression over j, and the terms that are exactly zero are left out of
the running sums: adding +0.0 changes no float64 sum.)  Everything is float64 until the two outputs are rounded to float32.
"""
import numpy as np

SENTINEL = np.float32(-999.0)


def edges_from_grid(wav_grid):
    """the rest-frame output edges the package derives from a grid: geometric midpoints, half a step of log10 beyond each end"""
    lg = np.log10(np.asarray(wav_grid, dtype=np.float64))
    mid = 0.5 * (lg[:-1] + lg[1:])
    return 10.0 ** np.concatenate([[lg[0] - 0.5 * (lg[1] - lg[0])], mid, [lg[-1] + 0.5 * (lg[-1] - lg[-2])]])


def input_edges(w):
    n = len(w)
    e = np.empty(n + 1, dtype=np.float64)
    e[1:n] = 0.5 * (w[:-1] + w[1:])
    e[0] = w[0] - (e[1] - w[0])
    e[n] = w[n - 1] + (w[n - 1] - e[n - 1])
    return e


def usable_pixels(flux, ivar, bad):
    with np.errstate(invalid="ignore"):
        use = (ivar > 0) & np.isfinite(ivar) & np.isfinite(flux)
    if bad is not None:
        use &= np.asarray(bad) == 0
    return use


def rebin_one(w, f, iv, bad, z, out_edges):
    """flux_k, ivar_k, coverage_k, W_k (float64, Npix each) of one spectrum; NaN where W = 0"""
    npix = len(out_edges) - 1
    fk, ik, cov, Wk = (np.full(npix, np.nan), np.full(npix, np.nan), np.zeros(npix), np.zeros(npix))
    zp1 = 1.0 + float(z)
    if len(w) < 2 or not (zp1 > 0.0 and np.isfinite(zp1)):
        return fk, ik, cov, Wk
    w = np.asarray(w, dtype=np.float64)
    e = input_edges(w)
    use = usable_pixels(f, iv, bad)
    u = np.where(use, iv, 0).astype(np.float64)
    ff = np.where(use, f, 0).astype(np.float64)
    E = np.asarray(out_edges, dtype=np.float64) * zp1
    for k in range(npix):
        ov = np.maximum(0.0, np.minimum(e[1:], E[k + 1]) - np.maximum(e[:-1], E[k]))
        c = ov / (E[k + 1] - E[k])
        W = S1 = S2 = cv = np.float64(0.0)
        for j in np.nonzero(c)[0]:
            cu = c[j] * u[j]
            W = W + cu
            S1 = S1 + cu * ff[j]
            S2 = S2 + c[j] * cu
            if use[j]:
                cv = cv + c[j]
        cov[k], Wk[k] = cv, W
        if W > 0:
            fk[k] = S1 / W
            ik[k] = W * W / S2
    return fk, ik, cov, Wk


def run_counts(valid):
    """n_valid, n_lead, n_trail, num_mask of a bool array"""
    valid = np.asarray(valid, dtype=bool)
    n = len(valid)
    nv = int(valid.sum())
    if nv == 0:
        return 0, n, n, 0
    idx = np.nonzero(valid)[0]
    lead, trail = int(idx[0]), int(n - 1 - idx[-1])
    inner = valid[idx[0]:idx[-1] + 1]
    runs = 0
    for k in range(1, len(inner)):
        if not inner[k] and inner[k - 1]:
            runs += 1
    return nv, lead, trail, runs


def preprocess_ref(wave, flux, ivar, offsets, zqso, wav_grid, out_edges=None, bad=None, min_coverage=0.5,
                   norm_window=(1270., 1290.), norm_min_pixels=5, snr_window=(1270., 1600.)):
    wav_grid = np.asarray(wav_grid, dtype=np.float64)
    out_edges = edges_from_grid(wav_grid) if out_edges is None else np.asarray(out_edges, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    N, npix = len(offsets) - 1, len(wav_grid)
    out = dict(flux=np.full((N, npix), SENTINEL, dtype=np.float32), error=np.full((N, npix), SENTINEL, dtype=np.float32),
               norm=np.full(N, np.nan), snr=np.full(N, np.nan), n_valid=np.zeros(N, np.int32), n_lead=np.zeros(N, np.int32),
               n_trail=np.zeros(N, np.int32), num_mask=np.zeros(N, np.int32), ok=np.zeros(N, np.int32),
               coverage=np.zeros((N, npix)), n_norm=np.zeros(N, np.int32), norm_scale=np.zeros(N))
    in_norm = (wav_grid >= norm_window[0]) & (wav_grid < norm_window[1])
    in_snr = (wav_grid >= snr_window[0]) & (wav_grid < snr_window[1])
    for i in range(N):
        a, b = int(offsets[i]), int(offsets[i + 1])
        fk, ik, cov, Wk = rebin_one(wave[a:b], flux[a:b], ivar[a:b], None if bad is None else bad[a:b], zqso[i], out_edges)
        valid = (cov >= min_coverage) & (Wk > 0)
        num = den = ssn = absn = np.float64(0.0)
        nn = ns = 0
        for k in range(npix):
            if valid[k] and in_norm[k]:
                num = num + ik[k] * fk[k]
                den = den + ik[k]
                absn = absn + ik[k] * abs(fk[k])
                nn += 1
            if valid[k] and in_snr[k]:
                ssn = ssn + fk[k] * np.sqrt(ik[k])
                ns += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            norm = num / den
        ok = bool(nn >= norm_min_pixels and norm > 0 and np.isfinite(norm))
        out["coverage"][i], out["n_norm"][i] = cov, nn
        out["norm"][i] = norm
        out["norm_scale"][i] = absn / den if nn > 0 else 0.0
        out["snr"][i] = ssn / ns if ns > 0 else np.nan
        out["n_valid"][i], out["n_lead"][i], out["n_trail"][i], out["num_mask"][i] = run_counts(valid)
        out["ok"][i] = int(ok)
        if ok:
            with np.errstate(over="ignore"):
                out["flux"][i, valid] = (fk[valid] / norm).astype(np.float32)
                out["error"][i, valid] = (1.0 / (np.sqrt(ik[valid]) * norm)).astype(np.float32)
    return out


def assert_away_from_thresholds(ref, min_coverage=0.5, tol=1e-9):
    """No validity decision and no ok decision of the restatement sits within `tol` of its bound.  coverage is O(1), so the
    distance to min_coverage is absolute; `ok` has one float bound, norm > 0, and |norm| is measured against the mean of
    |flux_k| under the same weights (what a sum in another order can move it by is a rounding of that)."""
    assert not np.any(np.abs(ref["coverage"] - min_coverage) <= tol), "a coverage sits on min_coverage: pick another seed"
    has = ref["n_norm"] > 0
    assert np.all(np.abs(ref["norm"][has]) > tol * ref["norm_scale"][has]), "a norm sits on 0: pick another seed"
