"""numpy port of the observed-frame contracts (include/qfa_hip.h, qfa_obs_stack_f32 and qfa_calibrate_f32).

What the contracts define bit for bit is computed exactly as specified: the coordinate u, x = (u - u0) inv_du and every bin / range
decision in float64, each operation rounded once (numpy never fuses).  The values c, r, iv and `use` are `_forest_ref.forest`'s, on
every pixel of the spectrum; the stack is `_forest_ref.stack_of`'s extended-precision sums with the sums of |terms| for the bounds."""
import numpy as np

import _forest_ref
from _forest_ref import U64, ivar_bound, trans_bound   # noqa: F401  (the tests' bars)

LOG, LINEAR = 0, 1


def coordinate(pix_u, spec_u, u0, du, mode):
    """x (B, Npix) float64 = (u - u0) inv_du with u = pix_u + spec_u (LOG) or pix_u spec_u (LINEAR), inv_du = 1.0 / du"""
    pu, su = np.asarray(pix_u, np.float64)[None, :], np.asarray(spec_u, np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        u = pu * su if mode == LINEAR else pu + su
        return (u - np.float64(u0)) * (np.float64(1.0) / np.float64(du))


def bin_index(x, nbin, spec_u=None):
    """k = floor(x) where 0 <= x < nbin (tested on the double), else -1; a spectrum whose spec_u is not finite is not stacked"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x < float(nbin))
    if spec_u is not None:
        ok &= np.isfinite(np.asarray(spec_u, np.float64))[:, None]
    return np.where(ok, np.floor(np.where(ok, x, 0.0)).astype(np.int64), -1)


def bin_index_brute(pix_u, spec_u, u0, du, nbin, mode):
    """the same by a loop over Python floats, one pixel at a time"""
    import math
    inv = 1.0 / float(du)
    k = np.full((len(spec_u), len(pix_u)), -1, np.int64)
    for b, su in enumerate(map(float, spec_u)):
        if not math.isfinite(su):
            continue
        for p, pu in enumerate(map(float, pix_u)):
            u = pu * su if mode == LINEAR else pu + su
            x = (u - float(u0)) * inv
            if 0.0 <= x < float(nbin):
                k[b, p] = math.floor(x)
    return k


def obs_stack(F, mu, flux, error, mask, h, unc, pix_u, spec_u, bins, cont_min, unit_w=False):
    """bins = (u0, du, nbin, p_lo, p_hi, mode).  Returns `_forest_ref.forest`'s dict over ALL pixels (c, cabs, T = r, iv, use (B, S,
    Npix)) with k (B, Npix), stack / stack_abs (S, 4, nbin)"""
    u0, du, nbin, p_lo, p_hi, mode = bins
    B, npix = np.asarray(flux).shape
    r = _forest_ref.forest(F, mu, flux, error, np.zeros((B, npix), np.float32), mask, h, unc, (0.0, 1.0, 1), cont_min)
    k = bin_index(coordinate(pix_u, spec_u, u0, du, mode), nbin, spec_u)
    p = np.arange(npix)
    k = np.where(((p >= p_lo) & (p < p_hi))[None, :], k, -1)
    r["k"] = k
    r["stack"], r["stack_abs"] = _forest_ref.stack_of(r["T"], r["iv"], r["use"], k, nbin, unit_w)
    return r


def stack_bars(r, Nh, unit_w=False):
    """(S, 4, nbin) bars of the stack: sum |term| (rel + n 2^-53), rel = the largest relative pixel bound of the row over the stacked
    pixels -- ivar's for sum w (0 under unit weights), plus one trans bound for sum w r, plus two for sum w r^2; the counts are exact"""
    sel = r["use"] & (r["k"] >= 0)[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        rt = np.where(sel, trans_bound(r, Nh) / np.abs(r["T"]), 0.0)
        ri = np.where(sel, ivar_bound(r, Nh) / np.abs(r["iv"]), 0.0)
    rt = np.nan_to_num(rt).max(axis=(0, 2)) if sel.any() else np.zeros(sel.shape[1])       # (S,)  (T == 0: no error at all)
    ri = np.zeros_like(rt) if unit_w else (np.nan_to_num(ri).max(axis=(0, 2)) if sel.any() else np.zeros(sel.shape[1]))
    rel = np.stack([ri, ri + rt, ri + 2 * rt, np.zeros_like(rt)], axis=1)[:, :, None]      # (S, 4, 1)
    n = r["stack"][:, 3][:, None, :]
    return r["stack_abs"] * (rel + n * U64)


def calibrate(flux, error, pix_u, spec_u, cal, u0, du, mode, c_min):
    """Returns flux_out, error_out (float32), n_uncal (int32), and j (N, Npix; -1 where x is outside the table), done (N, Npix) bool,
    the float64 quotients qf, qe"""
    flux, error, cal = np.asarray(flux, np.float32), np.asarray(error, np.float32), np.asarray(cal, np.float64)
    ncal = len(cal)
    with np.errstate(all="ignore"):
        x = coordinate(pix_u, spec_u, u0, du, mode) - np.float64(0.5)
        inside = (x >= 0.0) & (x <= float(ncal - 1))
        j = np.minimum(np.floor(np.where(inside, x, 0.0)).astype(np.int64), ncal - 2)
        f = x - j.astype(np.float64)
        d = cal[j + 1] - cal[j]
        # fma(f, d, cal[j]) rounded once: the product in extended precision, one rounding to float64
        c = (f.astype(np.longdouble) * d.astype(np.longdouble) + cal[j].astype(np.longdouble)).astype(np.float64)
        valid = (flux != np.float32(-999.0)) & (error != np.float32(-999.0))
        done = valid & inside & np.isfinite(c) & (c >= float(c_min))
        qf, qe = flux.astype(np.float64) / c, error.astype(np.float64) / c
        fo = np.where(done, qf.astype(np.float32), flux)
        eo = np.where(done, qe.astype(np.float32), error)
    return fo, eo, (valid & ~done).sum(axis=1).astype(np.int32), np.where(inside, j, -1), done, qf, qe
