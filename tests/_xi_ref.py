"""numpy port of the line-of-sight correlation contract (include/qfa_hip.h, qfa_xi_f32), and the bars the GPU is held to.

What the contract defines bit for bit is computed in float32 with its operation sequence: `used`, d and v are tests/_p1d_ref.py's
(`contrast`); wv = 1 / (v + sigma2_lss) is one float32 addition and one float32 division (numpy's float32 division is IEEE: these are
the GPU's bits), w and x = w d follow by selects and one product.  The pair sums W_l, A_l and N0 are float64 sums of the exact
float64 products of those float32 values.

Bars.
  pair    |dA_l| <= (L - l + 2) u sum_j |x_j x_{j+l}|, u = 2^-24; W_l the same with w; N0 the same form with L + 3.  Model: n = L - l
          float32 terms added in any order (a chain, a tree, several chains joined at the end, with or without zero terms between
          them), at most one rounding per product and one per addition (an fma has one for both).  Every term passes through at most
          n - 1 additions and one product rounding, each of which moves the running sum by at most u times the sum of |terms| so
          far: (1 + u)^n - 1 <= n u + (n u)^2, and the +2 covers that second order for every n <= 4096 (n u <= 2.5e-4).  N0's terms
          (w w) v hold a second product: one more u.
  stack   n 2^-53 sum |terms| against float64 sums of the GPU's own float32 rows (n = the segments of the entry: n - 1 additions
          of float64, each product rounded once before it is added -- the reference forms the same rounded products).  Counts are
          exact."""
import numpy as np

import _p1d_ref as R
from _forest_ref import U, U64, bin_index   # noqa: F401  (re-exported for the tests)

f32 = np.float32


def weights(trans, ivar, z, tbar, tbar_bins, sigma2_lss=0.0, unit_w=False):
    """per pixel: w, x, v (float32 values as float64) and used, for trans / ivar (B, S, Nb), z (B, Nb), tbar (St, nT)"""
    d, v, used = R.contrast(trans, ivar, z, tbar, tbar_bins)
    d32, v32 = d.astype(f32), v.astype(f32)                                           # (exact: they hold float32 values)
    with np.errstate(all="ignore"):
        wv = (f32(1.0) / (v32 + f32(sigma2_lss)).astype(f32)).astype(f32)
    if unit_w:
        w = np.where(used, f32(1.0), f32(0.0)).astype(f32)
    else:
        w = np.where(used & np.isfinite(wv), wv, f32(0.0)).astype(f32)
    x = (w * d32).astype(f32)
    return w.astype(np.float64), x.astype(np.float64), v, used


def lag_sums(a, nlag):
    """(..., nlag) sums over j of a_j a_{j+l} and of |a_j a_{j+l}| for a (..., L), l < nlag, in float64"""
    L = a.shape[-1]
    out = np.zeros(a.shape[:-1] + (nlag,))
    oabs = np.zeros_like(out)
    for l in range(nlag):
        p = a[..., :L - l] * a[..., l:]
        out[..., l] = p.sum(-1)
        oabs[..., l] = np.abs(p).sum(-1)
    return out, oabs


def xi(trans, ivar, z, tbar, tbar_bins, p_lo, L, nseg, min_used, bins, nlag, sigma2_lss=0.0, unit_w=False):
    """Returns a dict: w, x, v (B, S, nseg, L), n_used, valid (B, S, nseg), W, A, absW, absA (B, S, nseg, nlag), N0, absN0
    (B, S, nseg), kz (B, nseg), stack / stack_abs (S, nz, 2 + 5 nlag).  W, A and N0 are 0 on an invalid segment, as the outputs are."""
    w, x, v, used = weights(trans, ivar, z, tbar, tbar_bins, sigma2_lss, unit_w)
    B, S, _ = w.shape
    cut = lambda a: a[:, :, p_lo:p_lo + nseg * L].reshape(B, S, nseg, L)
    w, x, v, used = cut(w), cut(x), cut(v), cut(used)
    n_used = used.sum(-1)
    valid = n_used >= min_used
    W, absW = lag_sums(w, nlag)
    A, absA = lag_sums(x, nlag)
    with np.errstate(all="ignore"):
        t0 = (w * w) * v
    N0, absN0 = t0.sum(-1), np.abs(t0).sum(-1)
    zero = lambda a: np.where(valid[..., None] if a.ndim == 4 else valid, a, 0.0)
    W, absW, A, absA, N0, absN0 = (zero(a) for a in (W, absW, A, absA, N0, absN0))
    zc = np.asarray(z, f32)[:, p_lo + np.arange(nseg) * L + L // 2]                   # (B, nseg)
    kz = bin_index(zc, bins[0], bins[1], bins[2])
    stack, sabs = stack_of(np.stack([W, A], axis=3), N0, valid, kz, bins[2])
    return {"w": w, "x": x, "v": v, "n_used": n_used, "valid": valid, "W": W, "A": A, "absW": absW, "absA": absA, "N0": N0,
            "absN0": absN0, "kz": kz, "stack": stack, "stack_abs": sabs}


def stack_of(pairs, noise0, valid, kz, nz):
    """(S, nz, 2 + 5 nlag) sums [n | N0 | W_l | A_l | W_l^2 | A_l W_l | A_l^2] of pairs (B, S, nseg, 2, nlag) and noise0 (B, S, nseg)
    over the valid segments with bin kz (B, nseg) >= 0: the terms formed as the reducer forms them (float64, each product rounded
    once), added in extended precision; also the sums of |terms|"""
    pairs, noise0 = np.asarray(pairs, np.float64), np.asarray(noise0, np.float64)
    B, S, nseg, _, nlag = pairs.shape
    sums = np.zeros((S, nz, 2 + 5 * nlag), np.longdouble)
    sabs = np.zeros_like(sums)
    for b in range(B):
        for s in range(S):
            for g in range(nseg):
                if valid[b, s, g] and kz[b, g] >= 0:
                    W, A = pairs[b, s, g, 0], pairs[b, s, g, 1]
                    row = np.concatenate([[1.0, noise0[b, s, g]], W, A, W * W, A * W, A * A])
                    sums[s, kz[b, g]] += row
                    sabs[s, kz[b, g]] += np.abs(row)
    return sums.astype(np.float64), sabs.astype(np.float64)


def pair_bound(sum_abs, L):
    """(L - l + 2) u sum |terms| for (..., nlag) sums of |terms|"""
    nlag = sum_abs.shape[-1]
    return (L - np.arange(nlag) + 2) * U * sum_abs


def noise0_bound(abs_n0, L):
    """(L + 3) u sum |(w w) v|"""
    return (L + 3) * U * abs_n0


def brute_force(w, x, v, nlag):
    """W_l, A_l, N0 of ONE segment by the double loop of the definition (float64)"""
    L = len(w)
    W, A = np.zeros(nlag), np.zeros(nlag)
    for l in range(nlag):
        for j in range(L - l):
            W[l] += w[j] * w[j + l]
            A[l] += x[j] * x[j + l]
    return W, A, float(sum(w[j] * w[j] * v[j] for j in range(L)))
