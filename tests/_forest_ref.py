"""numpy port of the forest-transmission contract (include/qfa_hip.h, qfa_forest_f32).

What the contract defines bit for bit is computed in float32 exactly as specified: the redshift z (as given, or the factored
form's single-rounding fma), the bin index floorf((z - z0) inv_dz), sigma^2, u^2 and with them every bin / range / mask decision.
The continuum c, cabs = |mu| + sum |F h| (the scale of the fma chain's rounding error), T, iv and the stack are float64."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24              # unit roundoff of float32
U64 = 2.0 ** -53


def z_factored(zq1, ratio):
    """z = fma(zq1[r], pix_ratio[p], -1) rounded once: the float64 product of two float32 is exact, and so is the subtraction of
    1 from it (at most 48 significant bits), so that one rounding to float32 remains"""
    p = np.asarray(zq1, f32).astype(np.float64)[:, None] * np.asarray(ratio, f32).astype(np.float64)[None, :]
    return (p - 1.0).astype(f32)


def bin_index(z, z0, dz, nbin):
    """k of every z (float32 array), -1 where the pixel is not stacked; every step in float32, each rounded once"""
    z = np.asarray(z, f32)
    inv = f32(1.0) / f32(dz)
    with np.errstate(invalid="ignore", over="ignore"):
        kf = np.floor((z - f32(z0)).astype(f32) * inv).astype(f32)
        ok = (kf >= f32(0.0)) & (kf < f32(nbin))
    return np.where(ok, np.where(ok, kf, 0).astype(np.int64), -1)


def stack_of(T, iv, use, k, nbin, unit_w=False):
    """(S, 4, nbin) sums [w | w T | w T^2 | n] of (B, S, Nb) T, iv over the used pixels with bin k (B, Nb) >= 0, their terms formed
    as the kernel forms them (w T exact in float64, w (T T) rounded once) and added in extended precision; also the sums of
    |terms| and the number of terms, for summation bounds"""
    T = np.asarray(T, np.float64)
    B, S, Nb = T.shape
    w = np.ones_like(T) if unit_w else np.asarray(iv, np.float64)
    terms = np.stack([w, w * T, w * (T * T), np.ones_like(T)], axis=2)                # (B, S, 4, Nb)
    sums = np.zeros((S, 4, nbin), np.longdouble)
    asum = np.zeros((S, 4, nbin), np.longdouble)
    for b in range(B):
        for s in range(S):
            sel = use[b, s] & (k[b] >= 0)
            for q in range(4):
                np.add.at(sums[s, q], k[b][sel], terms[b, s, q][sel].astype(np.longdouble))
                np.add.at(asum[s, q], k[b][sel], np.abs(terms[b, s, q][sel]).astype(np.longdouble))
    return sums.astype(np.float64), asum.astype(np.float64)


def forest(F, mu, flux, error, z, mask, h, unc, bins, cont_min, unit_w=False, pixel_range=None):
    """F (Npix, Nh), mu (Npix,), flux / error (B, Npix), z (B, Nb) float32 as the kernel reads or forms it, mask (B, Npix) bool or
    None, h (B, S, Nh), unc (B, Npix) or None, bins = (z0, dz, nbin).  Returns a dict: c, cabs, T, iv (B, S, Nb) float64, use
    (B, S, Nb) bool, k (B, Nb), stack / stack_abs (S, 4, nbin), n_terms = stack[:, 3]."""
    F, mu, h = np.asarray(F, f32), np.asarray(mu, f32), np.asarray(h, f32)
    flux, error = np.asarray(flux, f32), np.asarray(error, f32)
    B, S, Nh = h.shape
    Nb = z.shape[1]
    z0, dz, nbin = bins
    Fb, hb = F[:Nb].astype(np.float64), h.astype(np.float64)
    c = mu[:Nb].astype(np.float64)[None, None, :] + np.einsum("pj,bsj->bsp", Fb, hb)
    cabs = np.abs(mu[:Nb].astype(np.float64))[None, None, :] + np.einsum("pj,bsj->bsp", np.abs(Fb), np.abs(hb))
    with np.errstate(all="ignore"):
        s2 = (error[:, :Nb] * error[:, :Nb]).astype(f32).astype(np.float64)[:, None, :]
        u2 = np.zeros_like(s2) if unc is None else \
            (np.asarray(unc, f32)[:, :Nb] * np.asarray(unc, f32)[:, :Nb]).astype(f32).astype(np.float64)[:, None, :]
        T = flux[:, :Nb].astype(np.float64)[:, None, :] / c
        iv = c * c / (T * T * u2 + s2)
        m = np.ones((B, Nb), bool) if mask is None else np.asarray(mask, bool)[:, :Nb]
        use = m[:, None, :] & (c > float(f32(cont_min))) & np.isfinite(T) & np.isfinite(iv)
    T, iv = np.where(use, T, 0.0), np.where(use, iv, 0.0)
    k = bin_index(z, z0, dz, nbin)
    p_lo, p_hi = (0, Nb) if pixel_range is None else pixel_range
    p = np.arange(Nb)
    k = np.where(((p >= p_lo) & (p < p_hi))[None, :], k, -1)
    stack, sabs = stack_of(T, iv, use, k, nbin, unit_w)
    return {"c": c, "cabs": cabs, "T": T, "iv": iv, "use": use, "k": k, "stack": stack, "stack_abs": sabs}


def trans_bound(r, Nh):
    """|dT| <= |T| ((Nh + 2) u cabs / |c| + 2 u): the fma chain (Nh roundings of partial sums bounded by cabs) plus one division"""
    return np.abs(r["T"]) * ((Nh + 2) * U * r["cabs"] / np.abs(r["c"]) + 2 * U)


def ivar_bound(r, Nh):
    """iv = fl(fl(c c) / fl(fl(fl(T T) u2) + s2)).  With dc = (Nh + 2) u cabs / |c| the relative error of c and dT = dc + 2 u that of
    T: c c carries 2 dc + u; T T carries 2 dT + u and its product with u2 one more u; s2 is the same float32 on both sides and the
    sum of the two non-negative terms adds one u, so den carries at most 2 dT + 3 u; the quotient adds u:
    2 dc + u + 2 dT + 3 u + u = 4 dc + 9 u, and one more u covers the second-order terms (dc < 1e-5)."""
    return np.abs(r["iv"]) * (4 * (Nh + 2) * U * r["cabs"] / np.abs(r["c"]) + 10 * U)
