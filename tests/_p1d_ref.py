"""numpy port of the 1D flux power contract (include/qfa_hip.h, qfa_p1d_f32).

What the contract defines bit for bit is computed in float32 exactly as specified: the bins of the mean transmission and of the
stack (tests/_forest_ref.py, bin_index), `used`, the contrast d = T / tb - 1 and the noise variance v = 1 / (ivar (tb tb)), each
operation rounded once.  The DFT -- twiddles at the exact integer (j m) mod L -- the power, the noise level and the stack are
float64."""
import numpy as np

from _forest_ref import U, U64, bin_index, z_factored   # noqa: F401  (re-exported for the tests)

f32 = np.float32


def dft_matrix(L):
    """(L, M) complex128 exp(-2 pi i ((j m) mod L) / L), m = 1 .. M = L // 2"""
    j = np.arange(L, dtype=np.int64)[:, None]
    m = np.arange(1, L // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((j * m) % L).astype(np.float64) / L
    return np.cos(ang) - 1j * np.sin(ang)


def contrast(trans, ivar, z, tbar, tbar_bins):
    """per pixel: d, v (float32 values as float64) and used, for trans / ivar (B, S, Nb), z (B, Nb), tbar (St, nT)"""
    trans, ivar, tbar = np.asarray(trans, f32), np.asarray(ivar, f32), np.atleast_2d(np.asarray(tbar, f32))
    B, S, Nb = trans.shape
    kT = bin_index(z, tbar_bins[0], tbar_bins[1], tbar_bins[2])                       # (B, Nb)
    rows = np.zeros(S, np.int64) if tbar.shape[0] == 1 else np.arange(S)
    tb = tbar[rows[None, :, None], np.maximum(kT, 0)[:, None, :]]                    # (B, S, Nb)
    with np.errstate(all="ignore"):
        used = (ivar > 0) & (kT >= 0)[:, None, :] & (tb > 0)
        d = ((trans / tb).astype(f32) - f32(1.0)).astype(f32)
        v = (f32(1.0) / (ivar * (tb * tb).astype(f32)).astype(f32)).astype(f32)
    d = np.where(used, d, f32(0.0)).astype(np.float64)
    v = np.where(used, v, f32(0.0)).astype(np.float64)
    return d, v, used


def p1d(trans, ivar, z, tbar, tbar_bins, p_lo, L, nseg, min_used, bins):
    """Returns a dict: d (B, S, nseg, L), n_used, valid, N (B, S, nseg), X (B, S, nseg, M) complex, P, sum_abs_d, kz (B, nseg),
    stack / stack_abs (S, nz, 2 + 2M).  N and P are 0 on an invalid segment, as the outputs are."""
    d, v, used = contrast(trans, ivar, z, tbar, tbar_bins)
    B, S, _ = d.shape
    cut = lambda x: x[:, :, p_lo:p_lo + nseg * L].reshape(B, S, nseg, L)
    d, v, used = cut(d), cut(v), cut(used)
    n_used = used.sum(-1)
    valid = n_used >= min_used
    X = d @ dft_matrix(L)
    P = np.where(valid[..., None], (X.real ** 2 + X.imag ** 2) / L, 0.0)
    N = np.where(valid, v.sum(-1) / L, 0.0)
    zc = np.asarray(z, f32)[:, p_lo + np.arange(nseg) * L + L // 2]                   # (B, nseg)
    kz = bin_index(zc, bins[0], bins[1], bins[2])
    stack, sabs = stack_of(P, N, valid, kz, bins[2])
    return {"d": d, "n_used": n_used, "valid": valid, "N": N, "X": X, "P": P, "sum_abs_d": np.abs(d).sum(-1), "kz": kz,
            "stack": stack, "stack_abs": sabs}


def stack_of(P, N, valid, kz, nz):
    """(S, nz, 2 + 2M) sums [n | N | P_m | P_m^2] of (B, S, nseg, M) P and (B, S, nseg) N over the valid segments with bin kz
    (B, nseg) >= 0: the terms formed as the reducer forms them (float64, P P rounded once), added in extended precision; also the
    sums of |terms|"""
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    B, S, nseg, M = P.shape
    sums = np.zeros((S, nz, 2 + 2 * M), np.longdouble)
    for b in range(B):
        for s in range(S):
            for g in range(nseg):
                if valid[b, s, g] and kz[b, g] >= 0:
                    row = sums[s, kz[b, g]]
                    row[0] += 1
                    row[1] += N[b, s, g]
                    row[2:2 + M] += P[b, s, g]
                    row[2 + M:] += P[b, s, g] * P[b, s, g]
    out = sums.astype(np.float64)
    return out, np.abs(out)                                                           # (every term is >= 0)


def amp_bound(r, L):
    """|dX_m| <= (2L + 8) u sum_j |d_j| per segment: a float32 twiddle (u), and a float32 fma chain of L steps, one rounding each,
    whose partial sums are bounded by sum |d| (L u to first order) give (L + 1) u sum |d| on Re and on Im alike, sqrt(2) of it on
    X; the factor 2 covers that, the second-order terms and the matrix pipe's internal rounding"""
    return (2 * L + 8) * U * r["sum_abs_d"]


def power_bound(r, L):
    """|dP_m| <= (2 |X_m| e + e^2) / L + 4 u P_m with e = amp_bound: the two squares, their sum and the division by L, each
    rounded once in float32"""
    e = amp_bound(r, L)[..., None]
    return (2 * np.abs(r["X"]) * e + e * e) / L + 4 * U * r["P"]


def noise_bound(r, L):
    """(L + 4) u N: any order of adding L non-negative float32 terms, and the division"""
    return (L + 4) * U * r["N"]
