"""numpy port of the flux PDF contract (include/qfa_hip.h, qfa_flux_pdf_f32), and the bar PDFStack.cov() is held to.

`used` is tests/_p1d_ref.py's (`contrast`); n_used, validity and the z-bin of a segment are formed from it as that port forms them.
The bin arithmetic is float32, operation by operation: x = T or the one division T / tb, the subtraction x - t0, the product with
inv_dt = 1 / dt (float32), floor, and the range test on the float.  Counts and the stack are int64: the GPU's float64 stack must
equal them entry for entry.

Bar of cov().  With T_ab = M_ab + r_b R_a + r_a R_b + r_a r_b Q (R_a = sum_c M_ac, Q = sum_cd M_cd: the sum of |terms| of the
four-term expansion, and equally sum_seg (h_a + r_a m)(h_b + r_b m)) and u = 2^-53:
  PDFStack.cov()   R and Q are sums of integers, exact.  r carries one rounding; r_b R_a two, r_a r_b Q four (two from r, two
                   products); three additions move the sum by at most u T each: 2 + 2 + 4 + 3 = 11 u T.  The scale n / (n - 1) /
                   (dt^2 N^2) and its product with the sum: six more roundings of the result, whose size is at most the scaled T.
  cov_bruteforce   per segment r_a m has two roundings, the difference one: each factor is off by at most 3 u (h_a + r_a m), the
                   product of the two by 6 u plus its own rounding: 7 u of the segment's part of T; n segments are added in a chain:
                   (n - 1) u T; the same six roundings of the scale.
Together (n + 30) u T, scaled; `cov_bar` rounds that up to n + 32 for the second-order terms (n u < 1e-12)."""
import numpy as np

import _p1d_ref as R
from _forest_ref import U64, bin_index   # noqa: F401  (re-exported for the tests)

f32 = np.float32


def pixel_bins(trans, ivar, z, tbar, tbar_bins, t0, dt, nt, relative=False, clamp=False, ivar_min=0.0):
    """per pixel: the flux bin (-1 = in none), counted and used, for trans / ivar (B, S, Nb), z (B, Nb), tbar (St, nT)"""
    trans, ivar, tbar = np.asarray(trans, f32), np.asarray(ivar, f32), np.atleast_2d(np.asarray(tbar, f32))
    _, _, used = R.contrast(trans, ivar, z, tbar, tbar_bins)
    S = trans.shape[1]
    kT = bin_index(z, tbar_bins[0], tbar_bins[1], tbar_bins[2])
    rows = np.zeros(S, np.int64) if tbar.shape[0] == 1 else np.arange(S)
    tb = tbar[rows[None, :, None], np.maximum(kT, 0)[:, None, :]]                    # (B, S, Nb)
    inv = f32(1.0) / f32(dt)
    with np.errstate(all="ignore"):
        x = (trans / tb).astype(f32) if relative else trans
        counted = used & (ivar >= f32(ivar_min))
        fa = np.floor(((x - f32(t0)).astype(f32) * inv).astype(f32)).astype(f32)
        inside = (fa >= f32(0.0)) & (fa < f32(nt))
        low, high = fa < f32(0.0), fa >= f32(nt)                                      # (a NaN is in neither)
    k = np.where(inside, np.where(inside, fa, 0).astype(np.int64), -1)
    if clamp:
        k = np.where(low, 0, np.where(high, nt - 1, k))
    return np.where(counted, k, -1), counted, used


def flux_pdf(trans, ivar, z, tbar, tbar_bins, p_lo, L, nseg, min_used, bins, t0, dt, nt, relative=False, clamp=False, ivar_min=0.0):
    """Returns a dict: hist (B, S, nseg, nt), n_used, n_cnt, valid (B, S, nseg), kz (B, nseg), stack (S, nz, 2 + nt + nt^2), all
    int64 (valid bool).  hist and n_cnt are 0 on an invalid segment, as the outputs are."""
    k, counted, used = pixel_bins(trans, ivar, z, tbar, tbar_bins, t0, dt, nt, relative, clamp, ivar_min)
    B, S, _ = k.shape
    cut = lambda a: a[:, :, p_lo:p_lo + nseg * L].reshape(B, S, nseg, L)
    k, counted, used = cut(k), cut(counted), cut(used)
    n_used = used.sum(-1)
    valid = n_used >= min_used
    hist = np.stack([(k == a).sum(-1) for a in range(nt)], axis=-1).astype(np.int64)
    hist = np.where(valid[..., None], hist, 0)
    n_cnt = np.where(valid, counted.sum(-1), 0).astype(np.int64)
    zc = np.asarray(z, f32)[:, p_lo + np.arange(nseg) * L + L // 2]                   # (B, nseg)
    kz = bin_index(zc, bins[0], bins[1], bins[2])
    return {"hist": hist, "n_used": n_used, "n_cnt": n_cnt, "valid": valid, "kz": kz, "stack": stack_of(hist, n_cnt, valid, kz, bins[2])}


def stack_of(hist, n_cnt, valid, kz, nz):
    """(S, nz, 2 + nt + nt^2) int64 sums [n_seg | n_cnt | h_a | h_a h_b] over the valid segments with bin kz (B, nseg) >= 0"""
    hist = np.asarray(hist, np.int64)
    B, S, nseg, nt = hist.shape
    out = np.zeros((S, nz, 2 + nt + nt * nt), np.int64)
    for k in range(nz):
        sel = valid & (kz == k)[:, None, :]                                          # (B, S, nseg)
        h = hist * sel[..., None]
        out[:, k, 0] = sel.sum((0, 2))
        out[:, k, 1] = (np.asarray(n_cnt, np.int64) * sel).sum((0, 2))
        out[:, k, 2:2 + nt] = h.sum((0, 2))
        out[:, k, 2 + nt:] = np.einsum("bsga,bsgc->sac", h, h).reshape(S, nt * nt)
    return out


def cov_bruteforce(hist, valid, kz, nz, dt):
    """(S, nz, nt, nt) the delta-method covariance of the PDF segment by segment in float64: n / (n - 1) sum_seg (h_a - r_a m)
    (h_b - r_b m) / (dt^2 N^2), r_a = H_a / N, m = sum_a h_a of the segment; NaN where n < 2 or N = 0"""
    hist = np.asarray(hist, np.int64)
    B, S, nseg, nt = hist.shape
    dt = float(f32(dt))
    out = np.full((S, nz, nt, nt), np.nan)
    for s in range(S):
        for k in range(nz):
            hs = [hist[b, s, g].astype(np.float64) for b in range(B) for g in range(nseg) if valid[b, s, g] and kz[b, g] == k]
            n = len(hs)
            N = float(sum(h.sum() for h in hs))
            if n < 2 or N == 0.0:
                continue
            r = sum(hs) / N
            acc = np.zeros((nt, nt))
            for h in hs:
                e = h - r * h.sum()
                acc = acc + e[:, None] * e[None, :]
            out[s, k] = n / (n - 1.0) * acc / (dt * dt * (N * N))
    return out


def cov_bar(stack, nt, dt):
    """(S, nz, nt, nt) (n + 32) 2^-53 T_ab n / (n - 1) / (dt^2 N^2) from an integer stack (the module docstring); also the scaled
    T_ab.  NaN where n < 2 or N = 0"""
    st = np.asarray(stack, np.float64)
    dt = float(f32(dt))
    n = st[:, :, 0][:, :, None, None]
    H = st[:, :, 2:2 + nt]
    M = st[:, :, 2 + nt:].reshape(st.shape[0], st.shape[1], nt, nt)
    N = H.sum(-1)[:, :, None, None]
    with np.errstate(all="ignore"):
        r = H[:, :, :, None] / N
        Ra = M.sum(-1)
        T = M + np.swapaxes(r, 2, 3) * Ra[:, :, :, None] + r * Ra[:, :, None, :] + r * np.swapaxes(r, 2, 3) * Ra.sum(-1)[:, :, None, None]
        scaled = T * n / (n - 1.0) / (dt * dt * N * N)
    scaled = np.where((n > 1) & (N > 0), scaled, np.nan)
    return (n + 32.0) * U64 * scaled, scaled
