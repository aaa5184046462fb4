"""numpy port of the band-power contract (include/qfa_hip.h, qfa_p1d_band_f32), from the per-segment power P (.., M) and noise N (..)
that qfa_p1d_f32 defines (tests/_p1d_ref.py): the band map, Q_a = sum_{m in a} w_m (P_m - s N), the stack
[n | sum Q_a | sum Q_a Q_b], and the bars the GPU is held to.  The sums are formed in extended precision (np.longdouble), so the
port's own rounding is far inside the bars.

The bars (u = 2^-53, float64 throughout, every operation rounded once, no contraction):

  Q_a.  A term t_m = w_m (P_m - s N): the product s N is exact (s is 0 or 1), the difference and the product with w_m round once
  each: |fl(t_m) - t_m| <= 2 u |w_m| (|P_m| + |N|) to first order.  Adding n_a terms in any order moves the sum by at most
  (n_a - 1) u sum |t_m| <= (n_a - 1) u sum |w_m| (|P_m| + |N|).  Together (n_a + 1) u A_a with A_a = sum_m |w_m| (|P_m| + |N|); the
  bar is (n_a + 2) u A_a, the extra u covering the second-order terms.

  sum Q_a and sum Q_a Q_b over the n segments of a (draw, z-bin).  A term is Q_a (exact) or fl(Q_a Q_b) (one rounding); a term
  added in chunk c at position i takes part in the additions after it in its chunk and in the additions of the later chunks'
  partials; a chunk without a segment of the bin adds an exact zero.  That is at most n - 1 additions that round, so the sum of the
  GPU's own terms is within (n + 1) u sum |terms| of exact; the bar is (n + 3) u sum |terms|.  The GPU's terms are formed from its
  own Q, which is within dQ_a of the port's: the port's sums move by sum_seg dQ_a and by sum_seg (|Q_a| dQ_b + |Q_b| dQ_a + dQ_a dQ_b).
"""
import numpy as np

U64 = 2.0 ** -53
LD = np.longdouble


def mode_k(L, dv):
    """(M,) wavenumbers 2 pi m / (L dv), m = 1 .. M = L // 2"""
    return 2.0 * np.pi * np.arange(1, L // 2 + 1, dtype=np.float64) / (L * dv)


def band_map(L, dv, k_edges):
    """band (M,) int32 of mode m (entry m - 1): a with k_edges[a] <= k_m < k_edges[a + 1], else -1; and the modes per band"""
    k, e = mode_k(L, dv), np.asarray(k_edges, np.float64)
    nband = len(e) - 1
    band = np.full(L // 2, -1, np.int32)
    for a in range(nband):
        band[(k >= e[a]) & (k < e[a + 1])] = a
    return band, np.array([(band == a).sum() for a in range(nband)], np.int64)


def weights(L, dv, k_edges, resolution_kms=None):
    """w_m = dv / (n_a W^2(k_m)) as float32 (what QFA.p1d_bands hands the kernel), 0 for a mode in no band"""
    band, count = band_map(L, dv, k_edges)
    k = mode_k(L, dv)
    w = np.full(L // 2, float(dv)) / np.maximum(count[np.maximum(band, 0)], 1)
    if resolution_kms is not None:
        w = w / (np.sinc(k * dv / (2.0 * np.pi)) * np.exp(-0.5 * (k * resolution_kms) ** 2)) ** 2
    return np.where(band >= 0, w, 0.0).astype(np.float32)


def band_q(P, N, band, weight, sub, nband):
    """Q (.., nband) float64, its bar dQ (.., nband), from P (.., M) and N (..): an invalid segment has P = N = 0, so Q = 0"""
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    M = P.shape[-1]
    w = np.ones(M) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    x = P.astype(LD) - LD(sub) * N.astype(LD)[..., None]
    mag = np.abs(P) + np.abs(N)[..., None]
    Q = np.zeros(P.shape[:-1] + (nband,), np.float64)
    dQ = np.zeros_like(Q)
    for a in range(nband):
        sel = np.asarray(band[:M]) == a
        Q[..., a] = (w[sel].astype(LD) * x[..., sel]).sum(-1).astype(np.float64)
        dQ[..., a] = (sel.sum() + 2) * U64 * (np.abs(w[sel]) * mag[..., sel]).sum(-1)
    return Q, dQ


def stack_of(Q, dQ, ok, kz, nz):
    """(S, nz, 1 + nband + nband^2) [n | sum Q_a | sum Q_a Q_b] of Q (B, S, nseg, nband) over the segments with ok (B, S, nseg) and
    bin kz (B, nseg) >= 0, and the bar of every entry: (n + 3) u sum |terms| plus the propagated bar of Q"""
    B, S, nseg, nband = Q.shape
    W = 1 + nband + nband * nband
    sums, sabs, prop = (np.zeros((S, nz, W), LD) for _ in range(3))
    for b in range(B):
        for s in range(S):
            for g in range(nseg):
                if ok[b, s, g] and kz[b, g] >= 0:
                    q, d = Q[b, s, g].astype(LD), dQ[b, s, g].astype(LD)
                    row = (s, kz[b, g])
                    sums[row][0] += 1
                    sums[row][1:1 + nband] += q
                    sabs[row][1:1 + nband] += np.abs(q)
                    prop[row][1:1 + nband] += d
                    qq = np.outer(q, q)
                    sums[row][1 + nband:] += qq.ravel()
                    sabs[row][1 + nband:] += np.abs(qq).ravel()
                    prop[row][1 + nband:] += (np.outer(np.abs(q), d) + np.outer(d, np.abs(q)) + np.outer(d, d)).ravel()
    n = sums[:, :, :1]
    bar = (n + 3) * U64 * sabs + prop
    return sums.astype(np.float64), bar.astype(np.float64)


def cov_of(stack, nband):
    """mean (S, nz, nband) and the covariance of the mean (S, nz, nband, nband) = (sum Q Q^T / n - mean mean^T) / (n - 1); NaN at
    n < 2"""
    stack = np.asarray(stack, np.float64)
    n = stack[:, :, 0]
    with np.errstate(all="ignore"):
        mean = stack[:, :, 1:1 + nband] / n[:, :, None]
        m2 = stack[:, :, 1 + nband:].reshape(stack.shape[:2] + (nband, nband)) / n[:, :, None, None]
        cov = (m2 - mean[..., :, None] * mean[..., None, :]) / (n[:, :, None, None] - 1.0)
    cov[n < 2] = np.nan
    return mean, cov
