"""Vectorised numpy port of the posterior-draw contract of include/qfa_hip.h (qfa_sample_latent_f32 / qfa_continua_f32).
Test infrastructure only: the library never calls it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32, key: (..., 2) uint32 (broadcastable) -> (..., 4) uint32 (Random123 philox4x32_10)."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint32).copy()
    k1 = np.asarray(key[..., 1], dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = M0 * c[0], M1 * c[2]
            hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
            hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
            c = [hi1 ^ c[1] ^ k0.astype(np.uint64), lo1, hi0 ^ c[3] ^ k1.astype(np.uint64), lo0]
            k0 = k0 + W0
            k1 = k1 + W1
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def normals(seed, rows, n_samples, nh):
    """z (len(rows), S, nh) float32 of the contract for global rows `rows` (int64 array)."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    nq = (nh + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, None, :]
    s = np.arange(n_samples, dtype=np.uint64)[None, :, None]
    r = rows[:, None, None]
    shape = (len(rows), n_samples, nq)
    ctr = np.stack([np.broadcast_to(q, shape), np.broadcast_to(s, shape), np.broadcast_to(r & MASK32, shape),
                    np.broadcast_to(r >> np.uint64(32), shape)], axis=-1).astype(np.uint32)
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    x = philox4x32_10(ctr, key).astype(np.float64)
    u = (x + 0.5) * 2.0 ** -32
    rad0, t0 = np.sqrt(-2.0 * np.log(u[..., 0])), 2 * np.pi * u[..., 1]
    rad1, t1 = np.sqrt(-2.0 * np.log(u[..., 2])), 2 * np.pi * u[..., 3]
    z = np.stack([rad0 * np.cos(t0), rad0 * np.sin(t0), rad1 * np.cos(t1), rad1 * np.sin(t1)], axis=-1)
    return z.reshape(len(rows), n_samples, 4 * nq)[..., :nh].astype(np.float32)


def chol64(a):
    """Lower Cholesky factor of the lower triangle of a (n, n) in float64; a pivot <= 0 zeroes its column."""
    L = np.tril(np.asarray(a, dtype=np.float64)).copy()
    n = L.shape[0]
    for k in range(n):
        piv = L[k, k]
        d = np.sqrt(piv) if piv > 0 else 0.0
        L[k, k] = d
        L[k + 1:, k] = L[k + 1:, k] / d if piv > 0 else 0.0
        L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    return L


def latent(hmean, hcov, seed, row0, n_samples):
    """h (B, S, Nh) float64 before the final rounding, the contract's hmean + C z (NaN for a non-finite spectrum)."""
    hmean = np.asarray(hmean, dtype=np.float64)
    B, nh = hmean.shape
    z = normals(seed, row0 + np.arange(B), n_samples, nh).astype(np.float64)
    out = np.empty((B, n_samples, nh))
    for b in range(B):
        if not (np.isfinite(hcov[b]).all() and np.isfinite(hmean[b]).all()):
            out[b] = np.nan
            continue
        out[b] = hmean[b] + z[b] @ chol64(hcov[b]).T
    return out
