"""Numpy restatement of the sightline bootstrap of include/qfa_hip.h (qfa_bootstrap_f64), without a matrix product: the weights from
`_philox_ref` and the contract's threshold table, the sums a plain float64 loop per (draw, replicate, z-bin).  Test infrastructure
only: the library never calls it."""
import numpy as np

import _philox_ref

# T_k = floor(2^32 sum_{i <= k} e^-1 / i!), k = 0 .. 12, as the header lists them
THRESHOLDS = np.array([0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f,
                       0xfffffe21, 0xffffffd4, 0xfffffffc, 0xffffffff], dtype=np.uint64)


def words(seed, rows, n_boot):
    """u (len(rows), n_boot) uint32: word r & 3 of the Philox call of counter (0x40000000 | (r >> 2), 0, g lo, g hi)"""
    g = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    nq = (int(n_boot) + 3) // 4
    shape = (len(g), nq)
    q = np.broadcast_to(np.uint64(0x40000000) | np.arange(nq, dtype=np.uint64)[None, :], shape)
    ctr = np.stack([q, np.zeros(shape, np.uint64), np.broadcast_to((g & _philox_ref.MASK32)[:, None], shape),
                    np.broadcast_to((g >> np.uint64(32))[:, None], shape)], axis=-1).astype(np.uint32)
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return _philox_ref.philox4x32_10(ctr, key).reshape(len(g), 4 * nq)[:, :int(n_boot)]


def weights(seed, rows, n_boot):
    """w (len(rows), n_boot) int64: the number of thresholds T_k <= u"""
    u = words(seed, rows, n_boot).astype(np.uint64)
    return (u[..., None] >= THRESHOLDS).sum(-1).astype(np.int64)


def bootstrap(rows, codes, nz, n_boot, seed, row_offset, boot=None):
    """boot (S, R, nz, 1 + W) float64 of rows (B, S, nseg, W) and codes (B, S, nseg): [sum w | sum w x] over the segments with code kz,
    added in order of (b, g) onto ``boot`` (None: zeros).  Also the bound's ingredients: (boot, n_terms (S, nz), absum (S, R, nz, 1 + W)
    = sum w |x|)"""
    rows, codes = np.asarray(rows), np.asarray(codes)
    B, S, nseg, W = rows.shape
    w = weights(seed, int(row_offset) + np.arange(B), n_boot)
    out = np.zeros((S, n_boot, nz, 1 + W)) if boot is None else np.array(boot, dtype=np.float64)
    absum = np.zeros((S, n_boot, nz, 1 + W))
    terms = np.zeros((S, nz), np.int64)
    for s in range(S):
        for kz in range(nz):
            hits = [(b, g) for b in range(B) for g in range(nseg) if codes[b, s, g] == kz]
            terms[s, kz] = len(hits)
            for r in range(n_boot):
                acc, ab = out[s, r, kz].copy(), np.zeros(1 + W)
                for b, g in hits:
                    x = np.concatenate([[1.0], rows[b, s, g].astype(np.float64)])
                    acc = acc + float(w[b, r]) * x
                    ab = ab + float(w[b, r]) * np.abs(x)
                out[s, r, kz], absum[s, r, kz] = acc, ab
    return out, terms, absum
