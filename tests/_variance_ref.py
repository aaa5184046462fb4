"""numpy port of the variance-function contract (include/qfa_hip.h, qfa_variance_f32), and the bar its float sums are held to.

`used`, d and v are tests/_p1d_ref.py's (`contrast`); n_used, validity and the z-bin of a segment are formed from them as that port
forms them.  The bin of v is taken from its bits (`v_code`), as the kernel takes it.  The terms are float64: v, d, d d (exact: two
24-bit factors) and (d d)(d d) (rounded once, the same rounding the kernel makes); the port adds them in extended precision.

Bar.  A sum of n terms formed in any order -- a tree with n - 1 inexact additions at most; additions of an exact 0 round nothing --
is off by at most (n - 1) u S(1 + O(n u)), S = sum |term|, u = 2^-53; the port's own sum, rounded once to float64, by u S.  So
|GPU - port| <= n 2^-52 S with a factor 2 to spare for the second-order terms: `bars` returns it per entry of `moments` and `stack`,
0 for the integer entries.  It holds for the segment rows, for the stack (whose terms are the pixels of all its segments: the rows,
chunks and launches are subtrees of one tree) and for stacks added by several calls."""
import numpy as np

import _p1d_ref as R
from _forest_ref import bin_index

f32 = np.float32
U52 = 2.0 ** -52
FLT_MAX = float(np.finfo(np.float32).max)


def v_code(v, e_lo, sub):
    """the bin code of float32 v from its bit pattern: (u >> (23 - sub)) - ((e_lo + 127) << sub), arithmetic shift"""
    u = np.ascontiguousarray(np.asarray(v, f32)).view(np.int32).astype(np.int64)
    return (u >> (23 - sub)) - ((e_lo + 127) << sub)


def v_edges(e_lo, n_oct, sub):
    """(nv + 1,) float64 edges, exact: bin c = [edge c, edge c + 1)"""
    c = np.arange((n_oct << sub) + 1)
    return np.ldexp(1.0 + (c & ((1 << sub) - 1)) / float(1 << sub), e_lo + (c >> sub))


def choose_bins(v_used, n_oct):
    """e_lo that puts the median of the used pixels' v in the middle octave of n_oct"""
    med = float(np.median(v_used)) if v_used.size else 1.0
    return int(np.clip(int(np.floor(np.log2(med))) - (n_oct - 1) // 2, -126, 127 - n_oct))


def variance(trans, ivar, z, tbar, tbar_bins, p_lo, L, nseg, min_used, bins, e_lo, n_oct, sub, d_max=None):
    """Returns a dict: moments / moments_abs (B, S, nseg, 5, nv) float64 = [n_a | sum v | sum d | sum d^2 | sum d^4] and the sums of
    |term|; n_used, valid (B, S, nseg); kz (B, nseg); stack / stack_abs (S, nz, 2 + 5 nv); v_all: the v of the used pixels of the
    segments.  moments are 0 on an invalid segment, as the outputs are."""
    nv = n_oct << sub
    d, v, used = R.contrast(trans, ivar, z, tbar, tbar_bins)
    B, S, _ = d.shape
    cut = lambda x: x[:, :, p_lo:p_lo + nseg * L].reshape(B, S, nseg, L)
    d, v, used = cut(d), cut(v), cut(used)
    n_used = used.sum(-1)
    valid = n_used >= min_used
    c = v_code(v.astype(f32), e_lo, sub)
    with np.errstate(all="ignore"):
        keep = np.abs(d.astype(f32)) <= f32(FLT_MAX if d_max is None else d_max)       # (false for a NaN)
    counted = used & valid[..., None] & (c >= 0) & (c < nv) & keep
    v_all = v[used]
    d, v = np.where(counted, d, 0.0), np.where(counted, v, 0.0)
    d2 = d * d
    terms = [counted.astype(np.float64), v, d, d2, d2 * d2]
    mom = np.zeros((B, S, nseg, 5, nv), np.longdouble)
    mab = np.zeros((B, S, nseg, 5, nv), np.longdouble)
    for a in range(nv):
        sel = counted & (c == a)
        for k, t in enumerate(terms):
            ts = np.where(sel, t, 0.0)
            mom[..., k, a] = ts.sum(-1, dtype=np.longdouble)
            mab[..., k, a] = np.abs(ts).sum(-1, dtype=np.longdouble)
    zc = np.asarray(z, f32)[:, p_lo + np.arange(nseg) * L + L // 2]                   # (B, nseg)
    kz = bin_index(zc, bins[0], bins[1], bins[2])
    nz = bins[2]
    # (S, nz, 2 + 5 nv) sums over the valid segments with bin kz >= 0, every segment added once to the row of its bin
    sel = valid & (kz >= 0)[:, None, :]                                              # (B, S, nseg)
    head = np.stack([np.ones_like(n_used), n_used], -1).astype(np.longdouble)        # (B, S, nseg, 2)
    rows = np.concatenate([head, mom.reshape(B, S, nseg, 5 * nv)], -1) * sel[..., None]
    rab = np.concatenate([head, mab.reshape(B, S, nseg, 5 * nv)], -1) * sel[..., None]
    flat = lambda x: np.moveaxis(x, 1, 2).reshape(B * nseg, S, 2 + 5 * nv)
    kf = np.maximum(kz, 0).reshape(B * nseg)
    st = np.zeros((nz, S, 2 + 5 * nv), np.longdouble)
    sab = np.zeros((nz, S, 2 + 5 * nv), np.longdouble)
    np.add.at(st, kf, flat(rows))
    np.add.at(sab, kf, flat(rab))
    st, sab = np.moveaxis(st, 0, 1), np.moveaxis(sab, 0, 1)
    return {"moments": mom.astype(np.float64), "moments_abs": mab.astype(np.float64), "n_used": n_used, "valid": valid, "kz": kz,
            "stack": st.astype(np.float64), "stack_abs": sab.astype(np.float64), "v_all": v_all, "nv": nv}


def stack_terms(ref):
    """the number of terms of every float entry of `stack` (0 for the counts), shaped like it"""
    nv = ref["nv"]
    n = np.zeros_like(ref["stack"])
    for k in range(1, 5):
        n[:, :, 2 + k * nv:2 + (k + 1) * nv] = ref["stack"][:, :, 2:2 + nv]
    return n


def bars(ref):
    """(bar of moments, bar of stack): (terms) 2^-52 sum |term| per float entry, 0 for the counts"""
    mb = ref["moments"][..., 0:1, :] * U52 * ref["moments_abs"]
    mb[..., 0, :] = 0.0
    return mb, stack_terms(ref) * U52 * ref["stack_abs"]
