"""numpy float64 restatement of the BAL finder's contracts (include/qfa_hip.h, qfa_bal_scan_f32 and qfa_bal_mask_f32), written pixel
by pixel in the obvious serial way: a walk along the window that opens a run on a below pixel, looks ahead over a gap, and closes it.

The continuum c is float64; `_forest_ref`'s cabs and `trans_bound` give the error of the kernel's float32 r.  The smoothed r~ of the
kernel is a float32 sum of n_i terms and one division: |dr~_i| <= (sum_j |dr_j| + (n_i + 1) u sum_j |r_j|) / n_i.  A threshold decision
is CONTESTED when |r~_i - thr| is within that bound; a (b, s, line) row with a contested pixel is not compared.  Bars of a row:
value: sum |dr~_i| width_i / thr + n 2^-53 sum |term|;  var: sum_q term_q 2 ((Nh + 2) u cabs / |c| + 2 u) -- the relative error of the
float32 sigma / c, squared -- + (n + 2 smooth + 8) 2^-53 sum term (a_q is smooth divisions and additions of exact widths)."""
import math

import numpy as np

from _forest_ref import U, U64, trans_bound

f32 = np.float32
C_KMS = 299792.458
WHOLE, AFTER = 0, 1
MAX_TROUGHS = 8
BI = (3000.0, 25000.0, 2000.0, AFTER)
AI = (0.0, 25000.0, 450.0, WHOLE)


def pixel_edges(grid, line):
    """(lower, upper) float64 velocity edges of every pixel of the grid for one line: v = C (1 - wav / line) at the centres, an edge
    halfway between neighbouring centres, extrapolated by half a step at the grid's ends"""
    g = [float(x) for x in grid]
    v = [C_KMS * (1.0 - x / float(line)) for x in g]
    n = len(v)
    upper = [v[0] + (v[0] - v[1]) / 2.0] + [(v[p] + v[p - 1]) / 2.0 for p in range(1, n)]
    lower = [(v[p + 1] + v[p]) / 2.0 for p in range(n - 1)] + [v[n - 1] - (v[n - 2] - v[n - 1]) / 2.0]
    return np.array(lower), np.array(upper)


def window(grid, line, p_lo, p_hi):
    """vedge (p_hi - p_lo + 1) of the pixels [p_lo, p_hi): window pixel i is pixel p_hi - 1 - i"""
    lower, upper = pixel_edges(grid, line)
    if p_hi == p_lo:
        return np.zeros(1)
    return np.array([lower[p_hi - 1 - i] for i in range(p_hi - p_lo)] + [upper[p_lo]])


def pixels(F, mu, flux, error, mask, h, cont_min):
    """c, cabs, T = r, sc = sigma / c, use (B, S, Npix) in float64 over all pixels; decisions on sigma^2 in float32 as the kernel's"""
    F, mu, h = np.asarray(F, f32).astype(np.float64), np.asarray(mu, f32).astype(np.float64), np.asarray(h, f32).astype(np.float64)
    flux, error = np.asarray(flux, f32), np.asarray(error, f32)
    B, npix = flux.shape
    c = mu[None, None, :] + np.einsum("pj,bsj->bsp", F, h)
    cabs = np.abs(mu)[None, None, :] + np.einsum("pj,bsj->bsp", np.abs(F), np.abs(h))
    with np.errstate(all="ignore"):
        s2 = (error * error).astype(f32).astype(np.float64)[:, None, :]
        T = flux.astype(np.float64)[:, None, :] / c
        iv = c * c / s2
        m = np.ones((B, npix), bool) if mask is None else np.asarray(mask, bool)
        use = m[:, None, :] & (c > float(f32(cont_min))) & np.isfinite(T) & np.isfinite(iv)
        sc = error.astype(np.float64)[:, None, :] / c
    return {"c": c, "cabs": cabs, "T": np.where(use, T, 0.0), "sc": np.where(use, sc, 0.0), "use": use}


def find_runs(dom, below, used, max_gap):
    """the runs of one index as (first, last, bridged pixels): the serial walk"""
    n = len(dom)
    runs = []
    i = 0
    while i < n:
        if not (dom[i] and below[i]):
            i += 1
            continue
        first = last = i
        bridged = []
        j = i + 1
        while j < n:
            if dom[j] and below[j]:
                last = j
                j += 1
                continue
            if max_gap > 0 and dom[j] and not used[j]:
                k = j
                while k < n and dom[k] and not used[k]:
                    k += 1
                if k - j <= max_gap and k < n and dom[k] and below[k]:
                    bridged += list(range(j, k))
                    j = k
                    continue
            break
        runs.append((first, last, bridged))
        i = last + 1
    return runs


def scan_row(r, dr, sc, relc, used, vedge, indices, thr, smooth, max_gap, trough_index):
    """one (spectrum, draw, line): r, dr, sc, relc, used over the WINDOW pixels i (velocity order).  Returns the row's outputs and bars"""
    n = len(r)
    hw = smooth // 2
    rt, drt, ni = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    for i in range(n):
        if not used[i]:
            continue
        box = [j for j in range(max(0, i - hw), min(n - 1, i + hw) + 1) if used[j]]
        ni[i] = len(box)
        rt[i] = math.fsum(r[j] for j in box) / len(box)
        drt[i] = (math.fsum(dr[j] for j in box) + (len(box) + 1) * U * math.fsum(abs(r[j]) for j in box)) / len(box)
    below = used & (rt < thr)
    contested = bool(np.any(used & (np.abs(rt - thr) <= drt)))
    out = {"contested": contested, "n_used": int(used.sum()), "value": [], "var": [], "value_bar": [], "var_bar": [], "counts": [],
           "n_troughs": 0, "troughs": np.full((MAX_TROUGHS, 2), np.nan)}
    for x, (v_lo, v_hi, w_min, mode) in enumerate(indices):
        dom = np.array([min(vedge[i + 1], v_hi) - max(vedge[i], v_lo) > 0.0 for i in range(n)], bool)
        w = np.zeros(n)
        n_runs = n_bridged = 0
        edges = []
        for first, last, bridged in find_runs(dom, below, used, max_gap):
            e0, e1 = max(vedge[first], v_lo), min(vedge[last + 1], v_hi)
            mine = [i for i in range(first, last + 1) if below[i]]
            if mode == WHOLE:
                ok = e1 - e0 >= w_min
                wr = {i: (min(vedge[i + 1], v_hi) - max(vedge[i], v_lo)) if ok else 0.0 for i in mine}
            else:
                wr = {i: max(0.0, min(vedge[i + 1], v_hi) - max(vedge[i], e0 + w_min)) for i in mine}
                ok = any(v > 0.0 for v in wr.values())
            if ok:
                n_runs += 1
                n_bridged += len(bridged)
                edges.append((e0, e1))
                for i, v in wr.items():
                    w[i] = v
        on = np.nonzero(w > 0.0)[0]
        terms = [(1.0 - rt[i] / thr) * w[i] for i in on]
        value = math.fsum(terms)
        vbar = math.fsum(drt[i] * w[i] / thr for i in on) + len(on) * U64 * math.fsum(abs(t) for t in terms)
        vt, vb = [], []
        for q in range(n):
            if not used[q]:
                continue
            aq = math.fsum(w[i] / ni[i] for i in range(max(0, q - hw), min(n - 1, q + hw) + 1) if used[i] and w[i] > 0.0)
            if aq > 0.0:
                t = sc[q] * sc[q] * aq * aq
                vt.append(t)
                vb.append(t * 2.0 * (relc[q] + 2 * U))
        var = math.fsum(vt) / (thr * thr)
        varbar = (math.fsum(vb) + (len(vt) + 2 * smooth + 8) * U64 * math.fsum(vt)) / (thr * thr)
        out["value"].append(value); out["var"].append(var); out["value_bar"].append(vbar); out["var_bar"].append(varbar)
        out["counts"].append((len(on), n_runs, n_bridged))
        if x == trough_index:
            out["n_troughs"] = len(edges)
            for t, e in enumerate(edges[:MAX_TROUGHS]):
                out["troughs"][t] = e
    return out


def bal_scan(F, mu, flux, error, mask, h, windows, indices, *, thr=0.9, smooth=1, max_gap=0, cont_min=0.0, trough_index=None):
    """windows: [(p_lo, p_hi, vedge)] per line; indices: [(v_lo, v_hi, w_min, mode)].  Returns value, var, value_bar, var_bar (B, S, L, I),
    counts (B, S, L, I, 3), line_counts (B, S, L, 2), troughs (B, S, L, 8, 2), contested (B, S, L) and the pixel dict"""
    px = pixels(F, mu, flux, error, mask, h, cont_min)
    B, S, _ = px["c"].shape
    Nh = np.asarray(h).shape[2]
    L, I = len(windows), len(indices)
    ti = I - 1 if trough_index is None else trough_index
    with np.errstate(all="ignore"):
        dr = np.where(px["use"], trans_bound(px, Nh), 0.0)
        relc = np.where(px["use"], (Nh + 2) * U * px["cabs"] / np.abs(px["c"]), 0.0)
    res = {"value": np.zeros((B, S, L, I)), "var": np.zeros((B, S, L, I)), "value_bar": np.zeros((B, S, L, I)),
           "var_bar": np.zeros((B, S, L, I)), "counts": np.zeros((B, S, L, I, 3), np.int32), "line_counts": np.zeros((B, S, L, 2), np.int32),
           "troughs": np.full((B, S, L, MAX_TROUGHS, 2), np.nan), "contested": np.zeros((B, S, L), bool), "px": px}
    for l, (p_lo, p_hi, vedge) in enumerate(windows):
        sel = np.arange(p_hi - 1, p_lo - 1, -1) if p_hi > p_lo else np.zeros(0, np.int64)
        for b in range(B):
            for s in range(S):
                o = scan_row(px["T"][b, s, sel], dr[b, s, sel], px["sc"][b, s, sel], relc[b, s, sel], px["use"][b, s, sel],
                             np.asarray(vedge, np.float64), indices, float(thr), smooth, max_gap, ti)
                res["value"][b, s, l], res["var"][b, s, l] = o["value"], o["var"]
                res["value_bar"][b, s, l], res["var_bar"][b, s, l] = o["value_bar"], o["var_bar"]
                res["counts"][b, s, l] = o["counts"]
                res["line_counts"][b, s, l] = (o["n_used"], o["n_troughs"])
                res["troughs"][b, s, l] = o["troughs"]
                res["contested"][b, s, l] = o["contested"]
    return res


def bal_mask(mask, wav, troughs, s_ref, lines, pad):
    """mask_out, n_masked: pixel by pixel, the operations of bal_intervals on (v_min - pad, v_max + pad)"""
    B, S, L = troughs.shape[:3]
    wav = np.asarray(wav, np.float64)
    out = np.ones((B, len(wav)), bool) if mask is None else np.array(mask, bool)
    before = out.copy()
    for b in range(B):
        for l in range(L):
            for v0, v1 in troughs[b, s_ref, l]:
                if not np.isfinite(v0):
                    continue
                for lam in lines:
                    lo = float(lam) * (1.0 - (float(v1) + float(pad)) / C_KMS)
                    hi = float(lam) * (1.0 - (float(v0) - float(pad)) / C_KMS)
                    out[b] &= ~((wav >= lo) & (wav < hi))
    return out, (before & ~out).sum(axis=1).astype(np.int32)
