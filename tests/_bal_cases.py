"""The seeded inputs the BAL tests share (tests/test_bal.py on the GPU, tests/test_bal_cpu.py for the condition on them): a coarse
grid whose C IV window has exactly the asked number of pixels, a model whose draws differ by about one per cent, and spectra
whose troughs have r = 0.3 .. 0.6 inside and r >= 0.95 outside, so that threshold decisions are clean.  The reference of a case is
computed once (`reference`, cached) and never modified."""
import functools

import numpy as np

import _bal_ref as R

LINES = (1549.06, 1559.40)                    # C IV and a second "line" 2 000 km/s redward of it: its window sees the same troughs shifted
MARGIN, NB = 3, 2                             # pixels outside the window on both sides; the model's blue pixels (all below the window)
INDICES = (R.BI, R.AI)
CONT_MIN = 0.05
PATTERNS = ("random", "crossing", "ends", "whole", "many", "gaps", "masked", "random")

# (n_win, Nh, S, B, smooth, max_gap, first pattern): window lengths around the 64-pixel chunk, every form of N_h, S, B, smooth and
# max_gap; B = 3 cases start at different patterns so that every pattern is met at several window lengths.  The last case has so many
# draws for its few spectra that a wave walks two draws one after the other (`draws_per_wave`)
CASES = ((1, 1, 1, 1, 1, 0, 3), (63, 8, 3, 3, 3, 1, 0), (64, 17, 1, 3, 1, 0, 3), (65, 32, 1, 70, 1, 3, 0), (128, 8, 5, 3, 5, 3, 3),
         (129, 17, 3, 3, 3, 0, 4), (200, 8, 1, 8, 1, 1, 0), (200, 32, 3, 3, 5, 3, 4), (200, 8, 1, 3, 3, 0, 1),
         (24, 8, 700, 3, 3, 1, 3))


def draws_per_wave(B, n_lines, S, blocks=4096):
    """how many consecutive draws one wave of qfa_bal_scan_f32 walks (qfa_bal.hip: a call aims at `blocks` blocks before it cuts the
    draws of a (spectrum, line) into groups); LDS arrays and counters are reused from one draw to the next when this exceeds 1"""
    pairs = B * n_lines
    nsg = max(1, min(S, -(-blocks // pairs)))
    return -(-S // nsg)


def grid_of(n_win):
    """(wav, p_lo, p_hi): n_win + 2 MARGIN pixels linear in C IV velocity; the window's pixels span [-500, 25 500] km/s, so both ends
    of both indices' ranges fall inside it"""
    dv = 26000.0 / n_win
    npix = n_win + 2 * MARGIN
    i = npix - 1 - np.arange(npix) - MARGIN                           # window pixel number of pixel p (negative / >= n_win: margin)
    v = (i + 0.5) * dv - 500.0
    return LINES[0] * (1.0 - v / R.C_KMS), MARGIN, MARGIN + n_win


def windows_of(wav, p_lo, p_hi, n_lines=2):
    """line 0: the whole window; line 1: the same without its last pixel (the lowest velocity)"""
    w = [(p_lo, p_hi, R.window(wav, LINES[0], p_lo, p_hi))]
    if n_lines > 1:
        hi = max(p_lo, p_hi - 1)
        w.append((p_lo, hi, R.window(wav, LINES[1], p_lo, hi)))
    return w


def profile(kind, n, rng):
    """(below (n,), gaps (n,)) in WINDOW order: where the trough is, and which pixels are masked on purpose"""
    below, gaps = np.zeros(n, bool), np.zeros(n, bool)
    if kind == "random":
        i = 0
        while i < n:
            ln = int(rng.choice([1, 2, 4, 7, 20, 70]))
            if rng.random() < 0.45:
                below[i:i + ln] = True
            i += ln
        gaps = rng.random(n) < 0.08
    elif kind == "crossing":
        below[58:70] = True
        below[max(0, n - 70):max(0, n - 58)] = True
    elif kind == "ends":
        below[:6] = True
        below[max(0, n - 6):] = True
    elif kind == "whole":
        below[:] = True
    elif kind == "many":
        below[np.arange(n) % 6 < 4] = True
    elif kind == "gaps":
        below[50:80] = True
        below[100:140] = True
        for a, b in ((60, 61), (62, 66), (110, 114), (120, 122), (126, 129)):   # 1, 4 (over a chunk boundary), 4, 2, 3 (over one) pixels
            gaps[a:b] = True
        below[3:30] = True
        gaps[10:13] = True                                                       # 3 pixels
    elif kind == "masked":
        below[n // 3:n // 2] = True
        gaps[:] = True
    return below, gaps


@functools.lru_cache(maxsize=None)
def inputs(n_win, nh, S, B, first):
    rng = np.random.default_rng(1000 + 7 * n_win + nh + 31 * S + B)
    wav, p_lo, p_hi = grid_of(n_win)
    npix = len(wav)
    F = (rng.uniform(-1, 1, (npix, nh)) * 0.005 / np.sqrt(nh)).astype(np.float32)
    mu = (1.0 + 0.1 * np.sin(np.arange(npix) / 7.0)).astype(np.float32)
    h = np.clip(rng.normal(0, 1, (B, S, nh)), -3, 3).astype(np.float32)
    c0 = mu.astype(np.float64)[None, :] + np.einsum("pj,bj->bp", F.astype(np.float64), h[:, 0].astype(np.float64))
    prof = rng.uniform(0.98, 1.05, (B, npix))
    mask = np.ones((B, npix), bool)
    for b in range(B):
        below, gaps = profile(PATTERNS[(b + first) % len(PATTERNS)], n_win, rng)
        sel = np.arange(p_hi - 1, p_lo - 1, -1)                                   # pixel of window pixel i
        prof[b, sel[below]] = rng.uniform(0.3, 0.6, int(below.sum()))
        mask[b, sel[gaps]] = False
    error = rng.uniform(0.01, 0.05, (B, npix)).astype(np.float32)
    flux = (c0 * prof).astype(np.float32)
    return {"wav": wav, "p_lo": p_lo, "p_hi": p_hi, "npix": npix, "F": F, "mu": mu, "h": h, "flux": flux, "error": error, "mask": mask}


@functools.lru_cache(maxsize=None)
def reference(case):
    n_win, nh, S, B, smooth, max_gap, first = case
    g = inputs(n_win, nh, S, B, first)
    w = windows_of(g["wav"], g["p_lo"], g["p_hi"])
    r = R.bal_scan(g["F"], g["mu"], g["flux"], g["error"], g["mask"], g["h"], w, INDICES, thr=0.9, smooth=smooth, max_gap=max_gap,
                   cont_min=CONT_MIN, trough_index=1)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
