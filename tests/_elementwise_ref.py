"""Row-by-row and element-by-element judges of the float32 HIP path against the float64 oracle -- plain numpy.

Two measures sit side by side in the suite.  The whole-tensor rel-L2 (``conftest.rel_l2`` at ``TOL_G``)
says how good the float32 arithmetic is overall; it scales with the tensor, so one wrong element of 10 000 moves it by less
than its bar.  The judges here say WHICH element or row is wrong:

* a per-pixel gradient is a sum over spectra of terms that cancel (|sum| / sum|terms| down to 6e-5 per element), so the
  error of an element is read in units of its own sum of |terms|, exactly as ``return_abs`` of
  ``oracle.qfa_oracle.nll_and_grads_single`` does for the three scalar gradients: ``grad_error_units``;
* the posterior is judged per row, every output with a scale of that row: ``predict_row_errors``.

The case tables and the inputs of tests/test_predict_rows.py and tests/test_gradient_elements.py live here as well, so that
tests/test_elementwise_ref_cpu.py and tools/elementwise_bars.py (which measures the bars, profiles/elementwise_accuracy.txt)
see exactly the inputs that the GPU tests see.
"""
import numpy as np

from oracle import qfa_oracle as O
from qfa_amd import synthetic

GKEYS = ("F", "Psi", "omega")
PKEYS = ("ll", "hmean", "hcov", "cont", "unc")

# The bars (profiles/elementwise_accuracy.txt).  The measures the suite already had keep their bars -- ll 5e-6, cont 1e-4 of the
# row's maximum --, which are ceilings for the others as well.  The new measures: 8 x the worst value of the numpy float32
# oracle against the float64 one over exactly PREDICT_CASES / GRADIENT_CASES below (tools/elementwise_bars.py prints them): the
# kernels sum in another order, use the hardware's exp / log / rcp and split-16-bit products.
PREDICT_BARS = {"ll": 5e-6, "hmean": 8 * 6.41e-6, "hcov": 8 * 7.24e-6, "cont": 1e-4, "unc": 8 * 2.56e-6}
# (elements of two and more terms, elements of ONE term).  A single term is itself a difference of pieces that cancel
# (w/D A^2 f - w/D M Z - u p for F, the two halves of diag(Sigma^-1) - u^2 for Psi and omega); in a sum of many the few
# cancelled terms weigh little next to sum|terms|, in a sum of one nothing does: the float32 oracle reads 2.7e-3 there
# against 3.3e-5, so the pixels that one spectrum sees are judged by a bar of their own.
GRADIENT_BARS = {"F": (8 * 3.34e-5, 8 * 2.68e-3), "Psi": (8 * 2.62e-6, 8 * 3.84e-5), "omega": (8 * 2.68e-6, 8 * 1.07e-6)}


# ----------------------------------------------------------------------------------------------------------------------
# the gradient judge
# ----------------------------------------------------------------------------------------------------------------------
def gradient_units(p, batch, rows=None, dtype=np.float64, keys=GKEYS, tau_which="becker", tau_series=1):
    """One pass of ``O.nll_and_grads_single`` over the spectra ``rows`` of ``batch`` (all of them by default).
    {key: {"sum": elementwise sum of the terms, "count": number of non-zero terms (as O.forward counts them),
           "abssum": elementwise sum of |terms|, "grad": sum / count (0/0 = NaN)}} plus "nll": the per-spectrum NLL."""
    rows = np.arange(len(batch["delta"])) if rows is None else np.asarray(rows)
    out = None
    nll = np.empty(len(rows))
    for j, r in enumerate(rows):
        nll[j], g = O.nll_and_grads_single(p, batch["delta"][r], batch["error"][r], batch["zabs"][r], batch["mask"][r],
                                           tau_which, tau_series, dtype=dtype)
        if out is None:
            out = {k: {"sum": np.zeros_like(g[k]), "count": np.zeros(g[k].shape), "abssum": np.zeros_like(g[k])} for k in keys}
        for k in keys:
            out[k]["sum"] = out[k]["sum"] + g[k]
            out[k]["count"] = out[k]["count"] + (g[k] != 0.0)
            out[k]["abssum"] = out[k]["abssum"] + np.abs(g[k])
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in keys:
            out[k]["grad"] = out[k]["sum"] / out[k]["count"]
    out["nll"] = nll
    return out


def grad_error_units(ours, ref, abssum, count):
    """|ours - ref| * count / sum|terms| per element of a NORMALISED gradient (sum / count).  An element without a term
    (count 0) is NaN on both sides and reads NaN here; NaN or inf on one side only reads inf."""
    ours, ref = np.asarray(ours, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    abssum, count = np.asarray(abssum, dtype=np.float64), np.asarray(count, dtype=np.float64)
    assert ours.shape == ref.shape == abssum.shape == count.shape, (ours.shape, ref.shape, abssum.shape, count.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.abs(ours - ref) * count / abssum
    empty = count == 0
    u[empty & np.isnan(ours) & np.isnan(ref)] = np.nan
    u[empty & ~(np.isnan(ours) & np.isnan(ref))] = np.inf
    u[~empty & ~(np.isfinite(ours) & np.isfinite(ref))] = np.inf
    return u


def worst_element(units):
    """(index tuple, value) of the largest entry, NaN entries aside; ((), 0.0) when there is none"""
    u = np.where(np.isnan(units), -1.0, units)
    if u.size == 0 or u.max() < 0:
        return (), 0.0
    idx = np.unravel_index(int(np.argmax(u)), u.shape)
    return tuple(int(i) for i in idx), float(u[idx])


def _first(cond):
    """index tuple of the first True element, or None"""
    bad = np.argwhere(cond)
    return tuple(int(i) for i in bad[0]) if bad.size else None


def check_gradient(key, ours, ref, bar, counts=None, what=""):
    """Every element of the normalised gradient ``ours`` against ``ref[key]`` of ``gradient_units``: the NaN pattern, the
    counts (``counts``: the implementation's own, per pixel or per element; None = not known) and the units against
    ``bar`` = (elements of two and more terms, elements of one term).  Returns the worst units of the two classes; raises
    AssertionError naming the worst (pixel, column), its count and its units."""
    r = ref[key]
    ours = np.asarray(ours, dtype=np.float64)
    assert ours.shape == r["grad"].shape, (key, what, ours.shape, r["grad"].shape)
    bad = _first(np.isnan(ours) != np.isnan(r["grad"]))
    assert bad is None, f"{key} {what}: NaN pattern differs from the oracle's first at element {bad} (count {r['count'][bad]:.0f})"
    if counts is not None:
        counts = np.asarray(counts, dtype=np.float64)
        counts = np.broadcast_to(counts.reshape(counts.shape + (1,) * (ours.ndim - counts.ndim)), ours.shape)     # (per pixel)
        bad = _first(counts != r["count"])
        assert bad is None, f"{key} {what}: count of element {bad} is {counts[bad]:.0f}, the oracle counts {r['count'][bad]:.0f}"
    u = grad_error_units(ours, r["grad"], r["abssum"], r["count"])
    single = r["count"] == 1
    worst = []
    for cls, b in ((~single, bar[0]), (single, bar[1])):
        idx, w = worst_element(np.where(cls, u, np.nan))
        assert w <= b, f"{key} {what}: element {idx} is {w:.3e} of its sum of |terms| from the oracle (bar {b:.1e}); " \
                       f"count {r['count'][idx]:.0f}, ours {ours[idx]!r}, oracle {r['grad'][idx]!r}"
        worst.append(w)
    return tuple(worst)


# ----------------------------------------------------------------------------------------------------------------------
# the posterior judge
# ----------------------------------------------------------------------------------------------------------------------
def predict_rows(p, mu, batch, rows=None, dtype=np.float64, tau_which="becker", tau_series=1):
    """``O.predict_single`` of every row, stacked: {"ll": (B,), "hmean": (B, k), "hcov": (B, k, k), "cont": (B, Npix),
    "unc": (B, Npix), "nvalid": (B,) unmasked pixels}."""
    rows = np.arange(len(batch["flux"])) if rows is None else np.asarray(rows)
    res = [O.predict_single(p, mu, batch["flux"][r], batch["error"][r], batch["zabs"][r], batch["mask"][r], tau_which,
                            tau_series, dtype=dtype) for r in rows]
    out = {k: np.stack([np.asarray(x[i]) for x in res]) for i, k in enumerate(PKEYS)}
    out["nvalid"] = np.array([int(batch["mask"][r].sum()) for r in rows])
    return out


def _row_max_rel(a, b):
    """max|a - b| / max|b| per row; a row whose reference is all zero must be met exactly (0, else inf)"""
    B = b.shape[0]
    a, b = a.reshape(B, -1), b.reshape(B, -1)
    with np.errstate(invalid="ignore"):
        err = np.max(np.where(np.isfinite(a) & np.isfinite(b), np.abs(a - b), np.inf), axis=1)
    top = np.max(np.abs(b), axis=1)
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), np.where(err == 0, 0.0, np.inf))


def predict_row_errors(ours, ref):
    """Per-row measures {name: (B,) vector} of the five outputs (``ours``: dict or the 5-tuple of ``QFA.predict`` as numpy):
    ll     |err| / max(|ll|, valid pixels, 1)           (as tests/test_fuzz_shapes.py scales it)
    hmean  max|err| / max|hmean| of the row             hcov   max|err| / max|hcov| of the row
    cont   max|err| / max|cont| of the row              (the project's north-star measure)
    unc    max_i |unc_i - o_i| / o_i over the pixels with o_i > 0 -- per PIXEL; a pixel with o_i = 0 is left out.
    A value that is NaN / inf where the oracle's is finite reads inf."""
    if not isinstance(ours, dict):
        ours = dict(zip(PKEYS, ours))
    o = {k: np.asarray(ours[k], dtype=np.float64) for k in PKEYS}
    r = {k: np.asarray(ref[k], dtype=np.float64) for k in PKEYS}
    for k in PKEYS:
        assert o[k].shape == r[k].shape, (k, o[k].shape, r[k].shape)
    out = {}
    scale = np.maximum(np.maximum(np.abs(r["ll"]), np.asarray(ref["nvalid"], dtype=np.float64)), 1.0)
    with np.errstate(invalid="ignore"):
        out["ll"] = np.where(np.isfinite(o["ll"]), np.abs(o["ll"] - r["ll"]) / scale, np.inf)
    for k in ("hmean", "hcov", "cont"):
        out[k] = _row_max_rel(o[k], r[k])
    pos = r["unc"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(np.isfinite(o["unc"]), np.abs(o["unc"] - r["unc"]) / np.where(pos, r["unc"], 1.0), np.inf)
    out["unc"] = np.max(np.where(pos, rel, 0.0), axis=1)
    return out


def check_predict(ours, ref, bars, what=""):
    """All rows, all five outputs; the non-finite pattern equal to the oracle's.  Returns {name: worst over the rows};
    raises AssertionError naming the row."""
    if not isinstance(ours, dict):
        ours = dict(zip(PKEYS, ours))
    for k in PKEYS:
        bad = _first(np.isfinite(np.asarray(ours[k])) != np.isfinite(ref[k]))
        assert bad is None, f"{k} {what}: NaN / inf pattern differs from the oracle's first at {bad}"
    errs = predict_row_errors(ours, ref)
    for k in PKEYS:
        row = int(np.argmax(errs[k]))
        assert errs[k][row] <= bars[k], f"{k} {what}: row {row} of {len(errs[k])} ({ref['nvalid'][row]} valid pixels) is " \
                                        f"{errs[k][row]:.3e} from the oracle (bar {bars[k]:.1e})"
    return {k: float(np.max(errs[k])) for k in PKEYS}


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the two GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def _remask(full, mask, mu_a):
    """the batch ``full`` (drawn without masks: data on every pixel) under ``mask``, sentinels as the loader sets them"""
    b = dict(full)
    b["mask"] = mask
    b["flux"] = np.where(mask, full["flux"], np.float32(-999.0)).astype(np.float32)
    b["error"] = np.where(mask, full["error"], np.float32(-999.0)).astype(np.float32)
    b["delta"] = np.where(mask, full["delta"], np.float32(-999.0) - mu_a).astype(np.float32)
    return b


def _draw(npix, nb, nh, N, seed, wav):
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    full = synthetic.make_batch_numpy(p, mu, wav, nb, N, seed=1000 + seed, masks=False)
    # (the same seed with masks: the data draws come first, so only the mask differs)
    mask = synthetic.make_batch_numpy(p, mu, wav, nb, N, seed=1000 + seed, masks=True)["mask"].copy()
    mu_a = (full["flux"].astype(np.float64) - full["delta"].astype(np.float64)).astype(np.float32)      # mu A as drawn
    return p, mu, full, mask, mu_a


def _rows_of(N, B, seed):
    """B of the N resident rows, a slice of a permutation (tests/test_fuzz_shapes.py)"""
    return np.random.default_rng(4242 + seed).permutation(N)[:B]


# The group sizes of the predict path, as the kernels have them (qfa_host.h, qfa_common.h, qfa_predict_x.h):
#   pass 1 (k_moments_x)                 blocks of 64 spectra (Layout::spb1), waves of 16
#   k_solve                              4 * (64 / KP) spectra per block: 32 / 16 / 8 at KP = 8 / 16 / 32
#   k_predict_x  (N_h <= 8)              64 * QFA_PX_SPW8 = 64 spectra per block
#   k_predict_x  (N_h = 9..16)           64 * QFA_PX_SPW = 128 spectra per block, a wave holds two groups of 16
#   k_predict_x32 (N_h = 17..32), k_predict_out (F_PREDICT_F32)     64 spectra per block
# so the B edges are 63 / 64 / 65 / 129 everywhere, 127 / 128 / 257 on top at N_h = 9..16, 15 / 16 / 17 for the waves.
PREDICT_GROUP = {8: 64, 16: 128, 32: 64}

# (N_pix, N_h, B): every B edge meets every N_h arm (<= 8 | 9..16 | 17..32) at least once
PREDICT_CASES = [
    (33, 1, 1), (97, 3, 63), (333, 8, 64), (33, 3, 65), (97, 8, 129), (640, 1, 300), (1913, 8, 65), (1920, 8, 63),
    (1913, 3, 17), (1920, 1, 15), (333, 3, 16),
    (33, 9, 1), (97, 13, 63), (333, 16, 64), (33, 16, 65), (97, 9, 129), (640, 13, 300), (333, 9, 127), (97, 16, 128),
    (33, 13, 257), (1913, 16, 15), (1920, 9, 17), (333, 13, 16),
    (33, 17, 1), (97, 32, 63), (333, 17, 64), (33, 32, 65), (97, 17, 129), (640, 32, 300), (1913, 17, 16), (1920, 32, 15),
    (333, 32, 17),
]


def predict_case(npix, nh, B):
    """(p, mu, wav, nb, batch of N >= B resident rows, rows) of a case of PREDICT_CASES.  In batch order (row j of the
    result = resident row rows[j]): masks with runs everywhere; one pixel masked in every spectrum; from 5 rows on a fully
    masked spectrum in the middle (B // 2), a red-only one (row 1) and one with errors of 1e-4 of its flux (row 3 B // 4: the
    high-S/N case of tests/test_posterior_samples.py, where C is worst conditioned)."""
    seed = 7 * npix + 131 * nh + B
    wav, nb, nr = synthetic.wavelength_grid(npix)
    N = B + 7
    p, mu, full, mask, mu_a = _draw(npix, nb, nh, N, seed, wav)
    rows = _rows_of(N, B, seed)
    mask[:, npix // 3] = False
    if B >= 5:
        mask[rows[B // 2], :] = False
        mask[rows[1], :nb] = False
        hi = rows[(3 * B) // 4]
        full["error"][hi] = (np.abs(full["flux"][hi]) * 1e-4 + 1e-12).astype(np.float32)
    return p, mu, wav, nb, _remask(full, mask, mu_a), rows


# (N_pix, N_b, N_h, B): the ragged, boundary and XDL tables of tests/test_hip_parity.py (N_b None: where the grid puts it)
GRADIENT_CASES = [(36, 7, 3, 5), (33, 32, 16, 21), (48, 17, 20, 6), (97, None, 9, 33), (200, None, 16, 70), (333, None, 5, 17),
                  (640, None, 16, 48), (450, None, 1, 65), (260, None, 24, 35), (500, None, 32, 20)]


def thin_pixels(npix):
    """(first, last + 1) of the block of pixels that only the LAST spectrum sees -- it crosses a 16-pixel tile edge --, the
    pixel that no spectrum sees, and the last pixel of the last (ragged) tile, which only the FIRST spectrum sees"""
    p0 = 16 * max(1, npix // 32) - 3
    return (p0, p0 + 6), p0 + 6, npix - 1


def gradient_case(npix, nb, nh, B):
    """(p, mu, wav, nb, batch of N >= B resident rows, rows) of a case of GRADIENT_CASES: masks with runs plus the thin
    coverage of ``thin_pixels`` (batch order: spectrum j = resident row rows[j])."""
    seed = 5 * npix + 17 * nh + B
    if nb is None:
        wav, nb, nr = synthetic.wavelength_grid(npix)
    else:
        wav = np.linspace(1100.0, 1300.0, npix)
    N = B + 5
    p, mu, full, mask, mu_a = _draw(npix, nb, nh, N, seed, wav)
    rows = _rows_of(N, B, seed)
    (a, e), none, last = thin_pixels(npix)
    mask[:, a:e] = False
    mask[rows[B - 1], a:e] = True
    mask[:, none] = False
    mask[:, last] = False
    mask[rows[0], last] = True
    return p, mu, wav, nb, _remask(full, mask, mu_a), rows


def long_case(npix, nh, B):
    """(p, mu, wav, nb, batch of N >= B resident rows, rows) of a case on a long pixel axis: masks with runs, without the
    thin coverage of gradient_case -- an F element of ONE term at N_pix = 2053 is beyond its bar in the float32 oracle
    itself (2e-1 against 2.1e-2: the bar was measured on GRADIENT_CASES), and what these cases are about is the walk"""
    seed = 5 * npix + 17 * nh + B
    wav, nb, nr = synthetic.wavelength_grid(npix)
    N = B + 5
    p, mu, full, mask, mu_a = _draw(npix, nb, nh, N, seed, wav)
    return p, mu, wav, nb, _remask(full, mask, mu_a), _rows_of(N, B, seed)


# ----------------------------------------------------------------------------------------------------------------------
# the N_h = 17..32 step at its walk edges (tests/test_s12_walk_edges.py, tests/test_s12_walk_edges_cpu.py)
# ----------------------------------------------------------------------------------------------------------------------
# (N_pix, N_b, N_h, B); N_b None: the long axis (long_case: the boundary where the grid puts it, no thin pixels).
# N_pix = 149 = 16 k + 5: a ragged last tile of 16 and of 32 pixels; N_b = 55: the boundary inside 32-pixel tile 1.
S12_SHORT = [(149, 55, 17, B) for B in (15, 16, 17, 33, 63, 64, 65, 129, 199)] + [(149, 55, 24, 65), (149, 55, 24, 199)] + \
            [(149, 55, 32, B) for B in (17, 65, 129)]
# 1029 = 33 tiles of 32 pixels (two pass-1 chains of 17 and 16 tiles, the last tile of 5 pixels)
S12_LONG = [(1029, None, 17, 17), (1029, None, 24, 70), (1029, None, 32, 17)]
# item lengths that the two axes above do not give on 256 compute units (s12_census; test_the_cases_reach_the_walk_edges):
# 293 = 10 tiles of 32 pixels: items of 4, 4 and 2 tiles; 389 = 13 tiles: items of 4, 4, 4 and 1 (the ragged tile alone);
# 69 = 5 tiles of 16 pixels with nine blocks of spectra: k_grads_s3 items of 5 tiles, block 8 starts its walk at tile 4 (the
# smallest N_pix B at which the plan gives that kernel a rotation of 4 or more: a small batch is cut into items of <= 5 tiles)
S12_PLAN = [(293, 110, 17, 17), (389, 150, 24, 65), (69, 23, 17, 513)]
# B = 1: every element is ONE term, and the float32 oracle itself is beyond the single-term bars at most (N_b, N_h) -- at N_pix =
# 149, as a fraction of the worst bar: (55, 17) 38.8, (55, 24) 1.55, (55, 32) 49.1, (55, 20) 23.1, (53, 17) 0.28, (40, 17) 0.21,
# (64, 17) 3.6, (70, 17) 1.3, (96, 17) 0.91, (75, 24) 5.7, (100, 24) 18.5, (75, 32) 0.19; the two kept are below 0.5
# (tests/test_s12_walk_edges_cpu.py asserts it): (60, 17) 0.16 and (100, 32) 0.09
S12_B1 = [(149, 60, 17, 1), (149, 100, 32, 1)]
S12_CASES = S12_SHORT + S12_LONG + S12_PLAN + S12_B1
# deterministic accumulation only, zabs form only: 33 slab rows = the second chunk of the fixed-order reducer
S12_DET_CASE = (149, 55, 17, 64 * 32 + 1)
S12_FAST_CASES = [(149, 55, 24, 65), (1029, None, 32, 70)]                      # QFA_F_S3_FAST


def s12_case(npix, nb, nh, B):
    return gradient_case(npix, nb, nh, B) if nb is not None else long_case(npix, nh, B)


K_MAX_SEG = 32                      # kMaxSeg (qfa_host.h)
P1_MAX_CHAIN = 32                   # QFA_P1_MAX_CHAIN
ROT_MUL = 2654435761                # the multiplier of the rotated tile order (qfa_s12_x.h)


def plan_work(B, ntiles, pro, slots, spb=64, max_chain=0):
    """(full, rem, nseg, seg_tiles): plan_work of qfa_host.h, line by line"""
    nblk = (B + spb - 1) // spb
    if max_chain > 0 and ntiles > max_chain:
        nn0 = (ntiles + max_chain - 1) // max_chain
        st = (ntiles + nn0 - 1) // nn0
        return 0, nblk, (ntiles + st - 1) // st, st
    best, best_cost = (0, nblk, 1, ntiles), 1e300
    full = (nblk // slots) * slots
    while full >= 0:
        rem = nblk - full
        for n in range(1, K_MAX_SEG + 1):
            latency_bound = full == 0 and rem * n <= slots // 2
            if n > 1 and ntiles // n < (3 if latency_bound else 8):
                break
            if n > 8 and not latency_bound:
                break
            st = (ntiles + n - 1) // n
            nn = (ntiles + st - 1) // st
            rounds_rem = (rem * nn + slots - 1) // slots if rem else 0           # ((long long) of the C++ double: its floor)
            cost = float(full // slots) * (ntiles + pro) + float(rounds_rem) * (st + pro)
            if cost < best_cost - 1e-9:
                best_cost = cost
                best = (full, rem, nn if rem else 1, st if rem else ntiles)
            if not rem:
                break
        if full == 0:
            break
        full -= slots
    return best


def plan_items(wp, ntiles):
    """[(blk, seg, t0, t1)] of every work item of a plan, in launch order: plan_item of qfa_common.h"""
    full, rem, nseg, st = wp
    out = []
    for item in range(full + rem * nseg):
        if item < full:
            out.append((item, 0, 0, ntiles))
        else:
            j = item - full
            seg = j // rem
            out.append((full + j % rem, seg, seg * st, min(seg * st + st, ntiles)))
    return out


def rot_of(blk, n, window):
    """first tile of the rotated walk of an item of n tiles (k_s12_x: window 4, k_grads_s3: window 32); unsigned 32-bit"""
    return (blk * ROT_MUL) % (1 << 32) % min(n, window) if n > 0 else 0


def s12_plans(npix, B, ncu):
    """{"wp2x": k_s12_x's plan over 32-pixel tiles, "wp2": k_grads_s3's over 16-pixel tiles, "wp1": pass 1's} at N_h = 17..32,
    each (plan, tiles of the axis), as make_layout_t<32> (qfa_host.h) calls plan_work"""
    nt32, nt16 = (npix + 31) // 32, (npix + 15) // 16
    return {"wp2x": (plan_work(B, nt32, 3, ncu), nt32), "wp2": (plan_work(B, nt16, 4, ncu), nt16),
            "wp1": (plan_work(B, nt32, 1, ncu, 64, P1_MAX_CHAIN), nt32)}


def s12_census(cases, ncu):
    """what the walks of k_s12_x and k_grads_s3 meet over ``cases`` on ``ncu`` compute units"""
    c = {"n_x": set(), "wrap_ragged": [], "rot_boundary": [], "rot_s3": set(), "inactive": set(), "nseg1": {}}
    for case in cases:
        npix, nb, nh, B = case
        if nb is None:
            nb = synthetic.wavelength_grid(npix)[1]
        pl = s12_plans(npix, B, ncu)
        wp, nt = pl["wp2x"]
        for blk, seg, t0, t1 in plan_items(wp, nt):
            n = t1 - t0
            c["n_x"].add(n)
            rot = rot_of(blk, n, 4)
            # the walk starts at tile t0 + rot and wraps behind the item's last tile: the ragged last tile of the axis is walked
            # at step n - 1 - rot and tile t0 follows it
            if rot and t1 == nt and npix % 32:
                c["wrap_ragged"].append((case, blk, seg, rot))
            if rot and nb % 32 and t0 <= nb // 32 < t1:
                c["rot_boundary"].append((case, blk, seg, rot))
        wp, nt = pl["wp2"]
        for blk, seg, t0, t1 in plan_items(wp, nt):
            c["rot_s3"].add(rot_of(blk, t1 - t0, 32))
        for blk in range((B + 63) // 64):
            c["inactive"].add(4 - (min(64, B - 64 * blk) + 15) // 16)
        c["nseg1"][case] = pl["wp1"][0][2]
    return c


def assert_s12_census(cases, ncu):
    """the walk edges that tests/test_s12_walk_edges.py is about, reached by ``cases`` on ``ncu`` compute units; returns the census"""
    c = s12_census(cases, ncu)
    nx = c["n_x"]
    # k_s12_x items of 1, 2, 3 and >= 4 tiles, the long ones odd and even (its walk is unrolled by two tiles)
    assert {1, 2, 3} <= nx and any(n >= 4 and n % 2 for n in nx) and any(n >= 4 and n % 2 == 0 for n in nx), (ncu, sorted(nx))
    assert c["wrap_ragged"], ncu                       # rot != 0 and the walk wraps behind the ragged last tile of the axis
    assert {rot for _, _, _, rot in c["wrap_ragged"]} >= {1, 2, 3}, (ncu, c["wrap_ragged"])
    assert c["rot_boundary"], ncu                      # rot != 0 in an item that holds the boundary tile
    assert max(c["rot_s3"]) >= 4, (ncu, sorted(c["rot_s3"]))               # k_grads_s3: a rotation beyond k_s12_x's window
    assert {0, 1, 2, 3} <= c["inactive"], (ncu, sorted(c["inactive"]))     # inactive waves of a block's last spectra
    long_axis = [nseg for case, nseg in c["nseg1"].items() if case[0] == 1029]
    assert len(long_axis) >= 3 and set(long_axis) == {2}, (ncu, c["nseg1"])    # pass 1 in two chains
    return c


def select(batch, rows):
    """the rows of a batch in batch order (what the zabs / zfac input forms are given)"""
    return {k: v[rows] for k, v in batch.items()}


def record(line):
    """QFA_ELEMENTWISE_LOG=<file>: the GPU tests append their achieved maxima there (profiles/elementwise_accuracy.txt)"""
    import os
    path = os.environ.get("QFA_ELEMENTWISE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
