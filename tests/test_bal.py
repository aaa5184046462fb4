"""The BAL finder on the GPU against its numpy restatement (tests/_bal_ref.py): qfa_bal_scan_f32 over the window lengths, N_h, S, B,
smooth and max_gap at which the kernel takes another path and over the run placements of tests/_bal_cases.py, qfa_bal_mask_f32
against bal_intervals -> mask_absorbers, the predict -> scan -> mask iteration, the refusals of the C-ABI and one end-to-end case.

Bars, derived and not tuned (tests/_bal_ref.py): on the rows the reference does not contest -- at least 95 % of them, asserted --
every integer output and every trough edge equals the reference exactly; value and var are within the reference's own bars.  The
achieved fractions of the bars are printed; profiles/bal_accuracy.txt records them."""
import ctypes as C

import numpy as np
import pytest

import _bal_cases as K
import _bal_ref as R
from _segment_harness import F_SYNC, T, dev   # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

FILL = -7.0
E_NULL, E_SIZE, E_FLAGS = -1, -2, -5


def call_scan(dev, g, windows, *, nh, smooth=1, max_gap=0, thr=0.9, indices=K.INDICES, trough_index=1, sel=None, draws=None,
              mask="own", flux=None, error=None, resident=False, nb=K.NB, expect=0, flags=0, null=(), bad=None, nrows=None, stride=None):
    """qfa_bal_scan_f32 by hand.  ``sel``: the spectra of the call; ``draws``: the draws of h; ``resident``: rows of B + 4 in another
    order, a stride of Npix + 7, NaN in what is not named; ``null``: names of pointers to pass as NULL; ``bad``: a function that
    spoils the qfa_bal_t.  Fresh outputs hold FILL.  Returns a dict of numpy arrays."""
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    sel = np.arange(g["flux"].shape[0]) if sel is None else np.asarray(sel)
    h = g["h"][sel] if draws is None else g["h"][sel][:, draws]
    B, S, npix = len(sel), h.shape[1], g["npix"]
    fl = (g["flux"] if flux is None else flux)[sel]
    er = (g["error"] if error is None else error)[sel]
    mk = g["mask"][sel] if isinstance(mask, str) else (None if mask is None else np.asarray(mask, bool)[sel])
    bs = _lib.Batch()
    keep = []
    if resident:
        N, wide = B + 4, npix + 7
        rows = np.random.default_rng(3).permutation(N)[:B].astype(np.int32)
        fr, err_ = np.full((N, wide), np.nan, np.float32), np.full((N, wide), np.nan, np.float32)
        mr = np.ones((N, wide), bool)
        fr[rows, :npix], err_[rows, :npix] = fl, er
        if mk is not None:
            mr[rows, :npix] = mk
        tf, te, tm, tr = T(fr, dev), T(err_, dev), (None if mk is None else T(mr, dev)), T(rows, dev)
        bs.rows, bs.row_stride = tr.data_ptr(), wide if stride is None else stride   # (``stride``: what the call is TOLD)
        keep.append(tr)
    else:
        tf, te, tm = T(fl, dev), T(er, dev), None if mk is None else T(mk, dev)
        bs.row_stride = 0
    bs.delta, bs.error, bs.mask = tf.data_ptr(), te.data_ptr(), None if tm is None else tm.data_ptr()
    tF, tmu, th = T(g["F"], dev), T(g["mu"], dev), T(np.ascontiguousarray(h), dev)
    q, kept = params_of(windows, dev, indices, thr, smooth, max_gap, trough_index)
    keep += kept
    if bad is not None:
        bad(q)
    L, I = len(windows), len(indices)
    B = B if nrows is None else nrows
    out = {"value": torch.full((B, S, L, I), FILL, dtype=torch.float64, device=dev),
           "var": torch.full((B, S, L, I), FILL, dtype=torch.float64, device=dev),
           "counts": torch.full((B, S, L, I, 3), int(FILL), dtype=torch.int32, device=dev),
           "line_counts": torch.full((B, S, L, 2), int(FILL), dtype=torch.int32, device=dev),
           "troughs": torch.full((B, S, L, R.MAX_TROUGHS, 2), FILL, dtype=torch.float64, device=dev)}
    ptr = lambda name, t: None if name in null else C.c_void_p(t.data_ptr())
    st = lib.qfa_bal_scan_f32(ptr("F", tF), ptr("mu", tmu), None if "b" in null else C.byref(bs), ptr("h", th), B, S, npix, nb, nh,
                              None if "q" in null else C.byref(q), K.CONT_MIN, flags, *(ptr(k, v) for k, v in out.items()),
                              _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert st == expect, st
    return {k: v.cpu().numpy() for k, v in out.items()}


def params_of(windows, dev, indices=K.INDICES, thr=0.9, smooth=1, max_gap=0, trough_index=1):
    """(qfa_bal_t, the device tensors it points to)"""
    import torch
    from qfa_amd import _lib
    q, keep = _lib.BalParams(), []
    q.n_lines, q.n_indices = len(windows), len(indices)
    for l, (p_lo, p_hi, vedge) in enumerate(windows):
        t = torch.tensor(np.asarray(vedge, np.float64), device=dev)
        keep.append(t)
        q.p_lo[l], q.p_hi[l], q.vedge[l] = p_lo, p_hi, t.data_ptr()
    for x, d in enumerate(indices):
        q.index[x] = _lib.BalIndex(*d)
    q.thr, q.smooth, q.max_gap, q.trough_index = thr, smooth, max_gap, trough_index
    return q, keep


def bits(a):
    return {k: v.view(np.int64 if v.dtype == np.float64 else v.dtype) for k, v in a.items()}


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(bits(a)[k], bits(b)[k]), (what, k)


def judge(got, r, what):
    """integers and trough edges exact, value and var within the bars, on the uncontested rows (>= 95 %); returns the worst fractions"""
    ok = ~r["contested"]
    assert ok.mean() >= 0.95, (what, float(ok.mean()))
    assert np.array_equal(got["counts"][ok], r["counts"][ok]), what
    assert np.array_equal(got["line_counts"][ok], r["line_counts"][ok]), what
    assert np.array_equal(np.isnan(got["troughs"][ok]), np.isnan(r["troughs"][ok])), what
    assert np.array_equal(np.nan_to_num(got["troughs"][ok], nan=-1.0), np.nan_to_num(r["troughs"][ok], nan=-1.0)), what
    worst = []
    for k in ("value", "var"):
        err, bar = np.abs(got[k][ok] - r[k][ok]), r[k + "_bar"][ok]
        frac = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0))) if err.size else 0.0
        print(f"bal_scan {what}: {k}: rows {int(ok.sum())} of {ok.size}, worst fraction of the bar {frac:.3f}, "
              f"largest value {float(np.max(np.abs(r[k][ok]), initial=0.0)):.6g}")
        assert np.all(err <= bar), (what, k, frac, float(np.max(err)))
        worst.append(frac)
    return worst


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "win{}-nh{}-S{}-B{}-smooth{}-gap{}-p{}".format(*c))
def test_scan_against_the_reference(dev, case):
    n_win, nh, S, B, smooth, max_gap, first = case
    g = K.inputs(n_win, nh, S, B, first)
    w = K.windows_of(g["wav"], g["p_lo"], g["p_hi"])
    r = K.reference(case)
    kw = dict(nh=nh, smooth=smooth, max_gap=max_gap)
    got = call_scan(dev, g, w, **kw)
    judge(got, r, "win{}-nh{}-S{}-B{}-smooth{}-gap{}-p{}".format(*case))
    same_bits(got, call_scan(dev, g, w, **kw), "two calls")
    # NaN / inf / -999 under the mask change nothing
    rng = np.random.default_rng(5)
    junk = np.array([np.nan, np.inf, -np.inf, -999.0], np.float32)
    fj = np.where(g["mask"], g["flux"], junk[rng.integers(0, 4, g["mask"].shape)])
    ej = np.where(g["mask"], g["error"], junk[rng.integers(0, 4, g["mask"].shape)])
    same_bits(got, call_scan(dev, g, w, flux=fj, error=ej, **kw), "junk under the mask")
    same_bits(got, call_scan(dev, g, w, resident=True, **kw), "the resident form")
    if S > 1:                                                  # draw s alone
        for s in (0, S - 1):
            one = call_scan(dev, g, w, draws=[s], **kw)
            same_bits({k: v[:, s:s + 1] for k, v in got.items()}, one, f"draw {s} alone")
    if B > 1:                                                  # a spectrum alone
        b = B - 1
        one = call_scan(dev, g, w, sel=[b], **kw)
        same_bits({k: v[b:b + 1] for k, v in got.items()}, one, f"spectrum {b} alone")


def test_several_draws_in_one_wave_equal_every_draw_alone(dev):
    """B L S large enough that a wave walks four draws one after the other, reusing its LDS arrays and counters: every output of every
    draw equals, to the bit, that draw scanned as a spectrum of its own (a call in which no wave walks more than one draw)"""
    n_win, nh, S, B, smooth, max_gap = 65, 8, 200, 40, 1, 3      # (smooth 3 with several draws per wave: the S = 700 case)
    assert K.draws_per_wave(B, 2, S) == 4 and K.draws_per_wave(B * S, 2, 1) == 1 and K.draws_per_wave(3, 2, 700) == 2
    g = K.inputs(n_win, nh, S, B, 0)
    w = K.windows_of(g["wav"], g["p_lo"], g["p_hi"])
    kw = dict(nh=nh, smooth=smooth, max_gap=max_gap)
    got = call_scan(dev, g, w, **kw)
    rep = lambda a: np.repeat(a, S, axis=0)
    alone = call_scan(dev, dict(g, flux=rep(g["flux"]), error=rep(g["error"]), mask=rep(g["mask"]), h=g["h"].reshape(B * S, 1, nh)), w, **kw)
    same_bits({k: v.reshape((B * S, 1) + v.shape[2:]) for k, v in got.items()}, alone, "draws in one wave")
    # the draws differ among themselves, and runs, bridges and capped trough lists are all present
    assert len({got["value"][0, s].tobytes() for s in range(S)}) > S // 2
    assert got["counts"][..., 1].min() == 0 and got["counts"][..., 2].max() > 0 and got["line_counts"][..., 1].max() > R.MAX_TROUGHS
    assert (got["line_counts"][..., 0] == 0).any()


def test_every_pattern_is_judged_with_runs():
    """the cases hold > 8 troughs with a capped list, bridged pixels, a fully masked window, and every setting"""
    refs = [K.reference(c) for c in K.CASES]
    assert max(int(r["line_counts"][..., 1].max()) for r in refs) > R.MAX_TROUGHS
    assert any(r["counts"][..., 2].sum() > 0 for r in refs) and any((r["line_counts"][..., 0] == 0).any() for r in refs[1:])
    for col, vals in ((0, (1, 63, 64, 65, 128, 129, 200)), (1, (1, 8, 17, 32)), (2, (1, 3, 5)), (3, (1, 3, 70)), (4, (1, 3, 5)), (5, (0, 1, 3))):
        assert {c[col] for c in K.CASES} >= set(vals), col


def test_window_cut_by_the_grid_and_empty_window(dev):
    """p_lo = Nb and p_hi = Npix: the window is the whole grid; an empty window writes zeros and NaN troughs"""
    n_win, nh = 70, 8
    g = K.inputs(n_win, nh, 3, 3, 1)
    npix = g["npix"]
    w = [(0, npix, R.window(g["wav"], K.LINES[0], 0, npix)), (5, 5, np.zeros(1))]
    r = R.bal_scan(g["F"], g["mu"], g["flux"], g["error"], g["mask"], g["h"], w, K.INDICES, smooth=3, max_gap=1, cont_min=K.CONT_MIN,
                   trough_index=1)
    got = call_scan(dev, g, w, nh=nh, smooth=3, max_gap=1, nb=0)
    judge(got, r, "grid-cut window")
    assert not got["value"][:, :, 1].any() and not got["counts"][:, :, 1].any() and not got["line_counts"][:, :, 1].any()
    assert np.isnan(got["troughs"][:, :, 1]).all()
    none = call_scan(dev, g, w, nh=nh, nb=0, nrows=0)
    assert all(v.size == 0 for v in none.values())


def test_loud_failures(dev):
    g = K.inputs(65, 8, 1, 3, 0)
    w = K.windows_of(g["wav"], g["p_lo"], g["p_hi"])

    def refused(code, **kw):
        got = call_scan(dev, g, w, nh=kw.pop("nh", 8), expect=code, **kw)
        for k, v in got.items():
            assert (v == FILL).all(), (kw, k)

    for name in ("F", "mu", "b", "h", "q", "value", "var", "counts", "line_counts", "troughs"):
        refused(E_NULL, null=(name,))
    refused(E_NULL, bad=lambda q: q.vedge.__setitem__(1, None))
    refused(E_SIZE, nh=33)
    refused(E_SIZE, nb=g["p_lo"] + 1)                          # a blue-side window
    refused(E_SIZE, smooth=2)
    refused(E_SIZE, smooth=17)
    refused(E_SIZE, max_gap=17)
    refused(E_SIZE, thr=0.0)
    refused(E_SIZE, trough_index=2)
    refused(E_SIZE, bad=lambda q: setattr(q, "n_lines", 5))
    refused(E_SIZE, bad=lambda q: setattr(q, "n_indices", 0))
    refused(E_SIZE, bad=lambda q: q.p_hi.__setitem__(0, g["npix"] + 1))
    refused(E_SIZE, bad=lambda q: (q.p_lo.__setitem__(0, 0), q.p_hi.__setitem__(0, 0)), nb=1)
    refused(E_SIZE, indices=((5000.0, 3000.0, 100.0, R.WHOLE),), trough_index=0)
    refused(E_SIZE, indices=((0.0, 3000.0, 100.0, 7),), trough_index=0)
    refused(E_FLAGS, flags=0x80)
    refused(E_NULL, flags=0x80, null=("q",))                   # the first failing check decides
    refused(E_SIZE, flags=0x80, nh=33)
    # a window longer than the cap
    from qfa_amd import _lib
    big = _lib.BAL_MAX_WIN + 1
    gb = dict(g, npix=big + 4)
    refused_big = call_scan(dev, dict(gb, flux=np.ones((1, big + 4), np.float32), error=np.ones((1, big + 4), np.float32),
                                      mask=np.ones((1, big + 4), bool), F=np.zeros((big + 4, 8), np.float32), mu=np.ones(big + 4, np.float32),
                                      h=g["h"][:1]), [(2, 2 + big, np.arange(big + 1, dtype=np.float64))], nh=8, expect=E_SIZE)
    assert all((v == FILL).all() for v in refused_big.values())
    # a row stride shorter than a row; more than 2^30 (spectrum, draw, line) rows (refused before anything is read)
    too_short = call_scan(dev, g, w, nh=8, resident=True, stride=g["npix"] - 1, expect=E_SIZE)
    assert all((v == FILL).all() for v in too_short.values())
    st = _lib.lib().qfa_bal_scan_f32(None, None, C.byref(_lib.Batch()), None, 1 << 20, 1 << 10, g["npix"], 0, 8, C.byref(params_of(w, dev)[0]),
                                      0.0, 0, None, None, None, None, None, None)
    assert st == E_SIZE
    assert _lib.lib().qfa_bal_scan_f32(None, None, C.byref(_lib.Batch()), None, 1 << 19, 1 << 10, g["npix"], 0, 8,
                                        C.byref(params_of(w, dev)[0]), 0.0, 0, None, None, None, None, None, None) == E_NULL
    # the mask call
    import torch
    lib = _lib.lib()
    lam = (C.c_double * 4)(*R_LINES)
    tr = torch.full((3, 1, 2, 8, 2), float("nan"), dtype=torch.float64, device=dev)
    wv = torch.tensor(g["wav"], device=dev)
    mo = torch.ones((3, g["npix"]), dtype=torch.bool, device=dev)
    nm = torch.full((3,), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda **k: lib.qfa_bal_mask_f32(k.get("mask_in"), k.get("wav", p(wv)), k.get("tr", p(tr)), k.get("B", 3), 1, k.get("L", 2),
                                            k.get("s_ref", 0), g["npix"], k.get("lam", lam), k.get("nlam", 4), k.get("pad", 0.0),
                                            k.get("out", p(mo)), p(nm), _lib.current_stream(dev))
    assert call(s_ref=1) == E_SIZE and call(L=5) == E_SIZE and call(nlam=0) == E_SIZE and call(pad=-1.0) == E_SIZE
    assert call(pad=float("nan")) == E_SIZE and call(lam=None) == E_NULL and call(wav=None) == E_NULL and call(out=None) == E_NULL
    assert call(B=0, wav=None) == 0
    torch.cuda.synchronize()
    assert (nm.cpu().numpy() == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (nm.cpu().numpy() == 0).all() and mo.all()


R_LINES = (1549.06, 1396.76, 1240.81, 1215.67)


@pytest.mark.parametrize("pad", [0.0, 300.0])
def test_mask_equals_the_host_route(dev, pad):
    """qfa_bal_mask_f32 == bal_intervals -> mask_absorbers(rest=..., correct=False) as a boolean array, all four mask lines"""
    import torch
    from qfa_amd.absorbers import BAL_LINES, mask_absorbers
    from qfa_amd.bal import BALScan, bal_mask
    assert tuple(BAL_LINES) == R_LINES
    rng = np.random.default_rng(8)
    B, S, L, npix = 9, 2, 2, 1500
    wav = 10 ** (np.log10(1100.0) + 1.2e-4 * np.arange(npix))
    tr = np.full((B, S, L, 8, 2), np.nan)
    for b in range(B):
        for s in range(S):
            for l in range(L):
                k = int(rng.integers(0, 9)) if b else 8
                v0 = np.sort(rng.uniform(0.0, 24000.0, k))
                tr[b, s, l, :k, 0], tr[b, s, l, :k, 1] = v0, v0 + rng.uniform(100.0, 3000.0, k)
    # edges that fall exactly on grid wavelengths: v = c (1 - wav / lam)
    tr[1, 1, 0, 0] = (R.C_KMS * (1.0 - wav[900] / 1549.06), R.C_KMS * (1.0 - wav[880] / 1549.06))
    mask = rng.random((B, npix)) > 0.1
    ttr = torch.tensor(tr, device=dev)
    out, nm = bal_mask(T(mask, dev), wav, ttr, draw=1, lines=BAL_LINES, pad_kms=pad)
    ref_out, ref_n = R.bal_mask(mask, wav, tr, 1, BAL_LINES, pad)
    assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(nm.cpu().numpy(), ref_n) and ref_n.sum() > 1000
    # the host route
    zero = torch.zeros((B, S, L, 2), dtype=torch.float64, device=dev)
    scan = BALScan(zero + 1.0, zero, torch.zeros((B, S, L, 2, 3), dtype=torch.int32, device=dev),
                   torch.zeros((B, S, L, 2), dtype=torch.int32, device=dev), ttr, (1549.06, 1396.76), {"BI": R.BI[:3] + ("after",), "AI": R.AI[:3] + ("whole",)},
                   "AI", 0.9)
    rest = scan.to_intervals(line=None, draw=1, pad_kms=pad, lines=BAL_LINES)
    flux = np.where(mask, 1.0, -999.0).astype(np.float32)
    fo, _, rec = mask_absorbers(flux, flux, np.full(B, 2.5), wav, rest=rest, correct=False, device=dev)
    assert np.array_equal(fo.cpu().numpy() != -999.0, out.cpu().numpy())
    assert np.array_equal(rec["n_interval_masked"].cpu().numpy(), nm.cpu().numpy())
    # in place, and no mask given
    tm = T(mask, dev)
    o2, _ = bal_mask(tm, wav, ttr, draw=1, lines=BAL_LINES, pad_kms=pad, out=tm)
    assert o2 is tm and np.array_equal(tm.cpu().numpy(), ref_out)
    o3, n3 = bal_mask(None, wav, ttr, draw=0, lines=BAL_LINES[:1], pad_kms=pad)
    r3, rn3 = R.bal_mask(None, wav, tr, 0, BAL_LINES[:1], pad)
    assert np.array_equal(o3.cpu().numpy(), r3) and np.array_equal(n3.cpu().numpy(), rn3)


def _bal_model(dev, B, seed, inject=True):
    """a model on a coarse rest-frame grid, spectra drawn as mu + F h + noise, every second one with a C IV trough of 6 000 km/s"""
    from qfa_amd import QFA, synthetic
    nh, step = 4, 6e-4
    wav = 10 ** np.arange(np.log10(1100.0), np.log10(1620.0), step)
    npix, nb = len(wav), int(np.sum(wav < synthetic.LYA))
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    p["Psi"] = np.where(np.arange(npix) >= nb, 1e-4, p["Psi"]).astype(np.float32)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1, masks=False)
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    m.mu = T(mu, dev)
    # the red side: the model's own continuum of a known h plus 2 % noise, so that r = 1 +- 0.02 outside a trough
    rng = np.random.default_rng(seed + 2)
    h = rng.normal(0, 1, (B, nh))
    b["error"] = b["error"].copy()
    b["error"][:, nb:] = 0.02
    flux = b["flux"].copy()
    flux[:, nb:] = (mu[None, nb:] + h @ p["F"][nb:].T.astype(np.float64)) + 0.02 * rng.normal(0, 1, (B, npix - nb))
    v = R.C_KMS * (1.0 - wav / 1549.06)
    if inject:
        flux[::2, (v > 8000.0) & (v < 14000.0)] *= 0.4
    return m, wav, b, flux.astype(np.float32)


def test_model_entry_point_iteration_and_resident_form(dev):
    import torch
    from qfa_amd._lib import QFAHipError
    from qfa_amd.bal import BALScan, bal_mask
    from qfa_amd.resident import ResidentBatch
    B = 6
    m, wav, b, flux = _bal_model(dev, B, 21)
    tf, te, tz = T(flux, dev), T(b["error"], dev), T(b["zabs"], dev)
    tm = torch.ones((B, len(wav)), dtype=torch.bool, device=dev)
    kw = dict(wav_grid=wav, n_samples=3, seed=4, offset=10, smooth=3, max_gap=1)
    two = m.bal_scan(tf, te, tm, zabs=tz, n_iter=2, pad_kms=300.0, **kw)
    assert isinstance(two, BALScan) and two.S == 3 and tuple(two.value.shape) == (B, 3, 2, 2)
    # the manual composition: predict -> scan -> mask -> predict -> scan
    _, hm, hc, _, _ = m.predict(tf, te, tz, tm)
    first = m.bal_scan(tf, te, tm, hmean=hm, hcov=hc, **kw)
    mask2, nm = bal_mask(tm, wav, first.troughs, draw=0, pad_kms=300.0)
    _, hm2, hc2, _, _ = m.predict(tf, te, tz, mask2)
    second = m.bal_scan(tf, te, tm, hmean=hm2, hcov=hc2, **kw)           # (the scan reads the caller's mask, the predict the new one)
    for name in ("value", "var", "counts", "line_counts"):
        assert torch.equal(getattr(two, name), getattr(second, name)), name
    assert torch.equal(two.troughs.view(torch.int64), second.troughs.view(torch.int64))
    assert torch.equal(two.mask, mask2) and torch.equal(two.n_masked, nm) and int(nm[0]) > 0 and int(nm[1]) == 0
    # masking its own troughs raises a BAL quasar's continuum: the second pass finds at least the first one's absorption
    assert float(second.ai()[0, 0, 0]) >= float(first.ai()[0, 0, 0]) > 0.0
    # the resident form of the first pass gives the same bits
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    nb = m.Nb
    zq1 = T((1.0 + b["zqso"]).astype(np.float32), dev)
    ratio = T((wav[:nb] / 1215.67).astype(np.float32), dev)
    rb = ResidentBatch(tf, None, te, tm, zq1, ratio, rows, len(wav), nb)
    res = m.bal_scan(batch=rb, hmean=hm, hcov=hc, **kw)
    assert torch.equal(res.value, first.value) and torch.equal(res.counts, first.counts)
    with pytest.raises(QFAHipError):
        m.bal_scan(batch=rb, n_iter=2, **kw)
    with pytest.raises(QFAHipError):
        m.bal_scan(tf, te, tm, hmean=hm, n_iter=2, wav_grid=wav)
    with pytest.raises(QFAHipError):
        m.bal_scan(tf, te, tm, hmean=hm, wav_grid=wav, lines=(1215.67,))      # a window on the blue side


def test_end_to_end_injected_trough(dev, tmp_path):
    """a spectrum with an injected C IV trough of 6 000 km/s gets BI > 0 and AI > BI, its Ly-alpha and N V images are masked after
    to_intervals -> mask_absorbers; a clean spectrum gets BI = 0 and no interval; the catalogue walks a loader to the same result"""
    from qfa_amd import io
    from qfa_amd.absorbers import mask_absorbers
    from qfa_amd.dataloader import DeviceDataloader
    B = 8
    m, wav, b, flux = _bal_model(dev, B, 33)
    loader = DeviceDataloader(flux, b["error"], b["zqso"], wav, batch_size=B, device=dev, shuffle=False)
    scan = m.bal_catalog(loader, smooth=3, batch_size=5)
    assert scan.B == B
    bi, ai = scan.bi()[:, 0, 0].cpu().numpy(), scan.ai()[:, 0, 0].cpu().numpy()
    print("BI", bi, "AI", ai)
    assert np.all(bi[::2] > 0.0) and np.all(ai[::2] > bi[::2]) and np.all(bi[1::2] == 0.0)
    assert np.all((bi[::2] > 1000.0) & (bi[::2] < 3500.0))                 # (1 - 0.4 / 0.9) (6 000 - 2 000) = 2 222 km/s, on 414 km/s pixels
    assert scan.is_bal("BI", min_value=500.0)[:, 0].cpu().numpy().tolist() == [True, False] * (B // 2)
    rest = scan.to_intervals(line=0, min_value=500.0, pad_kms=200.0)
    assert all(len(rest[i]) == 0 for i in range(1, B, 2)) and all(len(rest[i]) >= 4 for i in range(0, B, 2))
    fo, _, rec = mask_absorbers(flux, b["error"], b["zqso"], wav, rest=rest, correct=False, device=dev)
    gone = fo.cpu().numpy() == -999.0
    for lam in (1240.81, 1215.67, 1549.06):
        v = R.C_KMS * (1.0 - wav / lam)
        core = (v > 9000.0) & (v < 13000.0)
        assert gone[::2][:, core].all() and not gone[1::2].any(), lam
    # the catalogue does not depend on the batch size, and goes through the csv
    again = m.bal_catalog(loader, smooth=3, batch_size=B)
    assert np.array_equal(scan.value.cpu().numpy(), again.value.cpu().numpy())
    names = [f"spec-{i}.npz" for i in range(B)]
    path = io.write_bal_csv(str(tmp_path / "bal.csv"), scan.to_table(names, min_value=500.0))
    back = io.bal_rest_intervals(names, io.read_bal_csv(path), pad_kms=200.0)
    assert all(np.array_equal(x, y) for x, y in zip(back, rest))


def test_catalog_with_iterations_equals_bal_scan(dev):
    """bal_catalog(n_iter = 2) walks the loader's tensors in slices and equals one bal_scan(n_iter = 2) of the same rows, bit for bit"""
    import torch
    from qfa_amd.dataloader import DeviceDataloader
    B = 6
    m, wav, b, flux = _bal_model(dev, B, 41)
    loader = DeviceDataloader(flux, b["error"], b["zqso"], wav, batch_size=B, device=dev, shuffle=False)
    kw = dict(n_samples=2, seed=9, smooth=3, n_iter=2, pad_kms=150.0)
    cat = m.bal_catalog(loader, batch_size=4, **kw)
    f, e, z, mk, paths = loader.get_rows(0, B)
    a = m.bal_scan(f[:4], e[:4], mk[:4], zabs=z[:4], wav_grid=wav, offset=0, **kw)
    c = m.bal_scan(f[4:], e[4:], mk[4:], zabs=z[4:], wav_grid=wav, offset=4, **kw)
    for name in ("value", "var", "counts", "line_counts", "mask", "n_masked"):
        assert torch.equal(getattr(cat, name), torch.cat([getattr(a, name), getattr(c, name)])), name
    assert cat.names == [str(p) for p in paths] and int(cat.n_masked[0]) > 0 and int(cat.n_masked[1]) == 0
    one = m.bal_catalog(loader, batch_size=4, **dict(kw, n_iter=1))
    assert float(cat.ai()[0, 0, 0]) >= float(one.ai()[0, 0, 0]) > 0.0


def test_predict_mode_writes_the_catalogue(dev, tmp_path):
    """MODEL.BAL: predict mode writes bal_catalog.csv and bal_scan.npz, the rows of QFA.bal_catalog on the same loader"""
    from _segment_harness import cli_predict_case
    from qfa_amd import cli, io
    c = cli_predict_case(dev, tmp_path)
    out = tmp_path / "out"
    assert cli.main(c.argv(out, "MODEL.BAL", "True", "MODEL.BAL_SMOOTH", "3", "MODEL.BAL_MAX_GAP", "1", "MODEL.N_SAMPLES", "2")) == 0
    z = np.load(out / "bal_scan.npz")
    assert z["value"].shape == (len(c.names), 2, 2, 2) and list(z["index_names"]) == ["BI", "AI"] and np.isfinite(z["value"]).all()
    t = io.read_bal_csv(str(out / "bal_catalog.csv"))
    listed = (z["value"][:, 0, :, 1] > 0.0) * np.minimum(z["n_troughs"][:, 0], 8)
    assert len(t["file"]) == int(listed.sum()) and set(t["file"]) <= set(c.names)
    for f, lam, v0, v1, ai in zip(t["file"], t["line"], t["v_min"], t["v_max"], t["ai"]):
        i, l = c.names.index(f), [1549.06, 1396.76].index(lam)
        assert ai == z["value"][i, 0, l, 1] and any((tr[0] == v0) and (tr[1] == v1) for tr in z["troughs"][i, 0, l])


def test_preprocess_command_masks_a_bal_catalogue(dev, tmp_path):
    """python -m qfa_amd.preprocess --bal_catalog: the listed troughs, widened by --bal_pad_kms, become the sentinel in every line's
    image of the spectrum they belong to and nowhere else"""
    from qfa_amd import io
    from qfa_amd.absorbers import bal_intervals
    from qfa_amd.preprocess import main
    raw, out = tmp_path / "raw", tmp_path / "prepared"
    raw.mkdir()
    wave = 10 ** np.arange(np.log10(3500.0), np.log10(5800.0), 1e-4)
    for name in ("a.npz", "b.npz"):
        np.savez(raw / name, wave=wave, flux=np.ones(len(wave), np.float32), ivar=np.full(len(wave), 100.0, np.float32), z=2.5)
    (tmp_path / "obs.csv").write_text("file\na.npz\nb.npz\n")
    io.write_bal_csv(str(tmp_path / "bal.csv"), {"file": ["a.npz", "a"], "line": [1549.06] * 2, "v_min": [5000.0, 15000.0],
                                                 "v_max": [9000.0, 15500.0], "bi": [1.0, 1.0], "ai": [2.0, 2.0]})
    assert main(["--catalog", str(tmp_path / "obs.csv"), "--data_dir", str(raw), "--output_dir", str(out), "--loglam_delta", "1e-3",
                 "--bal_catalog", str(tmp_path / "bal.csv"), "--bal_pad_kms", "100", "--device", str(dev)]) == 0
    grid = io.wavelength_grid(1030.0, 1600.0, 1e-3)
    fa, fb = np.load(out / "a.npz")["flux"], np.load(out / "b.npz")["flux"]
    iv = bal_intervals(np.array([5000.0, 15000.0]) - 100.0, np.array([9000.0, 15500.0]) + 100.0)
    inside = np.any((grid[None, :] >= iv[:, :1]) & (grid[None, :] < iv[:, 1:]), axis=0)
    assert inside.sum() > 15 and (fb != -999.0).sum() > 150
    assert np.array_equal(fa == -999.0, (fb == -999.0) | inside)
