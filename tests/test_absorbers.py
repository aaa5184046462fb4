"""Absorber masking on the GPU (qfa_absorber_mask_f32) against the float64 restatement tests/_absorber_ref.py.

Bars: the mask pattern and the six integers exact; kept pixels (and the transmission) within 1 float32 ulp -- both sides hold T in
float64 to about 1e-14 relative, so they can differ only across a float32 rounding boundary; under mask-only the input's bits;
snr within (n 2^-52 + 2 (2^-23 + 2^-46)) sum |terms| / n: the float64 sum in another order, plus terms flux / error whose two
inputs are each within 1 ulp (2^-23 relative at most).  The absorber decision is a threshold: every case first asserts on the
restatement that no T at a valid pixel lies within 1e-9 of t_min.  No pixel is excluded from a comparison."""
import functools

import numpy as np
import pytest
import torch

import _absorber_ref as R
import _preprocess_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16                                                    # kTileAbs of qfa_amd/csrc/qfa_absorber.h: absorbers per LDS tile
N_ABS = (0, 1, 2, TILE + 1)


def _grid(npix):
    """(grid, snr window): one pixel inside the default window; 40 and 257 pixels across Ly-alpha; the SDSS grid"""
    if npix == 1:
        return np.array([1275.5]), (1270.0, 1600.0)
    if npix == 1913:
        from qfa_amd import synthetic
        return np.asarray(synthetic.wavelength_grid()[0], dtype=np.float64), (1270.0, 1600.0)
    return 1180.0 * 10 ** (1e-4 * np.arange(npix)), (1181.0, 1240.0)


@functools.lru_cache(maxsize=None)
def _case(N, npix, seed, lyb=True, correct=True, t_min=0.8):
    """N spectra with every kind of absorber list, invalid pattern and interval; inputs and the restatement's outputs"""
    rng = np.random.default_rng(seed)
    grid, snr_window = _grid(npix)
    zq = np.array([2.0 + 0.13 * (i % 7) for i in range(N)])
    flux = rng.normal(1.0, 0.2, (N, npix)).astype(np.float32)
    error = rng.uniform(0.05, 0.3, (N, npix)).astype(np.float32)
    for i in range(N):
        pat = (i // 2) % 6 if N > 1 else (2 if npix > 1 else 0)
        if pat == 1 and N > 3:
            flux[i] = error[i] = -999.0                      # a row entirely invalid
        elif pat == 2:
            flux[i, ::7], error[i, ::7] = -999.0, np.nan     # NaN / inf under the sentinel of the other array
        elif pat == 3:
            error[i, 1::5], flux[i, 1::5] = -999.0, np.inf
        elif pat == 4:
            flux[i, :5] = error[i, :5] = -999.0              # leading and trailing runs
            flux[i, npix - 3:] = -999.0
            error[i, npix - 3:] = -np.inf
    rows, lo_g, hi_g = [], min(grid[0], 1200.0), min(grid[-1], 1210.0)
    for i in range(N):
        n_abs = N_ABS[i % 4] if N > 1 else 2
        row = []
        for j in range(n_abs):
            kind = (i + j) % 3
            if kind == 0:
                za = zq[i] - 0.002                           # just below z_q: its wing reaches the blue end of the red side
            elif kind == 1:
                za = rng.uniform(lo_g, hi_g) * (1 + zq[i]) / 1215.67 - 1.0      # well below: somewhere on the grid's forest
            else:
                za = zq[i] + 0.05                            # above z_q: the line sits redward of the quasar's Ly-alpha
            lg = rng.uniform(19.0, 19.8) if n_abs > 2 else rng.uniform(19.0, 22.5)
            row.append((za, lg))
        rows.append(row)
    a_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = np.array([p for r in rows for p in r], dtype=np.float64).reshape(-1, 2)
    # interval edges that coincide exactly with pixel centres: [lo, hi) takes the first and leaves the second
    lam0 = grid * (1.0 + zq[0])
    k1, k2 = (npix // 3, npix // 3 + max(1, npix // 20)) if npix > 1 else (0, 0)
    obs = np.array([[lam0[k1], lam0[k2]], [lam0[-1], lam0[-1] + 1.0]]) if npix > 1 else np.array([[lam0[0] + 1.0, lam0[0] + 2.0]])
    rest, r_off = [], [0]
    for i in range(N):
        mine = []
        if i % 3 == 1 and npix > 4:
            mine = [(grid[2], grid[4])]
        elif i % 3 == 2 and npix > 30:
            mine = [(grid[npix - 9], grid[npix - 6]), (grid[10], grid[11])]
        rest += mine
        r_off.append(len(rest))
    rest, r_off = np.array(rest, dtype=np.float64).reshape(-1, 2), np.array(r_off, dtype=np.int64)
    ref = R.mask_ref(flux, error, zq, grid, a_off, flat[:, 0], flat[:, 1], obs, r_off, rest, t_min=t_min, lyb=lyb, correct=correct,
                     snr_window=snr_window)
    if t_min > 0.0:                                          # (at t_min = 0 no finite T decides anything: T < 0 never holds)
        R.assert_away_from_threshold(ref, t_min)
    return dict(flux=flux, error=error, z=zq, grid=grid, rows=rows, a_off=a_off, obs=obs, rest=rest, r_off=r_off, ref=ref,
                kw=dict(t_min=t_min, lyb=lyb, correct=correct, snr_window=snr_window))


def _run(c, rows=None, **kw):
    from qfa_amd.absorbers import mask_absorbers
    lo, hi = rows if rows is not None else (0, len(c["z"]))
    rest = (c["r_off"][lo:hi + 1] - c["r_off"][lo], c["rest"][c["r_off"][lo]:c["r_off"][hi]])
    args = dict(c["kw"], dla=c["rows"][lo:hi], sky=c["obs"], rest=rest, device=DEV)
    args.update(kw)
    return mask_absorbers(c["flux"][lo:hi], c["error"][lo:hi], c["z"][lo:hi], c["grid"], **args)


def _host(out):
    fo, eo, rec = out[0], out[1], out[-1]
    d = {k: v.cpu().numpy() for k, v in rec.items()}
    d.update(flux=fo.cpu().numpy(), error=eo.cpu().numpy())
    if len(out) == 4:
        d["trans"] = out[2].cpu().numpy()
    return d


def _within_one_ulp(a, r):
    a, r = np.asarray(a, dtype=np.float32), np.asarray(r, dtype=np.float32)
    ulp = np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(r))).astype(np.float64)
    return np.abs(a.astype(np.float64) - r.astype(np.float64)) <= ulp


def _compare(got, ref, c=None, lo=0, hi=None):
    """every pixel and every record entry of rows lo .. hi - 1 of the restatement; returns the number of kept pixels compared"""
    sl = slice(lo, hi)
    excluded = 0
    for k in ("n_valid", "n_lead", "n_trail", "num_mask", "n_absorber_masked", "n_interval_masked"):
        assert np.array_equal(got[k], ref[k][sl]), (k, got[k], ref[k][sl])
    kept = 0
    for k in ("flux", "error"):
        a, r = got[k], ref[k][sl]
        assert np.array_equal(a == R.SENTINEL, r == R.SENTINEL), k
        m = r != R.SENTINEL
        assert np.all(np.isfinite(r[m]))
        print(f"{k}: {int(m.sum())} kept pixels, {int((a[m] != r[m]).sum())} differ from the restatement in their last bit")
        assert np.all(_within_one_ulp(a[m], r[m])), k
        if c is not None and not c["kw"]["correct"]:
            assert a[m].tobytes() == c[k][sl][m].tobytes(), k                       # mask-only: the input's bits
        kept += int(m.sum())
    if "trans" in got:
        assert np.all(_within_one_ulp(got["trans"], ref["trans"][sl]))
    a, r, n, sab = got["snr"], ref["snr"][sl], ref["n_snr"][sl], ref["snr_abs"][sl]
    assert np.array_equal(np.isnan(a), np.isnan(r))
    m = n > 0
    bar = (n[m] * 2.0 ** -52 + 2.0 * (2.0 ** -23 + 2.0 ** -46)) * sab[m] / n[m]
    print(f"snr: max |d| / bar = {np.max(np.abs(a[m] - r[m]) / bar) if m.any() else 0.0:.3e}")
    assert np.all(np.abs(a[m] - r[m]) <= bar)
    assert excluded == 0
    return kept


@pytest.mark.parametrize("N,npix,seed,lyb,correct", [(1, 1, 0, True, True), (1, 40, 1, True, True), (3, 257, 2, True, True),
                                                      (70, 257, 3, True, True), (70, 257, 4, False, True), (70, 257, 5, True, False),
                                                      (3, 1913, 6, True, True)])
def test_kernel_matches_the_restatement(N, npix, seed, lyb, correct):
    c = _case(N, npix, seed, lyb, correct)
    ref = c["ref"]
    if N == 70:                                              # the mixed calls hold every kind of spectrum and decision
        assert (np.diff(c["a_off"]) == TILE + 1).any() and (np.diff(c["a_off"]) == 0).any()
        assert (ref["n_absorber_masked"] > 0).any() and (ref["n_interval_masked"] > 0).any() and (ref["n_valid"] == 0).any()
        assert (ref["n_lead"] > 0).any() and (ref["n_trail"] > 0).any() and ref["num_mask"].max() >= 2
        both = [(ref["valid_in"][i] & (ref["T"][i] < 0.8) & R.in_intervals(c["grid"] * (1.0 + c["z"][i]), c["obs"])).any()
                for i in range(N)]
        assert any(both)                                     # pixels masked for both reasons: counted as absorber-masked
        assert np.isfinite(ref["snr"]).any()
    if npix > 1:
        k1 = npix // 3                                       # the half-open edges: row 0's pixel at `lo` is masked, the one at `hi` is not
        k2 = k1 + max(1, npix // 20)
        if ref["valid_in"][0, k1]:
            assert ref["flux"][0, k1] == R.SENTINEL
        if ref["valid_in"][0, k2] and ref["T"][0, k2] >= 0.8:
            assert ref["flux"][0, k2] != R.SENTINEL
    kept = _compare(_host(_run(c, return_trans=True)), ref, c)
    assert kept > 0
    _compare(_host(_run(c)), ref, c)                         # trans_out NULL
    f = torch.as_tensor(c["flux"], device=DEV)               # in place
    e = torch.as_tensor(c["error"], device=DEV)
    from qfa_amd.absorbers import mask_absorbers
    rest = (c["r_off"], c["rest"])
    fo, eo, rec = mask_absorbers(f, e, c["z"], c["grid"], dla=c["rows"], sky=c["obs"], rest=rest, out=(f, e), device=DEV, **c["kw"])
    assert fo.data_ptr() == f.data_ptr() and eo.data_ptr() == e.data_ptr()
    _compare(_host((fo, eo, rec)), ref, c)


def test_t_min_zero_keeps_everything_finite_or_masks_it():
    """t_min = 0: only a T that underflowed or is not finite masks; the kept quotients may overflow float32 on both sides alike"""
    c = _case(3, 257, 7, True, True, 0.0)
    got, ref = _host(_run(c)), c["ref"]
    for k in ("n_valid", "n_absorber_masked", "n_interval_masked", "num_mask"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("flux", "error"):
        assert np.array_equal(got[k] == R.SENTINEL, ref[k] == R.SENTINEL)
        fin = np.isfinite(ref[k])
        assert np.array_equal(np.isfinite(got[k]), fin) and np.all(_within_one_ulp(got[k][fin], ref[k][fin]))


def test_rows_do_not_depend_on_the_call():
    c = _case(70, 257, 3)
    whole = _host(_run(c, return_trans=True))
    again = _host(_run(c, return_trans=True))
    for k in whole:
        assert whole[k].tobytes() == again[k].tobytes(), k   # two runs, the same bits
    for cuts in ((0, 1, 70), (0, 35, 70)):
        parts = [_host(_run(c, rows=(a, b), return_trans=True)) for a, b in zip(cuts[:-1], cuts[1:])]
        for k in whole:
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), (k, cuts)


def test_host_side_refusals_on_the_device():
    from qfa_amd._lib import QFAHipError
    from qfa_amd.absorbers import mask_absorbers
    c = _case(3, 257, 2)
    base = dict(device=DEV)
    for bad in (dict(t_min=1.0), dict(t_min=-0.1), dict(b_kms=0.0), dict(snr_window=(1600.0, 1270.0)), dict(sky=[[5.0, 4.0]]),
                dict(sky=[[np.nan, 4.0]]), dict(dla=[[(2.0, 20.3)]]), dict(dla=[[(np.nan, 20.3)], [], []]),
                dict(rest=[[], [], [(1200.0, 1100.0)]])):
        with pytest.raises(QFAHipError):
            mask_absorbers(c["flux"], c["error"], c["z"], c["grid"], **base, **bad)
    with pytest.raises(QFAHipError):
        mask_absorbers(c["flux"], c["error"][:, :-1], c["z"], c["grid"], **base)


@functools.lru_cache(maxsize=None)
def _observed_set():
    """32 synthetic spectra, each resampled onto an observed grid of its own, with a DLA catalogue for every other one"""
    from qfa_amd import synthetic
    npix, B = 512, 32
    wav, nb, _ = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, 8, seed=3)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=33)
    rng = np.random.default_rng(8)
    waves, fl, iv = [], [], []
    for s in range(B):
        z = float(b["zqso"][s])
        n = int(rng.integers(600, 800))
        w = np.linspace(wav[0] * (1 + z) * 0.99, wav[-1] * (1 + z) * 1.01, n)
        m = b["mask"][s]
        f = np.interp(w / (1 + z), wav[m], b["flux"][s][m])
        e = np.interp(w / (1 + z), wav[m], b["error"][s][m])
        v = 1.0 / np.maximum(e, 1e-3) ** 2
        for c0 in rng.integers(50, n - 50, int(rng.integers(0, 3))):
            v[c0:c0 + 12] = 0.0
        waves.append(w); fl.append(f.astype(np.float32)); iv.append(v.astype(np.float32))
    zq = b["zqso"].astype(np.float64)
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    rows = [[(zq[s] * 0.9 - 0.05 * (s % 3), 20.3 + 0.1 * (s % 5))] if s % 2 == 0 else [] for s in range(B)]
    sky = np.array([[wav[40] * (1 + zq[1]), wav[44] * (1 + zq[1])]])
    names = np.array([f"obs-{s}" for s in range(B)])
    return np.concatenate(waves), np.concatenate(fl), np.concatenate(iv), off, zq, names, np.asarray(wav, dtype=np.float64), rows, sky


def test_pass_through_without_a_catalogue():
    from qfa_amd.absorbers import mask_absorbers
    from qfa_amd.preprocess import preprocess
    c = _case(70, 257, 3)
    fo, eo, tr, rec = mask_absorbers(c["flux"], c["error"], c["z"], c["grid"], return_trans=True, device=DEV,
                                     snr_window=c["kw"]["snr_window"])
    valid = (c["flux"] != R.SENTINEL) & (c["error"] != R.SENTINEL)
    for got, src in ((fo, c["flux"]), (eo, c["error"])):
        g = got.cpu().numpy()
        assert g[valid].tobytes() == src[valid].tobytes() and np.all(g[~valid] == R.SENTINEL)
    assert np.all(tr.cpu().numpy() == 1.0)
    assert int(rec["n_absorber_masked"].sum()) == 0 and int(rec["n_interval_masked"].sum()) == 0
    for i in range(70):
        assert tuple(int(rec[k][i]) for k in ("n_valid", "n_lead", "n_trail", "num_mask")) == PR.run_counts(valid[i]), i
    # a Preprocessed input: bit-equal arrays, and the run counts are preprocess's own
    wave, flux, ivar, off, zq, names, wav, _, _ = _observed_set()
    pre = preprocess(wave, flux, ivar, off, zq, wav, device=DEV)
    same = pre.mask_absorbers()
    assert torch.equal(same.flux, pre.flux) and torch.equal(same.error, pre.error) and same.flux.data_ptr() != pre.flux.data_ptr()
    for k in ("n_valid", "n_lead", "n_trail", "num_mask", "ok", "norm", "zqso"):
        assert torch.equal(getattr(same, k), getattr(pre, k)), k
    assert int(same.n_absorber_masked.sum()) == 0 and int(same.n_interval_masked.sum()) == 0
    s0, s1 = same.snr.cpu().numpy(), pre.snr.cpu().numpy()   # the same mean, of float32-rounded terms
    assert np.array_equal(np.isnan(s0), np.isnan(s1)) and np.allclose(s0, s1, rtol=2.0 ** -21, atol=0, equal_nan=True)


def test_preprocessed_mask_absorbers_select_catalog_and_the_loader():
    """`Preprocessed.mask_absorbers` holds the restatement's rows; select / catalog work on it; from_observed(absorbers=...) holds
    the kernel's rows bit for bit and the restatement's selection; absorbers=None is the plain loader bit for bit."""
    from qfa_amd.absorbers import AbsorberCatalog
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.preprocess import preprocess
    wave, flux, ivar, off, zq, names, wav, rows, sky = _observed_set()
    pre = preprocess(wave, flux, ivar, off, zq, wav, device=DEV)
    cat = AbsorberCatalog(rows)
    ref = R.mask_ref(pre.flux.cpu().numpy(), pre.error.cpu().numpy(), zq, wav, cat.offsets, cat.z_abs, cat.log_nhi, sky)
    R.assert_away_from_threshold(ref)
    assert (ref["n_absorber_masked"] > 0).sum() >= 8 and (ref["n_interval_masked"] > 0).any()
    masked = pre.mask_absorbers(dla=cat, sky=sky)
    got = dict(flux=masked.flux.cpu().numpy(), error=masked.error.cpu().numpy(), snr=masked.snr.cpu().numpy(),
               n_absorber_masked=masked.n_absorber_masked.cpu().numpy(), n_interval_masked=masked.n_interval_masked.cpu().numpy())
    for k in ("n_valid", "n_lead", "n_trail", "num_mask"):
        got[k] = getattr(masked, k).cpu().numpy()
    _compare(got, ref)
    assert torch.equal(masked.ok, pre.ok) and torch.equal(masked.norm, pre.norm)
    ok = pre.ok.cpu().numpy().astype(bool)
    snr_min = float(np.nanmedian(ref["snr"]))
    assert np.all(np.abs(ref["snr"][np.isfinite(ref["snr"])] - snr_min) > 1e-6 * snr_min)       # the cut sits on no spectrum
    with np.errstate(invalid="ignore"):
        keep = np.nonzero(ok & (ref["snr"] >= snr_min) & (ref["num_mask"] <= 3))[0]
    assert 4 <= len(keep) < 32
    assert np.array_equal(masked.select(snr_min=snr_min, num_mask=3), keep)
    table = masked.catalog(names)
    assert len(table) == int(ok.sum()) and np.array_equal(table["num_mask"].values, ref["num_mask"][ok])
    kw = dict(shuffle=False)
    a = DeviceDataloader.from_observed(wave, flux, ivar, off, zq, wav, 8, DEV, names=names, snr_min=snr_min, num_mask=3,
                                       absorbers=dict(dla=rows, sky=sky), **kw)
    assert list(a.pathlist) == list(names[keep]) and a.data_size == len(keep)
    kd = torch.as_tensor(keep, device=DEV)
    r = DeviceDataloader(masked.flux[kd], masked.error[kd], zq[keep], wav, 8, DEV, paths=names[keep], **kw)
    assert torch.equal(a.flux, r.flux) and torch.equal(a.error, r.error) and np.array_equal(a.mu, r.mu)
    for x, y in zip(a.next_batch(), r.next_batch()):
        assert torch.equal(x, y)
    plain = DeviceDataloader.from_observed(wave, flux, ivar, off, zq, wav, 8, DEV, names=names, absorbers=None, **kw)
    sel = pre.select()
    sd = torch.as_tensor(sel, device=DEV)
    r0 = DeviceDataloader(pre.flux[sd], pre.error[sd], zq[sel], wav, 8, DEV, paths=names[sel], **kw)
    assert torch.equal(plain.flux, r0.flux) and torch.equal(plain.error, r0.error) and np.array_equal(plain.mu, r0.mu)
    assert list(plain.pathlist) == list(names[sel])


def test_end_to_end_mock_spectra_with_a_dla():
    """Mock spectra from a small model, a DLA's restatement profile multiplied into half of them on the host: after
    mask_absorbers with the true catalogue the kept blue pixels are the undamaged mocks within 2 float32 ulp (one multiplication,
    one division), and forest leaves the masked pixels at ivar = 0."""
    from qfa_amd import QFA, synthetic
    from qfa_amd.absorbers import mask_absorbers
    npix, nb, nh, B = 40, 16, 2, 12
    wav = 1215.67 * 10 ** (2e-3 * (np.arange(npix) - nb + 0.5))
    assert (wav < 1215.67).sum() == nb
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=4)
    T = lambda x: torch.as_tensor(x, device=DEV)
    m = QFA(nb, npix - nb, nh, torch.device(DEV), model_params=p)
    m.mu = T(mu)
    rng = np.random.default_rng(5)
    zq = rng.uniform(2.2, 3.0, B)
    zabs = ((1.0 + zq[:, None]) * wav[None, :nb] / 1215.67 - 1.0).astype(np.float32)
    error = rng.uniform(0.02, 0.05, (B, npix)).astype(np.float32)
    mock = m.sample_spectra(T(error), T(zabs), None, n_samples=1, seed=11)[:, 0].cpu().numpy()
    assert np.all(mock != R.SENTINEL) and np.all(np.isfinite(mock))
    rows = [[(float(zabs[i, 3 + i % 9]) + 1e-4, 20.3 + 0.05 * i)] if i % 2 == 0 else [] for i in range(B)]
    flux, err = mock.copy(), error.copy()
    Ts = np.ones((B, npix))
    for i in range(0, B, 2):
        Ts[i] = R.transmission(wav * (1.0 + zq[i]), [rows[i][0][0]], [rows[i][0][1]])
        flux[i] = (mock[i].astype(np.float64) * Ts[i]).astype(np.float32)
        err[i] = (error[i].astype(np.float64) * Ts[i]).astype(np.float32)
    assert not np.any(np.abs(Ts - 0.8) <= 1e-9)
    fo, eo, rec = mask_absorbers(flux, err, zq, wav, dla=rows, device=DEV, snr_window=(1230.0, 1400.0))
    gf, ge = fo.cpu().numpy(), eo.cpu().numpy()
    masked = Ts < 0.8
    assert np.array_equal(gf == R.SENTINEL, masked) and np.array_equal(ge == R.SENTINEL, masked)
    assert masked[0::2, :nb].any(axis=1).all() and not masked[1::2].any() and (~masked[0::2, :nb]).any(axis=1).all()
    assert np.array_equal(rec["n_absorber_masked"].cpu().numpy(), masked.sum(axis=1))
    blue = ~masked
    blue[:, nb:] = False
    for got, want in ((gf, mock), (ge, error)):
        d = np.abs(got[blue].astype(np.float64) - want[blue].astype(np.float64))
        assert np.all(d <= 2.0 * np.spacing(np.abs(want[blue])).astype(np.float64))
    assert gf[1::2].tobytes() == mock[1::2].tobytes()        # no absorber: untouched bits
    mask = (fo != -999.0) & (eo != -999.0)
    tr, iv, _ = m.forest(fo, eo, T(zabs), mask)
    iv = iv[:, 0].cpu().numpy()
    assert np.all(iv[masked[:, :nb]] == 0.0) and np.all(tr[:, 0].cpu().numpy()[masked[:, :nb]] == 0.0)
    assert (iv[~masked[:, :nb]] > 0.0).any()
