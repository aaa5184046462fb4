"""Observed-frame preprocessing on the GPU (qfa_preprocess_f32) against the float64 restatement tests/_preprocess_ref.py.

Bars: flux / error within 2^-23 relative (one float32 rounding: the float64 sums of the two sides may differ in their last bits,
which moves a float32 result across at most one rounding boundary); sentinels and the integer outputs exact; norm and snr within
1e-12 relative (float64 sums of at most a few thousand positive terms).  Validity and `ok` are threshold decisions: every case
first asserts on the restatement that no coverage lies within 1e-9 of min_coverage and no norm within 1e-9 of its bound."""
import functools

import numpy as np
import pytest
import torch

import _preprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = (0, 1, 2, 3, 65, 300, 520)                            # 520 = max_n_in of the mixed calls
LENS_SDSS = (4600, 520, 2100)                                # Npix = 1 913: an SDSS-length spectrum, a short and a coarse one
WHERE_SDSS = (0, 5, 0)                                       # ... the short one placed over the normalisation window
WHERE = (0, 5, 0, 1, 0, 2, 5, 3, 0, 4)                       # where a spectrum sits on the grid, per group of seven (see _case)


def _grid(npix):
    if npix == 1:
        return np.array([1275.5]), np.array([1275.0, 1276.0])
    from qfa_amd import synthetic
    g = synthetic.wavelength_grid()[0] if npix == 1913 else 1268.0 * 10 ** (1e-4 * np.arange(npix))
    return np.asarray(g, dtype=np.float64), R.edges_from_grid(g)


@functools.lru_cache(maxsize=None)
def _case(N, npix, seed):
    """N ragged spectra on every kind of input grid, position and usable pattern; returns inputs and the restatement's outputs"""
    rng = np.random.default_rng(seed)
    grid, edges = _grid(npix)
    waves, zs = [], []
    for i in range(N):
        n = LENS[(i + seed) % len(LENS)] if N > 1 else 300
        if npix == 1913:
            n = LENS_SDSS[i % 3]
        z = 2.0 + 0.13 * (i % 7)
        lo, hi = edges[0] * (1 + z), edges[-1] * (1 + z)
        step = (hi - lo) / npix
        kind, where = i % 5, WHERE[(i // 7) % len(WHERE)]
        if npix == 1913:
            where = WHERE_SDSS[i % 3]
        if kind == 0:                                        # log-linear at the output's step, fractional shift
            rel = 10 ** (1e-4 * (np.arange(n) + rng.uniform(0.1, 0.9)))
        elif kind == 1:                                      # linear
            rel = 1 + (0.83 * step / lo) * np.arange(n)
        elif kind == 2:                                      # coarser by 3
            rel = 1 + (3.0 * step / lo) * (np.arange(n) + 0.37)
        elif kind == 3:                                      # finer by 5
            rel = 1 + (0.2 * step / lo) * (np.arange(n) + 0.11)
        else:                                                # irregular
            rel = 1 + (step / lo) * np.cumsum(rng.uniform(0.3, 1.7, n))
        w = lo * rel
        span = (w[-1] - w[0]) if n > 1 else step
        if where == 1:
            w = w - (w[-1] if n else 0) + lo - 3 * step - span * 0.01      # wholly off the blue end
        elif where == 2:
            w = w - (w[0] if n else 0) + hi + 3 * step                     # wholly off the red end
        elif where == 3 and n > 1:
            w = w - w[-1] + lo + 0.77 * step                               # reaches into the first output pixel only
        elif where == 4 and n > 1:
            w = w - w[0] + hi - 0.81 * step                                # the last output pixel only
        elif where == 5:
            w = w + 0.4 * (hi - lo)
        else:
            w = w - 2.3 * step                                             # from before the blue end on
        waves.append(w)
        zs.append(z)
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    wave = np.concatenate(waves) if N else np.zeros(0)
    T = len(wave)
    flux = rng.normal(1.5, 0.3, T).astype(np.float32)
    ivar = rng.uniform(0.5, 30.0, T).astype(np.float32)
    bad = np.zeros(T, dtype=np.uint8)
    for i in range(N):
        a, b = off[i], off[i + 1]
        pat = (i // 3) % 7
        if pat == 1:
            ivar[a:b] = 0.0                                  # all unusable
        elif pat == 2:
            ivar[a:b:7] = -1.0                               # single unusable pixels
        elif pat == 3 and b - a > 40:                        # runs: several interior regions
            for s in (0.2, 0.5, 0.8):
                c = a + int(s * (b - a))
                ivar[c:c + 9] = 0.0
        elif pat == 4:
            bad[a:b:5] = 3                                   # bad without ivar = 0
        elif pat == 5:                                       # NaN and inf under unusable pixels
            ivar[a:b:6] = 0.0
            flux[a:b:6] = np.nan
            bad[a + 1:b:6] = 1
            flux[a + 1:b:6] = np.inf
        elif pat == 6:
            ivar[a:b:9] = np.inf                             # a non-finite ivar is unusable too
    zq = np.array(zs, dtype=np.float64)
    nmp = 1 if npix == 1 else 5                              # (a one-pixel grid can hold one pixel in the window)
    ref = R.preprocess_ref(wave, flux, ivar, off, zq, grid, out_edges=edges, bad=bad, norm_min_pixels=nmp)
    R.assert_away_from_thresholds(ref)
    return dict(wave=wave, flux=flux, ivar=ivar, bad=bad, off=off, z=zq, grid=grid, edges=edges, ref=ref, nmp=nmp)


def _run(c, rows=None, **kw):
    from qfa_amd.preprocess import preprocess
    if rows is None:
        args = (c["wave"], c["flux"], c["ivar"], c["off"], c["z"])
        bad = c["bad"]
    else:
        a, b = int(c["off"][rows[0]]), int(c["off"][rows[1]])
        args = (c["wave"][a:b], c["flux"][a:b], c["ivar"][a:b], c["off"][rows[0]:rows[1] + 1] - a, c["z"][rows[0]:rows[1]])
        bad = c["bad"][a:b]
    return preprocess(*args, c["grid"], bad=bad, out_edges=c["edges"], device=DEV, norm_min_pixels=c.get("nmp", 5), **kw)


def _host(p):
    g = lambda t: t.cpu().numpy()
    return dict(flux=g(p.flux), error=g(p.error), norm=g(p.norm), snr=g(p.snr), n_valid=g(p.n_valid), n_lead=g(p.n_lead),
                n_trail=g(p.n_trail), num_mask=g(p.num_mask), ok=g(p.ok).astype(np.int32))


def _compare(got, ref):
    for k in ("n_valid", "n_lead", "n_trail", "num_mask", "ok"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("flux", "error"):
        a, r = got[k], ref[k]
        assert np.array_equal(a == R.SENTINEL, r == R.SENTINEL), k
        m = r != R.SENTINEL
        assert np.all(np.abs(a[m].astype(np.float64) - r[m]) <= 2.0 ** -23 * np.abs(r[m].astype(np.float64))), k
    for k in ("norm", "snr"):
        a, r = got[k], ref[k]
        assert np.array_equal(np.isnan(a), np.isnan(r)), k
        m = np.isfinite(r)
        assert np.all(np.abs(a[m] - r[m]) <= 1e-12 * np.abs(r[m])), k


@pytest.mark.parametrize("N,npix,seed", [(1, 1, 0), (1, 40, 1), (3, 40, 2), (3, 257, 3), (70, 257, 4), (70, 40, 5), (3, 1913, 6)])
def test_kernel_matches_the_restatement(N, npix, seed):
    c = _case(N, npix, seed)
    ref = c["ref"]
    if N == 70:                                              # the mixed calls hold every kind of spectrum
        assert ref["ok"].min() == 0 and ref["ok"].max() == 1 and ref["num_mask"].max() >= 2
        assert (ref["n_valid"] == 0).any() and (ref["n_lead"] > 0).any() and (ref["n_trail"] > 0).any()
    if npix == 1913:                                         # two pixels per thread, the second pass with a partly filled last wave
        flux = ref["flux"]
        assert ref["ok"].min() == 1 and np.isfinite(ref["snr"]).all()
        assert (flux[:, 1024:] != R.SENTINEL).any(axis=1).all() and (flux[:, 1856:] != R.SENTINEL).any()
        assert (flux[1] == R.SENTINEL).any() and ref["n_lead"][1] > 0 and ref["n_trail"][1] > 1913 - 1024 - 600
    _compare(_host(_run(c)), ref)


def _window_case(n_in_window, sign=1.0):
    """the output grid itself as the input grid (z = 0): exactly `n_in_window` usable pixels inside the normalisation window"""
    grid, edges = _grid(40)
    w = grid.copy()
    flux = np.full(40, 2.0 * sign, dtype=np.float32)
    ivar = np.full(40, 4.0, dtype=np.float32)
    inwin = np.nonzero((grid >= 1270.0) & (grid < 1290.0))[0]
    ivar[inwin[n_in_window:]] = 0.0
    return dict(wave=w, flux=flux, ivar=ivar, bad=np.zeros(40, np.uint8), off=np.array([0, 40], np.int64), z=np.array([0.0]),
                grid=grid, edges=edges)


@pytest.mark.parametrize("n_in_window,sign,ok", [(4, 1.0, 0), (5, 1.0, 1), (12, -1.0, 0)])
def test_ok_decision_at_its_bounds(n_in_window, sign, ok):
    c = _window_case(n_in_window, sign)
    ref = R.preprocess_ref(c["wave"], c["flux"], c["ivar"], c["off"], c["z"], c["grid"], out_edges=c["edges"], bad=c["bad"])
    R.assert_away_from_thresholds(ref)
    assert ref["ok"][0] == ok and ref["n_norm"][0] == n_in_window
    got = _host(_run(c))
    _compare(got, ref)
    if not ok:
        assert np.all(got["flux"] == R.SENTINEL) and np.all(got["error"] == R.SENTINEL)
    else:
        assert got["norm"][0] == 2.0 and np.all(got["flux"][0][got["flux"][0] != R.SENTINEL] == 1.0)


def test_rows_do_not_depend_on_the_call():
    c = _case(70, 40, 5)
    whole = _host(_run(c))
    again = _host(_run(c))
    for k in whole:
        assert whole[k].tobytes() == again[k].tobytes(), k   # two runs, the same bits
    for i in reversed(range(70)):                            # one spectrum per call, in reversed order
        one = _host(_run(c, rows=(i, i + 1)))
        for k in whole:
            assert one[k][0].tobytes() == whole[k][i].tobytes(), (k, i)


def test_out_tensors_are_filled_in_place():
    c = _case(3, 40, 2)
    fo = torch.full((3, 40), 7.0, dtype=torch.float32, device=DEV)
    eo = torch.full((3, 40), 7.0, dtype=torch.float32, device=DEV)
    p = _run(c, out=(fo, eo))
    assert p.flux.data_ptr() == fo.data_ptr() and p.error.data_ptr() == eo.data_ptr()
    _compare(dict(_host(p), flux=fo.cpu().numpy(), error=eo.cpu().numpy()), c["ref"])


def test_device_tensors_as_input_and_host_side_refusals():
    from qfa_amd._lib import QFAHipError
    from qfa_amd.preprocess import preprocess
    c = _case(3, 40, 2)
    T = lambda x: torch.as_tensor(x, device=DEV)
    p = preprocess(T(c["wave"]), T(c["flux"]), T(c["ivar"]), T(c["off"]), T(c["z"]), c["grid"], bad=T(c["bad"]),
                   out_edges=c["edges"], device=DEV)
    _compare(_host(p), c["ref"])
    down = c["off"].copy()
    down[1], down[2] = max(down[1], down[2], 2), 1           # not monotone
    with pytest.raises(QFAHipError):
        preprocess(c["wave"], c["flux"], c["ivar"], down, c["z"], c["grid"], device=DEV)
    with pytest.raises(QFAHipError):
        preprocess(c["wave"], c["flux"], c["ivar"], c["off"], c["z"], c["grid"], out_edges=c["edges"][::-1].copy(), device=DEV)
    with pytest.raises(QFAHipError):                         # a spectrum longer than the limit
        n = 32769
        preprocess(np.arange(n) + 3000.0, np.ones(n, np.float32), np.ones(n, np.float32), [0, n], [2.0], c["grid"], device=DEV)


@functools.lru_cache(maxsize=None)
def _observed_set():
    """64 synthetic spectra, each resampled onto an observed grid of its own, the restatement's outputs and a selection that
    keeps about half of them"""
    from qfa_amd import synthetic
    npix, B = 512, 64
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
        for c0 in rng.integers(50, n - 50, int(rng.integers(0, 4))):     # up to three masked regions
            v[c0:c0 + 12] = 0.0
        waves.append(w); fl.append(f.astype(np.float32)); iv.append(v.astype(np.float32))
    zq = b["zqso"].astype(np.float64)
    names = np.array([f"obs-{s}" for s in range(B)])
    return wav, waves, fl, iv, zq, names


def _ragged(order):
    """the observed set in the given order of spectra: wave, flux, ivar, offsets, zqso, names, wav_grid"""
    wav, waves, fl, iv, zq, names = _observed_set()
    off = np.concatenate([[0], np.cumsum([len(waves[s]) for s in order])]).astype(np.int64)
    cat = lambda parts: np.concatenate([parts[s] for s in order])
    return cat(waves), cat(fl), cat(iv), off, zq[order], names[order], wav


@functools.lru_cache(maxsize=None)
def _observed_ref():
    wave, flux, ivar, off, zq, names, wav = _ragged(np.arange(64))
    ref = R.preprocess_ref(wave, flux, ivar, off, zq, wav)
    R.assert_away_from_thresholds(ref)
    snr_min = float(np.nanmedian(ref["snr"]))
    assert np.all(np.abs(ref["snr"][np.isfinite(ref["snr"])] - snr_min) > 1e-9 * snr_min)   # the cut sits on no spectrum
    keep = np.nonzero((ref["ok"] == 1) & (ref["snr"] >= snr_min) & (ref["num_mask"] <= 2))[0]
    assert 8 <= len(keep) < 64
    return ref, snr_min, keep


def test_from_observed_builds_the_loader_the_restatement_builds():
    """The selection and pathlist are the restatement's; the kernel's rows are the restatement's within the bars above; and the
    loader holds the kernel's rows, mu and first batch bit for bit -- from_observed adds nothing of its own to the numbers."""
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.preprocess import preprocess
    wave, flux, ivar, off, zq, names, wav = _ragged(np.arange(64))
    ref, snr_min, keep = _observed_ref()
    kw = dict(shuffle=False)
    a = DeviceDataloader.from_observed(wave, flux, ivar, off, zq, wav, 16, DEV, names=names, snr_min=snr_min, num_mask=2, **kw)
    assert list(a.pathlist) == list(names[keep]) and a.data_size == len(keep)
    pre = preprocess(wave, flux, ivar, off, zq, wav, device=DEV)
    _compare(_host(pre), ref)
    assert np.array_equal(pre.select(snr_min=snr_min, num_mask=2), keep)
    kd = torch.as_tensor(keep, device=DEV)
    r = DeviceDataloader(pre.flux[kd], pre.error[kd], zq[keep], wav, 16, DEV, paths=names[keep], **kw)
    assert torch.equal(a.flux, r.flux) and torch.equal(a.error, r.error) and np.array_equal(a.zqso, r.zqso)
    assert np.array_equal(a.mu, r.mu)
    for x, y in zip(a.next_batch(), r.next_batch()):
        assert torch.equal(x, y)


def _worker_from_observed(rank, world, port, q):
    import os
    import torch.distributed as dist
    from qfa_amd.dataloader import DeviceDataloader
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, snr_min, _ = _observed_ref()
    out = []
    for order in (np.arange(64), np.arange(64)[::-1]):       # the selected set leans to one half, then to the other
        wave, flux, ivar, off, zq, names, wav = _ragged(order)
        dl = DeviceDataloader.from_observed(wave, flux, ivar, off, zq, wav, 16, DEV, names=names, snr_min=snr_min, num_mask=2,
                                            shuffle=False, rank=rank, world=world)
        mine = dict(paths=list(dl.pathlist), flux=dl.flux.cpu().numpy(), error=dl.error.cpu().numpy(), z=dl.zqso, mu=dl.mu,
                    size=dl.data_size)
        both = [None, None]
        dist.all_gather_object(both, mine)
        out.append(both)
    if rank == 0:
        q.put(out)
    dist.destroy_process_group()


def test_from_observed_on_two_ranks_holds_the_single_process_rows():
    """Each rank preprocesses its half of the input; the selection of a half is not the loader's half of the selected set, so one
    rank fetches rows next to its shard in a second call -- from the half before it in one order of the spectra, from the half
    behind it in the reversed order.  The shards, concatenated, are the single-process loader's rows bit for bit."""
    from _segment_harness import two_ranks
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.distributed import shard_bounds
    _, snr_min, keep = _observed_ref()
    sel = np.zeros(64, dtype=bool)
    sel[keep] = True
    n_first = int(sel[:32].sum())
    assert n_first != len(keep) - n_first and abs(2 * n_first - len(keep)) >= 2          # the halves differ: rows do move
    got = two_ranks(_worker_from_observed, 35500)
    for order, both in zip((np.arange(64), np.arange(64)[::-1]), got):
        wave, flux, ivar, off, zq, names, wav = _ragged(order)
        one = DeviceDataloader.from_observed(wave, flux, ivar, off, zq, wav, 16, DEV, names=names, snr_min=snr_min, num_mask=2,
                                             shuffle=False)
        assert [len(b["paths"]) for b in both] == [hi - lo for lo, hi in (shard_bounds(len(keep), r, 2) for r in range(2))]
        assert both[0]["paths"] + both[1]["paths"] == list(one.pathlist) and both[0]["size"] == both[1]["size"] == len(keep)
        for k, ref in (("flux", one.flux.cpu().numpy()), ("error", one.error.cpu().numpy()), ("z", one.zqso)):
            assert np.concatenate([both[0][k], both[1][k]]).tobytes() == ref.tobytes(), k
        for b in both:                                       # mu: the all-reduced float64 sums of the two shards, in another grouping
            assert np.all(np.abs(b["mu"] - one.mu) <= 1e-12 * np.abs(one.mu))


def test_the_grid_limit_shape():
    """Npix = 16 384 with one spectrum of 32 768 input pixels: every thread owns its sixteen pixels, the bitmap is full"""
    rng = np.random.default_rng(11)
    npix, n = 16384, 32768
    grid = 1000.0 * 10 ** (2e-5 * np.arange(npix))
    edges = R.edges_from_grid(grid)
    z = 2.0
    w = np.sort(rng.uniform(edges[0] * 3 * 1.01, edges[-1] * 3 * 0.98, n))
    flux = rng.normal(1.0, 0.2, n).astype(np.float32)
    ivar = rng.uniform(1.0, 9.0, n).astype(np.float32)
    ivar[5000:5100] = 0.0
    ivar[20000:20900] = 0.0
    c = dict(wave=w, flux=flux, ivar=ivar, bad=np.zeros(n, np.uint8), off=np.array([0, n], np.int64), z=np.array([z]),
             grid=grid, edges=edges)
    ref = R.preprocess_ref(w, flux, ivar, c["off"], c["z"], grid, out_edges=edges, bad=c["bad"])
    R.assert_away_from_thresholds(ref)
    assert ref["ok"][0] == 1 and ref["num_mask"][0] >= 2 and ref["n_lead"][0] > 0 and ref["n_trail"][0] > 0
    _compare(_host(_run(c)), ref)
