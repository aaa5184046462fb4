"""Observed-frame preprocessing without a GPU: the float64 restatement of the rule (tests/_preprocess_ref.py) against hand-worked
cases, flux conservation and brute-force sub-sampling; run counting; `Preprocessed` on CPU tensors; the C-ABI's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _preprocess_ref as R


def _linear_edges(n, lo=1000.0, step=1.0):
    return lo + step * np.arange(n + 1)


def _centres(edges):
    return 0.5 * (edges[:-1] + edges[1:])


def test_identical_grid_reproduces_flux_and_ivar():
    edges = _linear_edges(12)
    w = _centres(edges)
    rng = np.random.default_rng(1)
    f, iv = rng.normal(1, 0.1, 12).astype(np.float32), rng.uniform(1, 4, 12).astype(np.float32)
    fk, ik, cov, W = R.rebin_one(w, f, iv, None, 0.0, edges)
    assert np.array_equal(fk, f.astype(np.float64)) and np.array_equal(ik, iv.astype(np.float64))
    assert np.array_equal(cov, np.ones(12))


def test_half_pixel_shift_is_the_even_mean():
    edges = _linear_edges(8)
    w = _centres(edges) + 0.5                              # input pixel j covers [j + 0.5, j + 1.5): halves of outputs j, j + 1
    f = np.arange(1, 9, dtype=np.float32)
    u = np.full(8, 2.0, dtype=np.float32)
    fk, ik, cov, W = R.rebin_one(w, f, u, None, 0.0, edges)
    assert np.array_equal(fk[1:], 0.5 * (f[:-1] + f[1:]).astype(np.float64))
    assert np.array_equal(ik[1:], np.full(7, 4.0))          # (u_a + u_b)^2 / (u_a + u_b) = 2 u for equal u
    u2 = np.array([1, 3, 1, 3, 1, 3, 1, 3], dtype=np.float32)
    fk, ik, _, _ = R.rebin_one(w, f, u2, None, 0.0, edges)
    ua, ub = u2[:-1].astype(np.float64), u2[1:].astype(np.float64)
    assert np.allclose(ik[1:], (ua + ub) ** 2 / (ua + ub), rtol=1e-15)
    assert np.allclose(fk[1:], (ua * f[:-1] + ub * f[1:]) / (ua + ub), rtol=1e-15)
    assert cov[0] == 0.5 and np.all(cov[1:] == 1.0)


def test_one_coarse_pixel_over_three_outputs_and_five_fine_per_output():
    edges = _linear_edges(3)
    w = np.array([998.5, 1001.5, 1004.5])                  # 3-wide pixels: the middle one is exactly the three outputs
    fk, ik, cov, _ = R.rebin_one(w, np.float32([7, 2, 9]), np.float32([1, 5, 1]), None, 0.0, edges)
    assert np.array_equal(fk, [2.0, 2.0, 2.0]) and np.array_equal(cov, [1.0, 1.0, 1.0])
    assert np.allclose(ik, 5.0, rtol=1e-15)                 # W^2 / sum c^2 u = (5)^2 / (1 * 5)
    edges = _linear_edges(4, 1000.0, 1.0)
    w = 1000.0 + 0.2 * (np.arange(20) + 0.5)               # five inputs per output, 0.2 wide
    f = np.arange(20, dtype=np.float32)
    u = np.ones(20, dtype=np.float32)
    fk, ik, cov, _ = R.rebin_one(w, f, u, None, 0.0, edges)
    assert np.allclose(fk, f.reshape(4, 5).mean(axis=1), rtol=1e-12)
    assert np.allclose(ik, 5.0, rtol=1e-12)                 # (5 x 0.2)^2 / (5 x 0.04)
    assert np.allclose(cov, 1.0, rtol=1e-12)


def test_constant_flux_is_conserved_under_any_ivar_pattern():
    rng = np.random.default_rng(7)
    grid = 10 ** np.arange(np.log10(1100.0), np.log10(1200.0), 1e-3)
    edges = R.edges_from_grid(grid)
    n = 300
    w = np.sort(rng.uniform(2900.0, 4100.0, n))
    iv = rng.uniform(0.1, 10.0, n).astype(np.float32)
    iv[rng.random(n) < 0.2] = 0.0
    bad = (rng.random(n) < 0.1).astype(np.uint8)
    f = np.full(n, 3.25, dtype=np.float32)
    f[(iv == 0) | (bad != 0)] = np.nan                      # unusable pixels hold NaN: they must not poison a sum
    fk, ik, cov, W = R.rebin_one(w, f, iv, bad, 1.9, edges)
    valid = (cov >= 0.5) & (W > 0)
    assert valid.sum() > 10
    assert np.allclose(fk[valid], 3.25, rtol=1e-14)


def test_against_sub_sampling_each_output_pixel():
    """Brute force: S = 4 096 sample points per output pixel, each given to the input pixel that contains it, i.e. c'_j = (points in
    j) / S.  A sample cell of length 1 / S goes wholly to one side of an input edge that cuts it, so every edge inside the pixel
    moves a length d <= 1 / (2 S) (in units of the pixel) between its two neighbours a and b.  With m such edges, weights in
    [u_min, u_max] and fluxes in [f_min, f_max], to first order in d:
      flux_k   the weighted mean moves by d |u_b (f_b - mean) - u_a (f_a - mean)| / W <= d u_max (f_max - f_min) / u_min per edge
               (W >= u_min at full coverage):  bar_f = m (u_max / u_min) (f_max - f_min) / (2 S).  That is the resolution of the
               sub-sampling, 1 / S of the largest weight ratio, times m (f_max - f_min) / 2 -- at most 1.5 of it here (m <= 3,
               f_max - f_min = 1), and the test also holds every pixel to that plain figure where m <= 2;
      ivar_k   = W^2 / Q, Q = sum c^2 u.  W moves by d |u_b - u_a| <= d (u_max - u_min) per edge;  Q by 2 d |c_b u_b - c_a u_a|
               <= 2 d u_max per edge, and Q >= u_min / (m + 1) (sum c = 1 over m + 1 pixels).  Relative:
               bar_i = m [2 (u_max - u_min) / u_min + 2 (m + 1) u_max / u_min] / (2 S);
      second order: the terms left out are d times these, so both bars carry the factor (1 + m / S); 1e-13 stands for the float64
      roundings of either side."""
    rng = np.random.default_rng(3)
    edges = _linear_edges(20, 1000.0, 1.0)
    n = 37
    w = np.sort(rng.uniform(998.0, 1022.0, n))
    u = rng.uniform(1.0, 4.0, n).astype(np.float32)
    f = rng.uniform(0.5, 1.5, n).astype(np.float32)
    u_min, u_max, f_span = float(u.min()), float(u.max()), float(f.max() - f.min())
    fk, ik, cov, W = R.rebin_one(w, f, u, None, 0.0, edges)
    e = R.input_edges(w)
    S = 4096
    full = 0
    for k in range(20):
        x = edges[k] + (np.arange(S) + 0.5) / S
        j = np.searchsorted(e, x, side="right") - 1
        inside = (j >= 0) & (j < n)
        if inside.sum() < S:                               # partly covered pixels: the coverage alone, one cell per end edge
            assert abs(cov[k] - inside.mean()) <= 1.0 / S
            continue
        full += 1
        cs = np.bincount(j, minlength=n) / S               # c'_j
        uu, ff = u.astype(np.float64), f.astype(np.float64)
        m = int((cs > 0).sum()) - 1
        assert 0 <= m <= 3                                 # (m = 0: one input pixel holds the whole output pixel; float64 rounding alone)
        second = 1.0 + m / S
        bar_f = m * (u_max / u_min) * f_span / (2 * S) * second + 1e-13
        err_f = abs(fk[k] - (cs * uu * ff).sum() / (cs * uu).sum())
        assert err_f <= bar_f, (k, err_f, bar_f)
        if m <= 2:
            assert err_f <= (u_max / u_min) / S, (k, err_f)
        bar_i = m * (2 * (u_max - u_min) / u_min + 2 * (m + 1) * u_max / u_min) / (2 * S) * second + 1e-13
        iv_s = (cs * uu).sum() ** 2 / (cs * cs * uu).sum()
        assert abs(ik[k] - iv_s) <= bar_i * iv_s, (k, abs(ik[k] - iv_s) / iv_s, bar_i)
        assert abs(cov[k] - 1.0) <= 1e-12
    assert full >= 15


@pytest.mark.parametrize("valid,expect", [
    ("1111111", (7, 0, 0, 0)), ("0000000", (0, 7, 7, 0)), ("0001111", (4, 3, 0, 0)), ("1111000", (4, 0, 3, 0)),
    ("1100110011", (6, 0, 0, 2)), ("1110111", (6, 0, 0, 1)), ("0101010", (3, 1, 1, 2)), ("1", (1, 0, 0, 0)), ("0", (0, 1, 1, 0))])
def test_run_counting(valid, expect):
    assert R.run_counts([c == "1" for c in valid]) == expect


def _cpu_preprocessed(n=9, npix=30, seed=2):
    from qfa_amd.preprocess import Preprocessed
    rng = np.random.default_rng(seed)
    grid = 10 ** np.arange(np.log10(1250.0), np.log10(1250.0) + npix * 1e-4 - 1e-9, 1e-4)[:npix]
    flux = rng.normal(1, 0.1, (n, npix)).astype(np.float32)
    err = rng.uniform(0.05, 0.2, (n, npix)).astype(np.float32)
    flux[0, 3:6] = err[0, 3:6] = -999.0
    ok = np.ones(n, dtype=bool)
    ok[[2, 5]] = False
    flux[~ok] = err[~ok] = -999.0
    snr = rng.uniform(1, 12, n)
    snr[7] = np.nan
    T = torch.as_tensor
    pre = Preprocessed(T(flux), T(err), T(rng.uniform(2.0, 3.5, n)), T(rng.uniform(1, 3, n)), T(snr),
                       T(rng.integers(0, 4, n).astype(np.int32)), T(np.full(n, npix, np.int32)), T(np.zeros(n, np.int32)),
                       T(np.zeros(n, np.int32)), T(ok), grid)
    return pre, flux, err, ok


def test_preprocessed_select_is_the_reference_criteria():
    pre, _, _, ok = _cpu_preprocessed()
    snr, z, nm = pre.snr.numpy(), pre.zqso.numpy(), pre.num_mask.numpy()
    for crit in (dict(), dict(snr_min=3.0, snr_max=10.0), dict(z_min=2.3, z_max=3.2, num_mask=1), dict(num_mask=0)):
        c = dict(snr_min=-np.inf, snr_max=np.inf, z_min=-np.inf, z_max=np.inf, num_mask=np.inf)
        c.update(crit)
        with np.errstate(invalid="ignore"):
            want = ok & (snr >= c["snr_min"]) & (snr <= c["snr_max"]) & (z >= c["z_min"]) & (z <= c["z_max"]) & (nm <= c["num_mask"])
        got = pre.select(**crit)
        assert np.array_equal(got, np.nonzero(want)[0])
        assert not set(got) & {2, 5, 7}                      # not ok, not ok, NaN snr


def test_write_npz_round_trips_through_the_catalogue_loader(tmp_path):
    from qfa_amd import io
    pre, flux, err, ok = _cpu_preprocessed()
    names = [f"spec-{i:03d}" for i in range(len(pre))]
    cat = pre.write_npz(str(tmp_path), names)
    written = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert written == [f"spec-{i:03d}.npz" for i in range(len(pre)) if ok[i]]
    table = pre.catalog(names)
    assert list(table.columns) == ["file", "snr", "z", "num_mask"] and len(table) == int(ok.sum())
    finite = np.nonzero(ok & np.isfinite(pre.snr.numpy()))[0]
    np.random.seed(0)
    f2, e2, z2, paths = io.load_from_catalog(cat, str(tmp_path), len(finite), -np.inf, np.inf, -np.inf, np.inf, np.inf)
    assert sorted(os.path.basename(p) for p in paths) == [f"spec-{i:03d}.npz" for i in finite]   # (drawn without replacement)
    for f, e, z, p in zip(f2, e2, z2, paths):
        i = int(os.path.basename(p)[5:8])
        assert f.dtype == np.float32 and f.tobytes() == flux[i].tobytes() and e.tobytes() == err[i].tobytes()
        assert z == pre.zqso.numpy()[i]


def test_read_observed_npz(tmp_path):
    from qfa_amd import io
    w0 = np.linspace(3600, 3700, 11)
    np.savez(tmp_path / "a.npz", wave=w0, flux=np.ones(11, np.float32), ivar=np.full(11, 2, np.float32), z=2.5)
    np.savez(tmp_path / "b.npz", loglam=np.log10(w0[:4]), flux=np.zeros(4, np.float32), ivar=np.ones(4, np.float32),
             and_mask=np.array([0, 4, 0, 1]), z=3.0)
    wave, flux, ivar, bad, off, z = io.read_observed_npz([str(tmp_path / "a.npz"), str(tmp_path / "b.npz")], nprocs=2)
    assert off.tolist() == [0, 11, 15] and off.dtype == np.int64 and z.tolist() == [2.5, 3.0]
    assert wave.dtype == np.float64 and flux.dtype == np.float32 and ivar.dtype == np.float32 and bad.dtype == np.uint8
    assert np.array_equal(wave[:11], w0) and np.allclose(wave[11:], w0[:4], rtol=1e-15) and bad.tolist() == [0] * 11 + [0, 1, 0, 1]


def test_cpu_device_is_refused_and_the_lazy_exports_exist():
    import qfa_amd
    from qfa_amd._lib import QFAHipError
    from qfa_amd.dataloader import DeviceDataloader
    assert callable(qfa_amd.preprocess) and qfa_amd.Preprocessed is qfa_amd.preprocess.Preprocessed
    assert hasattr(DeviceDataloader, "from_observed")
    w = np.linspace(3000, 4000, 50)
    with pytest.raises(QFAHipError):
        qfa_amd.preprocess(w, np.ones(50, np.float32), np.ones(50, np.float32), [0, 50], [2.0], np.linspace(1000, 1100, 20),
                           device="cpu")


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    from qfa_amd import _lib
    h = _lib.lib()
    assert "qfa_preprocess_f32" in _lib.EXPORTS and "qfa_preprocess_workspace_bytes" in _lib.EXPORTS
    wsb = h.qfa_preprocess_workspace_bytes
    assert wsb(1, 16384, 32768) > 0 and wsb(0, 1, 0) > 0
    assert wsb(1, 16385, 10) == 0 and wsb(1, 0, 10) == 0 and wsb(1, 10, 32769) == 0 and wsb(1, 10, -1) == 0 and wsb(-1, 10, 10) == 0

    def call(N=1, max_n_in=10, npix=10, q="good", **over):
        p = dict(min_coverage=0.5, norm_lo=1270.0, norm_hi=1290.0, snr_lo=1270.0, snr_hi=1600.0, norm_min_pixels=5)
        p.update(over)
        qq = None if q is None else C.byref(_lib.PreprocessParams(*[p[k] for k in ("min_coverage", "norm_lo", "norm_hi", "snr_lo",
                                                                                  "snr_hi", "norm_min_pixels")]))
        return h.qfa_preprocess_f32(None, None, None, None, None, None, N, max_n_in, None, None, npix, qq, None, None, None, None,
                                    None, 0, None)
    E_NULL, E_SIZE = -1, -2
    assert call() == E_NULL and call(q=None) == E_NULL
    assert call(N=-1) == E_SIZE
    assert call(npix=0) == E_SIZE and call(npix=16385) == E_SIZE
    assert call(max_n_in=-1) == E_SIZE and call(max_n_in=32769) == E_SIZE
    for mc in (0.0, -0.1, 1.0000001, float("nan")):
        assert call(min_coverage=mc) == E_SIZE
    assert call(norm_lo=1290.0) == E_SIZE and call(norm_hi=float("inf")) == E_SIZE and call(norm_lo=float("nan")) == E_SIZE
    assert call(snr_lo=1600.0) == E_SIZE and call(snr_hi=float("nan")) == E_SIZE
    assert call(norm_min_pixels=0) == E_SIZE
    assert call(N=0) == 0                                    # a no-op, whatever the pointers
    assert call(npix=16384, max_n_in=32768) == E_NULL        # the limits themselves pass the size checks


def test_kernel_uses_no_scratch():
    from conftest import REPO
    path = os.path.join(REPO, "qfa_amd", "csrc", "build", "qfa_preprocess-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "build first"
    txt = open(path).read()
    import re
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", txt)
    assert len(sizes) == 2 and all(int(s) == 0 for s in sizes)
