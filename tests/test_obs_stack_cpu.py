"""The observed-frame residual stack without a GPU: the header's text and the binding, the port's bin rule against a brute-force loop,
`ObservedStack` algebra and `find_lines` on closed-form sums, the file round trips, the `calibrate` port at its edges, and the
C-ABI's refusals (which return before any device work)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _obs_ref as R
from conftest import REPO


def test_header_binding_and_abi():
    from qfa_amd import _lib
    text = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in ("qfa_obs_stack_doubles", "qfa_obs_stack_workspace_bytes", "qfa_obs_stack_f32", "qfa_calibrate_f32"):
        assert name in _lib.EXPORTS and name + "(" in text
    for phrase in ("#define QFA_ABI_VERSION 4", "QFA_OBS_LOG = 0, QFA_OBS_LINEAR = 1", "#define QFA_F_OBS_UNIT_W 0x2000u",
                   "typedef struct { double u0, du; int nbin; int p_lo, p_hi; unsigned mode; } qfa_obs_bins_t;",
                   "NO transmission model is applied", "<T> x calibration", "1 <= nbin <= 32768"):
        assert phrase in text, phrase
    assert _lib.ABI_VERSION == 4 and _lib.F_OBS_UNIT_W == 0x2000 and _lib.OBS_MODES == {"log": 0, "linear": 1}
    flags = [v for k, v in vars(_lib).items() if k.startswith("F_") and isinstance(v, int)]
    assert len(set(flags)) == len(flags)                                  # the new flag took a free bit
    assert C.sizeof(_lib.ObsBins) == 32


def test_sizes_and_refusals_before_any_device_work():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_obs_stack_doubles(3, 7) == 84 and h.qfa_obs_stack_doubles(1, 32768) == 4 * 32768
    assert h.qfa_obs_stack_doubles(0, 7) == 0 and h.qfa_obs_stack_doubles(1, 0) == 0 and h.qfa_obs_stack_doubles(1, 32769) == 0
    assert h.qfa_obs_stack_workspace_bytes(64, 1, 257, 8, 300) >= 16 + 4 * 300 * 8
    assert h.qfa_obs_stack_workspace_bytes(0, 1, 257, 8, 300) > 0                   # B = 0 is a shape
    for bad in ((-1, 1, 257, 8, 300), (4, 0, 257, 8, 300), (4, 1, 0, 8, 300), (4, 1, 257, 0, 300), (4, 1, 257, 33, 300),
                (4, 1, 257, 8, 0), (4, 1, 257, 8, 32769)):
        assert h.qfa_obs_stack_workspace_bytes(*bad) == 0, bad
    # the plan is a function of the shape alone
    assert h.qfa_obs_stack_workspace_bytes(130, 3, 1027, 17, 5000) == h.qfa_obs_stack_workspace_bytes(130, 3, 1027, 17, 5000)

    one = C.c_void_p(16)                                                  # never dereferenced: every call below is refused first
    bt = _lib.Batch()
    bt.delta, bt.error = 16, 16

    def call(F=one, b=bt, pix=one, bins=(3.5, 1e-4, 300, 0, 257, 0), B=4, S=1, Npix=257, Nh=8, flags=0, stack=one, ws=one, wsb=1 << 30):
        ob = None if bins is None else C.byref(_lib.ObsBins(*bins))
        return h.qfa_obs_stack_f32(F, one, None if b is None else C.byref(b), one, None, pix, one, B, S, Npix, Nh, ob, 0.0, flags,
                                   stack, ws, wsb, None)
    E_NULL, E_SIZE, E_WS, E_FLAGS = -1, -2, -3, -5
    assert call(F=None) == E_NULL and call(b=None) == E_NULL and call(pix=None) == E_NULL and call(bins=None) == E_NULL
    assert call(stack=None) == E_NULL and call(ws=None) == E_NULL
    nod = _lib.Batch()
    nod.error = 16
    assert call(b=nod) == E_NULL
    assert call(B=-1) == E_SIZE and call(S=0) == E_SIZE and call(Npix=0) == E_SIZE and call(Nh=0) == E_SIZE and call(Nh=33) == E_SIZE
    for bins in ((3.5, 0.0, 300, 0, 257, 0), (3.5, -1e-4, 300, 0, 257, 0), (3.5, np.inf, 300, 0, 257, 0), (3.5, np.nan, 300, 0, 257, 0),
                 (np.nan, 1e-4, 300, 0, 257, 0), (3.5, 1e-320, 300, 0, 257, 0), (3.5, 1e-4, 0, 0, 257, 0), (3.5, 1e-4, 32769, 0, 257, 0),
                 (3.5, 1e-4, 300, -1, 257, 0), (3.5, 1e-4, 300, 9, 8, 0), (3.5, 1e-4, 300, 0, 258, 0), (3.5, 1e-4, 300, 0, 257, 2)):
        assert call(bins=bins) == E_SIZE, bins
    short = _lib.Batch()
    short.delta, short.error, short.row_stride = 16, 16, 256
    assert call(b=short) == E_SIZE
    assert call(flags=0x200) == E_FLAGS and call(flags=0x1) == E_FLAGS        # (the forest's unit-weight bit is not this call's)
    assert call(flags=0x2000, wsb=15) == E_WS
    assert call(wsb=h.qfa_obs_stack_workspace_bytes(4, 1, 257, 8, 300) - 1) == E_WS
    # error order follows the forest call: NULL before SIZE before FLAGS before WORKSPACE
    assert call(F=None, B=-1, flags=1, wsb=0) == E_NULL and call(B=-1, flags=1, wsb=0) == E_SIZE and call(flags=1, wsb=0) == E_FLAGS

    def cal(N=4, Npix=257, ncal=5, u0=3.5, du=1e-4, mode=0, c_min=0.1, flux=one):
        return h.qfa_calibrate_f32(flux, one, one, one, N, Npix, one, ncal, u0, du, mode, c_min, one, one, one, None)
    assert cal(N=-1) == E_SIZE and cal(Npix=0) == E_SIZE and cal(ncal=1) == E_SIZE and cal(du=0.0) == E_SIZE and cal(du=np.nan) == E_SIZE
    assert cal(u0=np.inf) == E_SIZE and cal(mode=2) == E_SIZE and cal(c_min=0.0) == E_SIZE and cal(c_min=np.nan) == E_SIZE
    assert cal(N=0, flux=None) == 0 and cal(flux=None) == E_NULL


@pytest.mark.parametrize("mode", [R.LOG, R.LINEAR])
def test_bin_rule_against_a_brute_force_loop(mode):
    rng = np.random.default_rng(5)
    npix = 61
    # coordinates exactly on bin edges: every number below is a small multiple of a power of two, so that x is an integer
    if mode == R.LOG:
        pix_u, spec_u, u0, du = 3.0 + np.arange(npix) * 2.0 ** -13, np.array([0.0, 5.0, 17.0, 40.0, -3.0]) * 2.0 ** -13, 3.0 + 4 * 2.0 ** -13, 2.0 ** -13
    else:
        pix_u, spec_u, u0, du = 1000.0 + 0.5 * np.arange(npix), np.array([2.0, 3.0, 4.0, -2.0, 0.0]), 2002.0, 0.25
    for nbin in (1, 7, 300):
        x = R.coordinate(pix_u, spec_u, u0, du, mode)
        assert np.all(x == np.round(x))                                   # on the edges
        k = R.bin_index(x, nbin, spec_u)
        assert np.array_equal(k, R.bin_index_brute(pix_u, spec_u, u0, du, nbin, mode))
        on = (x >= 0) & (x < nbin)
        assert on.any() and np.array_equal(k[on], x[on].astype(np.int64))      # an edge belongs to the bin above it
        assert np.all(k[x == nbin] == -1) and np.all(k[x < 0] == -1)
    # generic coordinates, a NaN and a non-positive 1 + z, bins coarser and finer than the pixels
    wav = 10 ** (np.log10(1040.0) + 2e-4 * np.arange(npix))
    z1 = np.concatenate([rng.uniform(3.0, 4.5, 6), [np.nan, -0.5, 0.0, np.inf]])
    with np.errstate(invalid="ignore", divide="ignore"):
        pix_u, spec_u = (np.log10(wav), np.log10(z1)) if mode == R.LOG else (wav, z1)
    for du, nbin in ((16e-4, 40), (0.7e-4, 3000)) if mode == R.LOG else ((8.0, 300), (0.3, 5000)):
        u0 = np.log10(3600.0) if mode == R.LOG else 3600.0
        k = R.bin_index(R.coordinate(pix_u, spec_u, u0, du, mode), nbin, spec_u)
        assert np.array_equal(k, R.bin_index_brute(pix_u, spec_u, u0, du, nbin, mode))
        assert (k[:6] >= 0).any() and (k[:6] < 0).any() and np.all(k[6:] == -1)
        # the rule is monotone in p: the pixels of a bin are a contiguous run
        for row in k[:6]:
            inb = row[row >= 0]
            assert np.all(np.diff(inb) >= 0)


def _closed_form_stack(nbin=60, n0=200.0, S=1):
    """flat bins: n0 pixels of weight 4 whose r are 1 +- 0.1 in equal halves (mean 1, weighted scatter 0.01 w); bins 20..22 with
    the scatter inflated 9 times at the same mean; bins 40..41 with the mean 10 % low; bin 50 under-populated with a wild mean"""
    from qfa_amd.calibration import ObservedStack
    w, n = np.full(nbin, 4.0), np.full(nbin, n0)
    m, s2 = np.ones(nbin), np.full(nbin, 0.01)
    s2[20:23] = 0.09
    m[40:42] = 0.9
    n[50], m[50], s2[50] = 3.0, 2.0, 1.0
    buf = np.stack([n * w, n * w * m, n * w * (s2 + m * m), n])
    return ObservedStack(torch.tensor(np.repeat(buf[None], S, 0)), np.log10(3600.0), 1e-3, nbin, "log"), m, s2, w


def test_observed_stack_algebra():
    from qfa_amd._lib import QFAHipError
    from qfa_amd.calibration import ObservedStack, obs_grid
    st, m, s2, w = _closed_form_stack(S=2)
    assert st.S == 2 and st.bins == (np.log10(3600.0), 1e-3, 60, "log")
    assert np.allclose(st.mean()[0].numpy(), m, rtol=1e-14) and np.allclose(st.var()[1].numpy(), s2, rtol=1e-10)
    assert np.allclose(st.err()[0].numpy(), np.sqrt(s2 / (st.n[0].numpy() - 1)), rtol=1e-10)
    assert np.allclose(st.wave_edges, 10 ** (np.log10(3600.0) + 1e-3 * np.arange(61))) and len(st.wave_centers) == 60
    assert st.wave_edges[0] < st.wave_centers[0] < st.wave_edges[1]
    assert np.allclose(st.chi2(1.0), w * (s2 + (m - 1.0) ** 2), rtol=1e-10)
    assert np.allclose(st.chi2(m), w * s2, rtol=1e-10)
    assert np.allclose(st.calibration(0), m, rtol=1e-14)
    c3 = st.calibration(3)
    assert np.allclose(c3[:10], 1.0, rtol=1e-14) and 0.9 < c3[40] < 1.0
    assert float(st.std_over_draws().max()) == 0.0
    two = st.clone().add_(st)
    assert torch.equal(two.buf, 2 * st.buf) and torch.equal(two.mean(), st.mean())
    assert torch.equal(st.draws(1, 2).buf, st.buf[1:2])
    a = st.arrays()
    assert a["sums"].shape == (2, 4, 60) and a["mode"] == "log" and a["mean"].shape == (2, 60)
    lin = ObservedStack.zeros(1, 3600.0, 0.8, 7781, "linear")
    assert np.allclose(lin.wave_edges[[0, -1]], [3600.0, 3600.0 + 0.8 * 7781]) and np.isnan(lin.calibration(2)).all()
    assert obs_grid(3600.0, 4607, dloglam=1e-4) == (float(np.log10(3600.0)), 1e-4, 4607, "log")
    assert obs_grid(3600.0, 7781, dlam=0.8) == (3600.0, 0.8, 7781, "linear")
    for bad in (dict(lam_min=3600.0, nbin=7), dict(lam_min=3600.0, nbin=7, dloglam=1e-4, dlam=0.8), dict(lam_min=0.0, nbin=7, dlam=1.0),
                dict(lam_min=3600.0, nbin=0, dlam=1.0), dict(lam_min=3600.0, nbin=32769, dlam=1.0), dict(lam_min=3600.0, nbin=7, dlam=0.0)):
        with pytest.raises(QFAHipError):
            obs_grid(**bad)
    with pytest.raises(QFAHipError):
        st.add_(lin)
    with pytest.raises(QFAHipError):
        ObservedStack(torch.zeros((1, 4, 8), dtype=torch.float32), 3.5, 1e-4, 8)
    with pytest.raises(QFAHipError):
        ObservedStack.zeros(1, 3.5, 1e-4, 8).std_over_draws()


def test_find_lines_on_closed_form_sums():
    st, m, s2, w = _closed_form_stack()
    kw = dict(min_count=50, chi2_ratio=3.0, max_dev=0.05, half_width=5)
    # the reference alone: the flat bins sit below both thresholds, the injected ones above one of them
    cal = st.calibration(5)
    chi = st.chi2(cal)
    mean = st.mean()[0].numpy()
    flat = np.ones(60, bool)
    flat[[20, 21, 22, 40, 41, 50]] = False
    med = np.median(chi[st.n[0].numpy() >= 50])
    assert np.all(chi[flat] <= 3.0 * med) and np.all(np.abs(mean[flat] / cal[flat] - 1.0) <= 0.05)
    assert np.all(chi[20:23] > 3.0 * med) and np.all(np.abs(mean[40:42] / cal[40:42] - 1.0) > 0.05)
    assert abs(mean[50] / cal[50] - 1.0) > 0.05                           # the under-populated bin would be flagged on its mean
    e = st.wave_edges
    got = st.find_lines(grow=0, **kw)
    assert got.dtype == np.float64 and np.array_equal(got, np.array([[e[20], e[23]], [e[40], e[42]]]))
    assert np.array_equal(st.find_lines(grow=1, **kw), np.array([[e[19], e[24]], [e[39], e[43]]]))
    assert np.array_equal(st.find_lines(grow=9, **kw), np.array([[e[11], e[51]]]))          # grown runs merge
    assert np.array_equal(st.find_lines(grow=0, min_count=2, chi2_ratio=3.0, max_dev=0.05, half_width=5)[-1], [e[50], e[51]])
    assert st.find_lines(grow=0, min_count=50, chi2_ratio=1e9, max_dev=0.5, half_width=5).shape == (0, 2)
    from qfa_amd.calibration import ObservedStack
    assert ObservedStack.zeros(1, 3.5, 1e-4, 9).find_lines().shape == (0, 2)


def test_file_round_trips(tmp_path):
    from qfa_amd import io
    st, *_ = _closed_form_stack()
    iv = st.find_lines(grow=1, min_count=50, chi2_ratio=3.0, max_dev=0.05, half_width=5)
    back = io.read_intervals(io.write_intervals(str(tmp_path / "sky_lines.txt"), iv, header="found by find_lines"))
    assert back.dtype == np.float64 and np.array_equal(back, iv) and len(iv) == 2
    assert io.read_intervals(io.write_intervals(str(tmp_path / "none.txt"), np.zeros((0, 2)))).shape == (0, 2)
    from qfa_amd.absorbers import _intervals
    assert np.array_equal(_intervals(back, "sky"), iv)                    # what mask_absorbers(sky=...) takes
    for table in (st, st.table(5), {"u0": 3600.0, "du": 0.8, "mode": "linear", "cal": np.array([1.0, np.nan, 0.5])}):
        t = io.read_calibration(io.write_calibration(str(tmp_path / "calibration.npz"), table, half_width=5))
        want = table.table(5) if hasattr(table, "table") else table
        assert t["u0"] == want["u0"] and t["du"] == want["du"] and t["mode"] == want["mode"]
        assert t["cal"].dtype == np.float64 and np.array_equal(t["cal"], want["cal"], equal_nan=True)
    np.savez(tmp_path / "bad.npz", u0=1.0)
    with pytest.raises(ValueError):
        io.read_calibration(str(tmp_path / "bad.npz"))


def test_calibrate_port_edges():
    u0, du = 3600.0, 2.0
    pix_u = np.array([1800.0, 1800.5, 1801.0, 1802.0, 1803.25, 1804.0, 1804.5, 1805.0, 1806.0])
    spec_u = np.array([2.0, 2.0])
    flux = np.tile(np.arange(1.0, 10.0, dtype=np.float32), (2, 1))
    err = np.full_like(flux, 0.5)
    flux[1, 3], err[1, 4] = -999.0, -999.0
    cal = np.array([1.0, 2.0, 4.0, np.nan, 0.05, 1.0])                    # centres at 3601, 3603, ..., 3611
    fo, eo, nu, j, done, qf, _ = R.calibrate(flux, err, pix_u, spec_u, cal, u0, du, R.LINEAR, 0.1)
    # observed 3600 (below the first centre), 3601 (the first centre: x = 0), 3602, 3604, 3606.5 (next to the NaN), 3608 (between NaN and
    # sub-c_min), 3609 (the sub-c_min entry), 3610 (0.525), 3612 (above the last centre)
    assert list(j[0]) == [-1, 0, 0, 1, 2, 3, 4, 4, -1]
    assert list(done[0]) == [False, True, True, True, False, False, False, True, False]
    assert fo[0, 1] == np.float32(2.0 / 1.0) and fo[0, 2] == np.float32(3.0 / 1.5) and fo[0, 3] == np.float32(4.0 / 3.0)
    assert fo[0, 7] == np.float32(8.0 / 0.525) and eo[0, 7] == np.float32(0.5 / 0.525)
    assert fo[0, 0] == 1.0 and fo[0, 8] == 9.0 and nu[0] == 5
    assert fo[1, 3] == -999.0 and eo[1, 3] == 0.5 and fo[1, 4] == 5.0 and eo[1, 4] == -999.0 and nu[1] == 4
    # ncal = 2: j is always 0, both ends of the table are calibrated with the end values
    fo, eo, nu, j, done, *_ = R.calibrate(flux[:1, :4], err[:1, :4], np.array([1800.5, 1801.0, 1801.5, 1801.75]), spec_u[:1], np.array([2.0, 4.0]),
                                          u0, du, R.LINEAR, 0.1)
    assert list(j[0]) == [0, 0, 0, -1] and list(done[0]) == [True, True, True, False]
    assert list(fo[0]) == [np.float32(1.0 / 2.0), np.float32(2.0 / 3.0), np.float32(3.0 / 4.0), 4.0] and nu[0] == 1
    # a NaN spec_u calibrates nothing and counts every valid pixel
    _, _, nu, _, done, *_ = R.calibrate(flux, err, pix_u, np.array([np.nan, 2.0]), cal, u0, du, R.LINEAR, 0.1)
    assert not done[0].any() and nu[0] == 9


def test_kernels_use_no_scratch_and_never_fuse_the_coordinate():
    import re
    path = os.path.join(REPO, "qfa_amd", "csrc", "build", "qfa_obs-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "build first"
    text = open(path).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) >= 8 and all(int(x) == 0 for x in sizes)            # six forms of k_obs_stack (N_h = 32 among them), the reducer, k_calibrate
    names = re.findall(r"^(_ZN7qfa_obs\w+):", text, re.M)
    assert len([n for n in names if "k_obs_stack" in n]) == 6 and any("k_calibrate" in n for n in names)
    for name in names:
        if "k_obs_stack" in name or "k_obs_reduce" in name:
            code = text.split("\n" + name + ":", 1)[1].split("s_endpgm", 1)[0]
            assert "v_mul_f64" in code or "k_obs_reduce" in name
            assert "v_fma_f64" not in code and "v_fmac_f64" not in code, name
