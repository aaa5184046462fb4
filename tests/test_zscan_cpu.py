"""The redshift finder without a GPU: the C-ABI's declarations, the restatement against the oracle, the condition under which the GPU
test may compare arg-maxes with no spectrum left out (on every committed seed the restatement finds the injected shift and its
top-two gap is more than 100 x the bar), the host arithmetic of ``RedshiftScan``, the refusals and the chunk size of the batch walk."""
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import _zscan_ref as R
from conftest import REPO

CALLS = ("qfa_zscan_workspace_bytes", "qfa_redshift_scan_f32")


def test_header_and_exports():
    from qfa_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "qfa_hip.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS and hasattr(h, name), name


@pytest.mark.parametrize("tau", ["becker", "fg", "kamble", "mock"])
def test_zero_shift_is_the_oracles_nll(tau):
    """m = 0: the window is the whole spectrum and the restatement is oracle.forward's NLL of that spectrum"""
    from oracle import qfa_oracle as O
    npix, nb, nh = 70, 30, 5
    params, mu, wav, _ = R.model(npix, nb, nh, seed=3)
    d = R.draw(params, mu, wav, 3, 4, 0, tau_which=tau)
    _, nll0, nll = R.scan(params, mu, d["flux"], d["error"], d["mask"], d["zqso"], wav, 0, tau)
    assert nll.shape == (3, 1)
    z = R.z_pixels(d["zqso"], wav).astype(np.float64)           # (the float32 z the device forms, promoted as the oracle promotes it)
    for s in range(3):
        A = np.ones(npix)
        A[:nb] = np.exp(-O.tau_eff(z[s, :nb], tau))
        delta = (d["flux"][s].astype(np.float64) - A * mu)[None]
        loss, _ = O.forward(params, delta, d["error"][s][None], z[s, :nb][None], d["mask"][s][None], tau)
        assert abs(nll0[s] - loss) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("i", range(len(R.RECOVERY)))
def test_restatement_recovers_the_injected_shifts(i):
    c = R.recovery_case(i)
    best = R.argbest(c["llr"])
    top = np.sort(c["nll"], axis=1)
    gap = top[:, 1] - top[:, 0]
    bar = R.BAR * np.abs(c["nll"]).max(axis=1)
    print("set", i, "recovered", int(np.sum(best == c["shift"])), "of", len(best), "; min gap / bar", float(np.min(gap / bar)),
          "; min relative gap", float(np.min(gap / np.abs(c["nll"]).max(axis=1))))
    assert np.array_equal(best, c["shift"])
    assert np.array_equal(np.argmin(c["nll"], axis=1) - c["m"], c["shift"])
    assert np.all(gap > 100.0 * bar)
    assert len(np.unique(c["shift"])) > c["m"]                      # (the shifts cover the scan)


def test_all_masked_and_masked_values():
    params, mu, wav, _ = R.model(70, 30, 3, seed=5)
    d = R.draw(params, mu, wav, 2, 6, [1, -2])
    mask = d["mask"].copy()
    mask[1] = False
    flux = d["flux"].copy()
    flux[1] = np.nan
    flux[0][~mask[0]] = np.inf
    llr, nll0, _ = R.scan(params, mu, flux, d["error"], mask, d["zqso"], wav, 4)
    assert np.all(llr[1] == 0.0) and nll0[1] == 0.0 and R.argbest(llr)[1] == 0
    assert np.all(np.isfinite(llr[0])) and R.argbest(llr)[0] == 1 and np.all(llr[:, 4] == 0.0)


def test_argbest_order():
    llr = np.array([[1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 2.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [3.0, 3.0, 0.0, 0.0, 0.0]])
    assert R.argbest(llr).tolist() == [-2, -1, 0, -1]


def _scan(best_s, offset, sigma, zq, d, m=3):
    from qfa_amd.redshift import RedshiftScan
    B = len(best_s)
    llr = np.zeros((B, 2 * m + 1), dtype=np.float32)
    return RedshiftScan(llr, np.zeros(B, dtype=np.float32), np.asarray(best_s, dtype=np.int32), np.zeros(B, dtype=np.float32),
                        np.asarray(offset, dtype=np.float64), np.asarray(sigma, dtype=np.float64), zq, d)


def test_host_arithmetic_against_hand_values(tmp_path):
    from qfa_amd import io
    from qfa_amd.redshift import parabola
    d = 1e-4
    s = _scan([2, -3, 0, 3], [0.25, np.nan, -0.5, np.nan], [0.5, np.nan, 2.0, np.nan], [2.0, 2.5, 3.0, 3.5], d)
    assert np.array_equal(s.shift(), [2.25, -3.0, -0.5, 3.0])
    assert np.allclose(s.z(), [3.0 * 10 ** (-2.25e-4) - 1, 3.5 * 10 ** (3e-4) - 1, 4.0 * 10 ** (0.5e-4) - 1, 4.5 * 10 ** (-3e-4) - 1], rtol=0, atol=1e-15)
    kms = d * np.log(10.0) * 299792.458                            # one pixel of 1e-4 dex: 69.03 km/s
    assert abs(kms - 69.0298) < 1e-3
    assert np.allclose(s.dv_kms(), [-2.25 * kms, 3.0 * kms, 0.5 * kms, -3.0 * kms], rtol=1e-15)
    assert np.allclose(s.sigma_kms()[[0, 2]], [0.5 * kms, 2.0 * kms], rtol=1e-15) and np.all(np.isnan(s.sigma_kms()[[1, 3]]))
    assert np.allclose(s.sigma_z()[[0, 2]], (1.0 + s.z()[[0, 2]]) * np.log(10.0) * d * np.array([0.5, 2.0]), rtol=1e-15)
    assert s.at_edge().tolist() == [False, True, False, True]
    assert np.allclose(s.log_evidence().numpy(), 0.0, atol=1e-15)  # llr = 0 everywhere: logsumexp - log n_s = 0
    # the parabola y = -(x - 0.25)^2 / (2 0.5^2) at x = -1, 0, 1: vertex 0.25, sigma 0.5; a flat and a convex triple: NaN
    y = lambda x: -(x - 0.25) ** 2 / (2 * 0.25)
    off, sig = parabola([y(-1.0), 1.0, 0.0], [y(0.0), 1.0, 0.0], [y(1.0), 1.0, 1.0])
    assert abs(off[0] - 0.25) < 1e-15 and abs(sig[0] - 0.5) < 1e-15 and np.all(np.isnan(off[1:])) and np.all(np.isnan(sig[1:]))
    ro, rs = R.parabola(np.array([[y(-1.0), y(0.0), y(1.0)]]), [0])
    assert ro[0] == off[0] and rs[0] == sig[0]
    t = s.to_table(["a.npz", "b.npz", "c.npz", "d.npz"])
    p = io.write_redshift_csv(str(tmp_path / "z.csv"), t)
    back = io.read_redshift_csv(p)
    assert list(back) == list(io.REDSHIFT_COLUMNS)
    for k in io.REDSHIFT_COLUMNS:
        if k == "file":
            assert back[k].tolist() == t[k].tolist()
        else:
            assert back[k].dtype == t[k].dtype and np.array_equal(back[k], t[k], equal_nan=True), k
    a = s.arrays()
    assert a["llr"].shape == (4, 7) and np.array_equal(a["z"], s.z()) and float(a["dloglam"]) == d


def _fake_model(npix=40, nb=15, nh=2, mu=True, tau_callable=None):
    """a QFA that holds what redshift_scan reads before any device work (the class needs a GPU to construct)"""
    from qfa_amd.model import QFA
    m = object.__new__(QFA)
    m.Npix, m.Nb, m.Nh = npix, nb, nh
    m.mu = torch.zeros(npix) if mu else None
    m._tau_callable = tau_callable
    return m


def test_refusals():
    from qfa_amd._lib import QFAHipError
    from qfa_amd.redshift import check_grid
    wav, _ = R.grid(40)
    x = torch.zeros((3, 40))
    ok = dict(zqso=np.array([2.0, 2.5, 3.0]), wav_grid=wav, max_shift=4)
    call = lambda m, **kw: m.redshift_scan(x, x, x > 0, **{**ok, **kw})
    with pytest.raises(QFAHipError, match="uniform in log"):
        call(_fake_model(), wav_grid=np.linspace(1030.0, 1600.0, 40))
    with pytest.raises(QFAHipError, match="uniform in log"):
        call(_fake_model(), wav_grid=wav * (1.0 + 3e-6 * (np.arange(40) % 2)))
    with pytest.raises(QFAHipError, match="the model has 40 pixels"):
        call(_fake_model(), wav_grid=R.grid(41)[0])
    with pytest.raises(QFAHipError, match="2 max_shift"):
        call(_fake_model(), max_shift=20)
    with pytest.raises(QFAHipError, match="max_shift"):
        call(_fake_model(), max_shift=-1)
    with pytest.raises(QFAHipError, match="custom tau"):
        call(_fake_model(tau_callable=partial(torch.mul, 2.0)))
    with pytest.raises(QFAHipError, match="model.mu"):
        call(_fake_model(mu=False))
    with pytest.raises(QFAHipError, match="zqso"):
        call(_fake_model(), zqso=np.array([2.0, 2.5]))
    # a grid within the tolerance passes the host check and gives its step
    g, d = check_grid(wav * (1.0 + 1e-9 * (np.arange(40) % 2)), 40, 19)
    assert abs(d - np.log10(1600.0 / 1030.0) / 40) < 1e-9 and len(g) == 40


def test_workspace_is_bounded_and_the_chunked_case_has_chunks():
    from qfa_amd import _lib
    f = _lib.lib().qfa_zscan_workspace_bytes
    npix, _, nh, m = R.CHUNK_SHAPE
    bc = R.chunk_size(f, npix, nh, m)
    print("Bc =", bc, "at", R.CHUNK_SHAPE)
    assert 4 <= bc < 64
    assert f(1 << 20, 1913, 8, 20) == f(1 << 24, 1913, 8, 20) < (1 << 27)          # bounded whatever B
    assert R.chunk_size(f, 200, 32, 40, limit=4096) > 19                          # the parity shapes stay one chunk
    for bad in ((0, 100, 8, 2), (4, 100, 0, 2), (4, 100, 33, 2), (4, 100, 8, -1), (4, 100, 8, 50), (4, 100, 8, 4097)):
        assert f(*bad) == 0, bad
    assert f(4, 101, 8, 50) > 0 and f(4, 1, 1, 0) > 0
