"""Band powers of the P1D and their covariance without a GPU: the boundary (header, exports, size functions, every argument check),
the config key and the command line, the numpy port (tests/_p1d_band_ref.py) by hand and on white noise of known variance, and
P1DBandStack's arithmetic on CPU tensors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _p1d_band_ref as RB
import _p1d_ref as R
from conftest import REPO

NAMES = ("qfa_p1d_band_stack_doubles", "qfa_p1d_band_workspace_bytes", "qfa_p1d_band_chunk_segments", "qfa_p1d_band_f32")


def test_boundary_declares_and_exports_the_band_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_p1d_band_t" in txt and "#define QFA_ABI_VERSION 4" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert _lib.lib().qfa_abi_version() == 4
    assert [f[0] for f in _lib.P1DBandParams._fields_] == ["nband", "band", "weight", "subtract_noise"]
    assert C.sizeof(_lib.P1DBandParams) == 32


def test_size_functions_and_the_chunk_constant():
    from qfa_amd import _lib
    h = _lib.lib()
    chunk = h.qfa_p1d_band_chunk_segments()
    assert chunk > 0
    assert h.qfa_p1d_band_stack_doubles(3, 7, 5) == 3 * 7 * (1 + 5 + 25)
    assert h.qfa_p1d_band_stack_doubles(1, 4096, 1) == 4096 * 3 and h.qfa_p1d_band_stack_doubles(2, 1, 64) == 2 * (1 + 64 + 4096)
    for a in ((0, 7, 5), (3, 0, 5), (3, 4097, 5), (3, 7, 0), (3, 7, 65), (3, 7, -1)):
        assert h.qfa_p1d_band_stack_doubles(*a) == 0, a
    ok = (12, 3, 100, 37, 2, 7, 5)                                                 # R = B S, S, Nb, L, nseg, nz, nband
    # the rows qfa_p1d_f32 needs, the sorted band list, and one chunk's partials [n | sum Q | upper triangle] per (draw, z-bin)
    assert h.qfa_p1d_band_workspace_bytes(*ok) >= 37 * 8 + 12 * 2 * (18 + 2) * 4 + (5 + 1 + 18) * 4 + 3 * 7 * (1 + 5 + 15) * 8
    for i, bad in ((0, -3), (0, 13), (1, 0), (2, 73), (3, 0), (3, 4097), (3, 51), (4, 0), (4, 3), (5, 0), (5, 4097), (6, 0), (6, 65)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_p1d_band_workspace_bytes(*a) == 0, a
    assert h.qfa_p1d_band_workspace_bytes(0, 1, 1, 1, 1, 1, 1) > 0                  # B = 0 is a shape the call accepts
    # capped as qfa_p1d_f32's rows are: the survey shape at a hundred draws and 35 bands stays near one launch's worth
    assert h.qfa_p1d_band_workspace_bytes(4096 * 100, 100, 720, 240, 3, 8, 35) < (80 << 20)


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=3, Nb=40, prm=None, band=None, flags=0, ws_bytes=None, null=(), batch=None, outs="bs"):
        bs = _lib.Batch()
        bs.zabs = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        d = dict(zT0=2.0, dzT=0.1, nT=5, St=1, p_lo=1, seg_len=13, nseg=3, min_used=2, z0=2.0, dz=0.25, nz=4)
        d.update(prm or {})
        pp = _lib.P1DParams(**d)
        q = dict(nband=3, band=4096, weight=4096, subtract_noise=1)
        q.update(band or {})
        qq = _lib.P1DBandParams(**q)
        need = h.qfa_p1d_band_workspace_bytes(2 * 3, 3, 40, 13, 3, 4, 3)
        a = lambda name, v: None if name in null else v
        return h.qfa_p1d_band_f32(a("trans", P), a("ivar", P), a("b", C.byref(bs)), a("tbar", P), B, S, Nb, a("p", C.byref(pp)),
                                  a("q", C.byref(qq)), flags, P if "b" in outs else None, P if "s" in outs else None,
                                  a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("trans", "ivar", "b", "tbar", "p", "q", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1 and call(band={"band": None}) == -1                 # both outputs NULL; no band array
    assert call(batch={"zabs": None}) == -1
    assert call(batch={"zabs": None, "zq1": 4096}) == -1 and call(batch={"pix_ratio": 4096}) == -1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(S=0), dict(Nb=0), dict(prm={"seg_len": 0}), dict(prm={"seg_len": 4097}), dict(prm={"nseg": 0}),
               dict(prm={"p_lo": -1}), dict(prm={"p_lo": 2}), dict(prm={"seg_len": 14}), dict(prm={"nseg": 4}), dict(Nb=39),
               dict(prm={"min_used": 0}), dict(prm={"dz": 0.0}), dict(prm={"dz": -1.0}), dict(prm={"dz": nan}), dict(prm={"z0": inf}),
               dict(prm={"nz": 0}), dict(prm={"nz": 4097}), dict(prm={"dzT": 0.0}), dict(prm={"dzT": nan}), dict(prm={"zT0": inf}),
               dict(prm={"nT": 0}), dict(prm={"nT": 4097}), dict(prm={"St": 2}), dict(prm={"St": 0}), dict(batch={"row_stride": 39}),
               dict(band={"nband": 0}), dict(band={"nband": 65}), dict(band={"nband": -1}), dict(band={"subtract_noise": 2}),
               dict(band={"subtract_noise": -1})):
        assert call(**kw) == -2, kw
    # the accepted values of the same arguments, on a call with nothing to do (B = 0: no device work is reached)
    assert call(B=0, prm={"St": 3}) == 0 and call(B=0, batch={"row_stride": 40}) == 0
    assert call(B=0, band={"nband": 64}, ws_bytes=1 << 30) == 0 and call(B=0, band={"subtract_noise": 0, "weight": None}) == 0
    assert call(B=0, outs="b") == 0 and call(B=0, outs="s") == 0                   # either output alone
    for flags in (0x1, 0x100, 0x200, 0x400, 0x80 | 0x8):
        assert call(flags=flags) == -5, flags
    need = h.qfa_p1d_band_workspace_bytes(6, 3, 40, 13, 3, 4, 3)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(B=0) == 0


def test_config_key_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    import qfa_amd
    from qfa_amd.cli import build_parser
    assert Cf.get_config().MODEL.P1D_NBANDS == 0 and "MODEL.P1D_NBANDS" in Cf.EXTRA_KEYS
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.P1D_NBANDS", "12", "MODEL.P1D_SEGMENTS", "3"])
    assert Cf.get_config(args).MODEL.P1D_NBANDS == 12
    assert qfa_amd.P1DBandStack is model.P1DBandStack
    sig = inspect.signature(model.QFA.p1d_bands)
    assert list(sig.parameters)[1:3] == ["trans", "ivar"]
    want = {"zabs": None, "zfac": None, "batch": None, "tbar_bins": None, "pixel_start": 0, "bins": None, "stack": None,
            "return_segments": False, "dv": 1.0, "resolution_kms": None, "subtract_noise": True}
    for k, d in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d, k
    for k in ("tbar", "seg_len", "n_segments", "min_used", "k_edges"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is inspect.Parameter.empty, k
    sig = inspect.signature(model.QFA.band_power)
    assert list(sig.parameters)[1:6] == ["dataloader", "z_min", "z_max", "n_zbins", "k_edges"]
    fp = inspect.signature(model.QFA.flux_power)
    for k, prm in fp.parameters.items():                                          # every keyword of flux_power, same defaults
        if prm.kind is inspect.Parameter.KEYWORD_ONLY:
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == prm.default, k
    assert sig.parameters["resolution_kms"].default is None


def test_cli_refuses_bands_without_segments_before_any_work(tmp_path):
    from qfa_amd import cli
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="P1D_NBANDS"):
        cli.main(["--type", "predict", "--output_dir", str(out), "--catalog", str(tmp_path / "none.csv"),
                  "--opts", "MODEL.P1D_NBANDS", "8", "MODEL.FOREST_NBINS", "10"])
    assert not out.exists()


def test_band_map_by_hand():
    import torch
    from qfa_amd.model import P1DBandStack
    # L = 8, dv = 1: k_m = 2 pi m / 8 = 0.785, 1.571, 2.356, 3.142
    edges = [0.5, 1.7, 2.5]
    band, count = RB.band_map(8, 1.0, edges)
    assert band.tolist() == [0, 0, 1, -1] and count.tolist() == [2, 1]
    st = P1DBandStack.zeros(1, 2.0, 0.5, 2, 8, 1.0, edges, "cpu")
    b2, c2 = st.band_map()
    assert b2.dtype == np.int32 and b2.tolist() == [0, 0, 1, -1] and c2.tolist() == [2, 1]
    assert np.allclose(st.k_centers.numpy(), [2 * np.pi * 1.5 / 8, 2 * np.pi * 3 / 8]) and st.k_edges.tolist() == edges
    # an edge exactly on a mode: the band is [lo, hi); L = 9 (odd, M = 4), dv = 2: an empty band gives NaN for its centre
    k = RB.mode_k(9, 2.0)
    band, count = RB.band_map(9, 2.0, [k[0], k[1], k[1] * 1.01, 10.0])
    assert band.tolist() == [0, 1, 2, 2] and count.tolist() == [1, 1, 2]
    st = P1DBandStack.zeros(1, 2.0, 0.5, 2, 9, 2.0, [0.01, 0.02, 0.03, 10.0], "cpu")
    assert st.band_map()[1].tolist() == [0, 0, 4] and torch.isnan(st.k_centers[:2]).all()
    # the command line's bands: every mode in a band, equal widths from the fundamental to Nyquist
    for L, nb in ((24, 3), (37, 5), (240, 35)):
        e = P1DBandStack.linear_k_edges(L, 69.0, nb)
        band, count = RB.band_map(L, 69.0, e)
        assert (band >= 0).all() and count.sum() == L // 2 and (np.diff(band) >= 0).all() and count.max() - count.min() <= 1
    # weights: dv / n_a, the window folded in
    w = RB.weights(8, 3.0, [0.1, 0.6, 0.9])                                         # k = 0.262, 0.524, 0.785, 1.047
    assert w.tolist() == [1.5, 1.5, 3.0, 0.0]
    w2 = RB.weights(8, 3.0, [0.1, 0.6, 0.9], resolution_kms=2.0)
    k = RB.mode_k(8, 3.0)
    assert np.allclose(w2[:3], w[:3] / (np.sinc(k * 3 / (2 * np.pi)) * np.exp(-0.5 * (2 * k) ** 2))[:3] ** 2, rtol=1e-6)


def test_band_average_of_a_constant_spectrum_is_the_constant():
    L, dv = 37, 2.5
    edges = [0.0, 0.2, 0.201, 0.5, 2.0]                                             # (the second band is empty)
    band, count = RB.band_map(L, dv, edges)
    assert count[1] == 0 and count.sum() == L // 2
    P = np.full((3, L // 2), 0.75)
    Q, dQ = RB.band_q(P, np.full(3, 0.25), band, RB.weights(L, dv, edges), 1, 4)
    want = np.where(count > 0, 0.5 * dv, 0.0)
    assert (np.abs(Q - want) <= dQ + 1e-7 * want).all() and (Q[:, 1] == 0).all()   # (1e-7: the weights are float32)
    Q0, _ = RB.band_q(P, np.full(3, 0.25), band, None, 0, 4)                        # unit weights, noise kept: n_a times the constant
    assert np.allclose(Q0, 0.75 * count)


@pytest.fixture(scope="module")
def white_noise():
    """T = 1 + sigma eps at tbar = 1, ivar = 1 / sigma^2, no mask: L = 64, 4000 segments, four bands over the modes 1 .. 31 (the
    Nyquist mode is real, its power is chi^2_1 and not chi^2_2 / 2, so it stays outside)"""
    rng = np.random.default_rng(11)
    nsg, L, sigma = 4000, 64, 0.25
    trans = (1.0 + sigma * rng.normal(0, 1, (nsg, 1, L))).astype(np.float32)
    ivar = np.full((nsg, 1, L), 1.0 / sigma ** 2, np.float32)
    z = np.full((nsg, L), 2.5, np.float32)
    r = R.p1d(trans, ivar, z, np.ones((1, 3), np.float32), (2.0, 0.5, 3), 0, L, 1, L, (2.0, 1.0, 1))
    k = RB.mode_k(L, 1.0)
    edges = [0.5 * k[0], 0.5 * (k[7] + k[8]), 0.5 * (k[15] + k[16]), 0.5 * (k[23] + k[24]), 0.5 * (k[30] + k[31])]
    band, count = RB.band_map(L, 1.0, edges)
    assert count.tolist() == [8, 8, 8, 7] and band[31] == -1
    Q, dQ = RB.band_q(r["P"], r["N"], band, RB.weights(L, 1.0, edges), 0, 4)
    stack, _ = RB.stack_of(Q, dQ, r["valid"], r["kz"], 1)
    return nsg, sigma, count, stack


def test_port_band_means_recover_the_variance(white_noise):
    """P_m = sigma^2 chi^2_2 / 2 independently per mode (the field is Gaussian and white): Q_a, the mean of n_a of them, has mean
    sigma^2 and variance sigma^4 / n_a; the mean of n segments has standard error sigma^2 / sqrt(n_a n)"""
    n, sigma, count, stack = white_noise
    mean, _ = RB.cov_of(stack, 4)
    assert stack[0, 0, 0] == n
    se = sigma ** 2 / np.sqrt(count * n)
    assert (np.abs(mean[0, 0] - sigma ** 2) <= 5 * se).all(), np.abs(mean[0, 0] - sigma ** 2) / se


def test_port_covariance_is_diagonal_with_the_known_variance(white_noise):
    """cov n is the unbiased sample covariance s_ab of the Q.  Q_a is Gamma(n_a, sigma^2 / n_a): v_a = sigma^4 / n_a and, from the
    Gaussian field's eighth moment, mu_4 = 3 v_a^2 (1 + 2 / n_a).  Var s_aa = (mu_4 - v_a^2 (n - 3) / (n - 1)) / n and, the bands
    being independent, Var s_ab = v_a v_b / (n - 1)"""
    n, sigma, count, stack = white_noise
    _, cov = RB.cov_of(stack, 4)
    s = cov[0, 0] * n
    v = sigma ** 4 / count
    mu4 = 3 * v ** 2 * (1 + 2.0 / count)
    se_diag = np.sqrt((mu4 - v ** 2 * (n - 3) / (n - 1)) / n)
    assert (np.abs(np.diag(s) - v) <= 5 * se_diag).all(), np.abs(np.diag(s) - v) / se_diag
    se_off = np.sqrt(np.outer(v, v) / (n - 1))
    off = ~np.eye(4, dtype=bool)
    assert (np.abs(s[off]) <= 5 * se_off[off]).all(), (np.abs(s) / se_off)[off].max()
    assert np.array_equal(s, s.T)


def test_p1d_band_stack_arithmetic():
    import torch
    from qfa_amd.model import P1DBandStack
    from qfa_amd._lib import QFAHipError
    rng = np.random.default_rng(3)
    B, S, nseg, nb, nz = 40, 3, 2, 3, 3
    Q = rng.normal(1.0, 0.3, (B, S, nseg, nb))
    ok = rng.random((B, S, nseg)) < 0.9
    kz = rng.integers(-1, 2, (B, nseg))                                            # bins 0 and 1 fill, bin 2 stays empty
    kz[0, 0], ok[0, :, 0] = 2, True
    kz[1:, :] = np.minimum(kz[1:, :], 1)                                           # ... but for one segment: n = 1 in bin 2
    edges = [0.1, 0.2, 0.3, 0.4]
    whole, _ = RB.stack_of(Q, np.zeros_like(Q), ok, kz, nz)
    st = P1DBandStack(torch.tensor(whole), 2.0, 0.5, nz, 24, 2.0, edges)
    assert st.S == S and st.nband == nb and st.bins == (2.0, 0.5, 3) and st.L == 24 and st.M == 12 and st.dv == 2.0
    assert st.z_centers.tolist() == [2.25, 2.75, 3.25] and st.z_edges.tolist() == [2.0, 2.5, 3.0, 3.5]
    assert st.n[:, 2].tolist() == [1.0, 1.0, 1.0] and (st.n[:, :2] > 5).all()
    mean, cov = RB.cov_of(whole, nb)
    assert np.allclose(st.mean.numpy(), mean, rtol=1e-14) and st.mean.shape == (S, nz, nb)
    c = st.cov
    assert c.shape == (S, nz, nb, nb) and torch.equal(c[:, :2], c[:, :2].transpose(2, 3))     # symmetric to the bit
    assert torch.isnan(c[:, 2]).all() and torch.isfinite(c[:, :2]).all()                      # NaN at n < 2
    assert np.allclose(c[:, :2].numpy(), cov[:, :2], rtol=1e-9, atol=1e-15)
    # against numpy's own covariance of the mean on one (draw, bin)
    sel = ok[:, 1, :] & (kz == 0)
    assert np.allclose(c[1, 0].numpy(), np.cov(Q[:, 1][sel].T, ddof=1) / sel.sum(), rtol=1e-9)
    assert np.allclose(st.err[:, :2].numpy() ** 2, np.diagonal(cov[:, :2], axis1=2, axis2=3), rtol=1e-9)
    cr = st.corr[:, :2]
    assert np.allclose(torch.diagonal(cr, dim1=2, dim2=3).numpy(), 1.0) and (cr.abs() <= 1 + 1e-12).all()
    # draws: the continuum posterior's covariance, and the total
    mod = np.cov(mean[:, 0].T, ddof=1)
    assert st.mean_over_draws.shape == (nz, nb) and np.allclose(st.mean_over_draws[0].numpy(), mean[:, 0].mean(0))
    assert st.cov_over_draws.shape == (nz, nb, nb) and np.allclose(st.cov_over_draws[0].numpy(), mod, rtol=1e-9, atol=1e-18)
    assert torch.equal(st.total_cov[:2], (st.cov.mean(0) + st.cov_over_draws)[:2])
    assert np.allclose(st.total_cov[0].numpy(), cov[:, 0].mean(0) + mod, rtol=1e-9)
    # add_ of two halves is the whole; clone is a copy; draws is a view
    h1, _ = RB.stack_of(Q[:17], np.zeros_like(Q[:17]), ok[:17], kz[:17], nz)
    h2, _ = RB.stack_of(Q[17:], np.zeros_like(Q[17:]), ok[17:], kz[17:], nz)
    a = P1DBandStack(torch.tensor(h1), 2.0, 0.5, nz, 24, 2.0, edges)
    both = a.clone().add_(P1DBandStack(torch.tensor(h2), 2.0, 0.5, nz, 24, 2.0, edges))
    assert torch.equal(both.n, st.n) and np.allclose(both.buf.numpy(), whole, rtol=1e-13) and np.array_equal(a.buf.numpy(), h1)
    assert st.draws(1, 2).S == 1 and st.draws(1, 2).buf.data_ptr() == st.buf[1:].data_ptr()
    with pytest.raises(QFAHipError):
        st.draws(0, 1).cov_over_draws
    with pytest.raises(QFAHipError):
        st.draws(0, 1).total_cov
    mk = lambda **kw: P1DBandStack(**{**dict(buf=st.buf.clone(), z0=2.0, dz=0.5, nz=nz, L=24, dv=2.0, k_edges=edges), **kw})
    for other in (st.draws(0, 1), mk(dz=0.25), mk(L=25), mk(dv=1.0), mk(k_edges=[0.1, 0.2, 0.3, 0.5])):
        with pytest.raises(QFAHipError):
            st.add_(other)
    for bad in (dict(buf=st.buf.float()), dict(buf=st.buf[:, :, :5].contiguous()), dict(buf=st.buf[0]), dict(dz=0.0),
                dict(k_edges=[0.1, 0.3, 0.2, 0.4]), dict(k_edges=[0.1]), dict(k_edges=[0.1, 0.2, 0.3])):
        with pytest.raises(QFAHipError):
            mk(**bad)
    assert P1DBandStack.zeros(3, 2.0, 0.1, 7, 37, 69.0, np.linspace(0.001, 0.05, 6), "cpu").buf.shape == (3, 7, 31)
