"""The line-of-sight correlation function without a GPU: the numpy port (tests/_xi_ref.py) against the double loop of the definition
and against the autocorrelation identity with numpy.fft, the inputs of the GPU tests' shapes, XiStack's arithmetic on CPU tensors,
the boundary (header, exports, size functions, argument checks) and the config keys and command line."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _forest_ref as RF
import _xi_ref as R
from conftest import REPO

NAMES = ("qfa_xi_stack_doubles", "qfa_xi_workspace_bytes", "qfa_xi_f32")
TB_BINS = (1.5, 0.125, 17)


def _inputs(rng, B, S, nb, masked=0.2):
    trans = rng.uniform(0.2, 1.2, (B, S, nb)).astype(np.float32)
    ivar = rng.uniform(10.0, 100.0, (B, S, nb)).astype(np.float32)
    ivar[rng.random((B, S, nb)) < masked] = 0
    z = (rng.uniform(1.7, 2.0, (B, 1)) + np.linspace(0.0, 1.2, nb)[None, :]).astype(np.float32)
    tbar = rng.uniform(0.3, 0.9, (S, TB_BINS[2])).astype(np.float32)
    return trans, ivar, z, tbar


@pytest.mark.parametrize("sigma2,unit", [(0.0, False), (0.1, False), (0.0, True)])
def test_port_against_the_double_loop(sigma2, unit):
    rng = np.random.default_rng(1)
    B, S, L, nseg, p_lo, nlag = 3, 2, 13, 2, 1, 13
    trans, ivar, z, tbar = _inputs(rng, B, S, p_lo + nseg * L + 2)
    r = R.xi(trans, ivar, z, tbar, TB_BINS, p_lo, L, nseg, 11, (1.6, 0.45, 4), nlag, sigma2, unit)
    assert r["valid"].any() and not r["valid"].all()
    for b in range(B):
        for s in range(S):
            for g in range(nseg):
                W, A, N0 = R.brute_force(r["w"][b, s, g], r["x"][b, s, g], r["v"][b, s, g], nlag)
                if not r["valid"][b, s, g]:
                    W, A, N0 = 0 * W, 0 * A, 0.0
                assert np.allclose(r["W"][b, s, g], W, rtol=1e-13, atol=0) and np.allclose(r["A"][b, s, g], A, rtol=1e-12, atol=1e-300)
                assert np.isclose(r["N0"][b, s, g], N0, rtol=1e-13)
    # the per-pixel rule by hand on one used and one masked pixel
    b, s, j = 0, 0, p_lo
    used = ivar[b, s, j] > 0
    tb = tbar[s, int(np.floor((z[b, j] - np.float32(1.5)) * (np.float32(1.0) / np.float32(0.125))))]
    v = np.float32(1.0) / (ivar[b, s, j] * (tb * tb)) if used else np.float32(0.0)
    w = (np.float32(1.0) if unit else np.float32(1.0) / (v + np.float32(sigma2))) if used else np.float32(0.0)
    d = (trans[b, s, j] / tb - np.float32(1.0)) if used else np.float32(0.0)
    assert r["w"][b, s, 0, 0] == w and r["x"][b, s, 0, 0] == np.float32(w * d) and r["v"][b, s, 0, 0] == v
    assert (r["w"][~(ivar[:, :, p_lo:p_lo + nseg * L].reshape(B, S, nseg, L) > 0)] == 0).all()
    # the stack: counts, and the sums of the rows
    sel = r["valid"] & (r["kz"][:, None, :] >= 0)
    assert r["stack"][:, :, 0].sum() == sel.sum() > 0
    assert np.allclose(r["stack"][:, :, 2:2 + nlag].sum((0, 1)), r["W"][sel].sum(0), rtol=1e-13)
    assert np.allclose(r["stack"][:, :, 2 + 3 * nlag:2 + 4 * nlag].sum((0, 1)), (r["A"] * r["W"])[sel].sum(0), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("L", [16, 37])
def test_port_against_the_autocorrelation_identity(L):
    """unit weights, no mask, nlag = L: |FFT(d)_m|^2 = A_0 + 2 sum_{l >= 1} A_l cos(2 pi l m / L), and the zero-padded FFT returns
    the A_l themselves"""
    rng = np.random.default_rng(L)
    trans, ivar, z, tbar = _inputs(rng, 4, 1, L + 3, masked=0.0)
    r = R.xi(trans, ivar, z, tbar, TB_BINS, 2, L, 1, L, (1.6, 0.45, 4), L, 0.0, True)
    assert r["valid"].all() and (r["W"] == (L - np.arange(L))).all()
    d = r["x"][:, 0, 0]                                                                # (4, L): x = d at unit weights
    P = np.abs(np.fft.fft(d, axis=-1)) ** 2
    l, m = np.arange(1, L), np.arange(L)
    A = r["A"][:, 0, 0]
    assert np.allclose(P, A[:, :1] + 2.0 * A[:, 1:] @ np.cos(2.0 * np.pi * l[:, None] * m[None, :] / L), rtol=1e-11, atol=1e-12)
    acf = np.fft.irfft(np.abs(np.fft.rfft(d, 2 * L, axis=-1)) ** 2, 2 * L, axis=-1)[:, :L]
    assert np.allclose(acf, A, rtol=1e-11, atol=1e-12)


def test_inputs_of_the_gpu_shapes_have_segments_on_both_sides_of_min_used():
    """the first GPU test asserts valid segments at L >= 37 and invalid ones too at rows >= 16: confirmed here on the ports' own
    inputs (the forest port in the place of the kernel that writes trans / ivar; validity depends on ivar > 0 alone)"""
    from test_forest import geometry
    from test_xi import BINS, CASES, case_shape
    for rows, L, nseg, p_lo, nlag in CASES:
        if L < 37:
            continue
        B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
        g = geometry(nb + 20, nb, 4, B, S, seed)
        f = RF.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zabs"], g["mask"], g["h"], None, (1.5, 0.5, 4), 0.05)
        tbar = np.random.default_rng(seed + 1).uniform(0.3, 0.9, (S, TB_BINS[2])).astype(np.float32)
        tr, iv = np.where(f["use"], f["T"], 0).astype(np.float32), np.where(f["use"], f["iv"], 0).astype(np.float32)
        valid = R.xi(tr, iv, g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, BINS, min(nlag, 3))["valid"]
        assert valid.any() and (rows < 16 or not valid.all()), (rows, L)


def test_bars_hold_for_float32_sums_in_other_orders():
    """the pair bar is a statement about float32 summation: a float32 chain, a pairwise tree and four interleaved chains of the
    same products all stay inside it"""
    rng = np.random.default_rng(5)
    L, nlag = 667, 256
    x = rng.normal(0, 1, L).astype(np.float32)
    exact, sabs = R.lag_sums(x.astype(np.float64)[None, :], nlag)
    bar = R.pair_bound(sabs, L)[0]
    for l in (0, 1, 100, 255):
        p = (x[:L - l] * x[l:]).astype(np.float32)
        chain = np.float32(0)
        for t in p:
            chain = np.float32(chain + t)
        four = sum(np.add.reduce(p[i::4], dtype=np.float32) for i in range(4))
        for got in (chain, np.add.reduce(p, dtype=np.float32), np.float32(four)):
            assert abs(float(got) - exact[0, l]) <= bar[l], l


def test_xi_stack_arithmetic():
    import torch
    import qfa_amd
    from qfa_amd._lib import QFAHipError
    from qfa_amd.model import XiStack
    assert qfa_amd.XiStack is XiStack
    rng = np.random.default_rng(3)
    B, S, nseg, nlag, nz, L = 40, 3, 2, 5, 3, 24
    W = rng.uniform(5.0, 10.0, (B, S, nseg, nlag))
    A = rng.normal(0.5, 0.3, (B, S, nseg, nlag)) * W
    N0 = rng.uniform(0.1, 0.2, (B, S, nseg))
    ok = rng.random((B, S, nseg)) < 0.9
    kz = rng.integers(-1, 2, (B, nseg))
    kz[0, 0], ok[0, :, 0] = 2, True
    kz[1:, :] = np.minimum(kz[1:, :], 1)                                           # bin 2 holds one segment
    pairs = np.stack([W, A], axis=3)
    whole, _ = R.stack_of(pairs, N0, ok, kz, nz)
    st = XiStack(torch.tensor(whole), 2.0, 0.5, nz, L, nlag, 69.0)
    assert st.S == S and st.nlag == nlag and st.bins == (2.0, 0.5, 3) and st.L == L and st.dv == 69.0
    assert st.lags_kms.tolist() == [0.0, 69.0, 138.0, 207.0, 276.0] and st.n[:, 2].tolist() == [1.0, 1.0, 1.0]
    for s in range(S):
        for k in range(2):
            sel = ok[:, s, :] & (kz == k)
            w, a, n0 = W[:, s][sel], A[:, s][sel], N0[:, s][sel]
            n = sel.sum()
            assert st.n[s, k] == n
            xi_raw = a.sum(0) / w.sum(0)
            assert np.allclose(st.xi(subtract_noise=False)[s, k].numpy(), xi_raw, rtol=1e-13)
            sub = a.sum(0).copy()
            sub[0] -= n0.sum()
            assert np.allclose(st.xi()[s, k].numpy(), sub / w.sum(0), rtol=1e-12)
            assert np.allclose(st.xi()[s, k, 1:].numpy(), xi_raw[1:], rtol=1e-13)   # only lag 0 holds noise
            # the delta method, directly per segment: residuals r_i = A_i - xi W_i around the ratio
            res = a - xi_raw[None, :] * w
            direct = np.sqrt((res ** 2).sum(0) / w.sum(0) ** 2 * n / (n - 1))
            assert np.allclose(st.err()[s, k].numpy(), direct, rtol=1e-8)
    assert torch.isnan(st.err()[:, 2]).all() and torch.isfinite(st.xi()[:, 2]).all()     # one segment: a ratio, no error
    empty = XiStack.zeros(2, 2.0, 0.5, nz, L, nlag, 69.0, "cpu")
    assert empty.buf.shape == (2, 3, 27) and torch.isnan(empty.xi()).all() and torch.isnan(empty.err()).all()
    assert st.mean_over_draws.shape == (nz, nlag) and torch.allclose(st.mean_over_draws, st.xi().mean(0), equal_nan=True)
    assert torch.allclose(st.std_over_draws[:2], st.xi()[:, :2].std(0, unbiased=True))
    # add_ of two halves is the whole; draws is a view; layouts are checked
    h1, _ = R.stack_of(pairs[:17], N0[:17], ok[:17], kz[:17], nz)
    h2, _ = R.stack_of(pairs[17:], N0[17:], ok[17:], kz[17:], nz)
    a = XiStack(torch.tensor(h1), 2.0, 0.5, nz, L, nlag, 69.0)
    both = a.clone().add_(XiStack(torch.tensor(h2), 2.0, 0.5, nz, L, nlag, 69.0))
    assert torch.equal(both.n, st.n) and np.allclose(both.buf.numpy(), whole, rtol=1e-13) and np.array_equal(a.buf.numpy(), h1)
    assert st.draws(1, 2).S == 1 and st.draws(1, 2).buf.data_ptr() == st.buf[1:].data_ptr()
    with pytest.raises(QFAHipError):
        st.draws(0, 1).std_over_draws
    mk = lambda **kw: XiStack(**{**dict(buf=st.buf.clone(), z0=2.0, dz=0.5, nz=nz, L=L, n_lags=nlag, dv=69.0), **kw})
    for other in (st.draws(0, 1), mk(dz=0.25), mk(L=25), mk(dv=1.0)):
        with pytest.raises(QFAHipError):
            st.add_(other)
    for bad in (dict(buf=st.buf.float()), dict(buf=st.buf[:, :, :5].contiguous()), dict(n_lags=4), dict(n_lags=0), dict(L=4), dict(dz=0.0)):
        with pytest.raises(QFAHipError):
            mk(**bad)
    assert XiStack._round_bins(0.1, 0.2, 3) == (float(np.float32(0.1)), float(np.float32(0.2)), 3)


def test_boundary_declares_and_exports_the_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_xi_t" in txt and "#define QFA_F_XI_UNIT_W 0x400u" in txt and "#define QFA_ABI_VERSION 4" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert [f[0] for f in _lib.XiParams._fields_] == ["nlag", "sigma2_lss"] and C.sizeof(_lib.XiParams) == 8
    assert _lib.F_XI_UNIT_W == 0x400


def test_size_functions():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_xi_stack_doubles(3, 7, 5) == 3 * 7 * (2 + 25) and h.qfa_xi_stack_doubles(1, 4096, 4096) == 4096 * (2 + 5 * 4096)
    for a in ((0, 7, 5), (3, 0, 5), (3, 4097, 5), (3, 7, 0), (3, 7, 4097), (3, 7, -1)):
        assert h.qfa_xi_stack_doubles(*a) == 0, a
    ok = (12, 3, 100, 37, 2, 7, 20)                                                # R = B S, S, Nb, L, nseg, nz, nlag
    # the rows [code | N0 | W | A] of the segments and one chunk's partials per (draw, z-bin)
    assert h.qfa_xi_workspace_bytes(*ok) >= 12 * 2 * (2 + 2 * 20) * 4 + 3 * 7 * (2 + 5 * 20) * 8
    for i, bad in ((0, -3), (0, 13), (1, 0), (2, 73), (3, 0), (3, 4097), (3, 51), (4, 0), (4, 3), (5, 0), (5, 4097), (6, 0), (6, 38)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_xi_workspace_bytes(*a) == 0, a
    assert h.qfa_xi_workspace_bytes(12, 3, 100, 37, 2, 7, 37) > 0                    # nlag = L
    assert h.qfa_xi_workspace_bytes(0, 1, 1, 1, 1, 1, 1) > 0                         # B = 0 is a shape the call accepts
    assert h.qfa_xi_workspace_bytes(4096 * 100, 100, 720, 240, 3, 8, 120) < (80 << 20)


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=3, Nb=40, prm=None, xi=None, flags=0, ws_bytes=None, null=(), batch=None, outs="pns"):
        bs = _lib.Batch()
        bs.zabs = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        d = dict(zT0=2.0, dzT=0.1, nT=5, St=1, p_lo=1, seg_len=13, nseg=3, min_used=2, z0=2.0, dz=0.25, nz=4)
        d.update(prm or {})
        pp = _lib.P1DParams(**d)
        q = dict(nlag=7, sigma2_lss=0.1)
        q.update(xi or {})
        xx = _lib.XiParams(**q)
        need = h.qfa_xi_workspace_bytes(2 * 3, 3, 40, 13, 3, 4, 7)
        a = lambda name, v: None if name in null else v
        return h.qfa_xi_f32(a("trans", P), a("ivar", P), a("b", C.byref(bs)), a("tbar", P), B, S, Nb, a("p", C.byref(pp)),
                            a("x", C.byref(xx)), flags, P if "p" in outs else None, P if "n" in outs else None,
                            P if "s" in outs else None, a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("trans", "ivar", "b", "tbar", "p", "x", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1 and call(batch={"zabs": None}) == -1
    assert call(batch={"zabs": None, "zq1": 4096}) == -1 and call(batch={"pix_ratio": 4096}) == -1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(S=0), dict(Nb=0), dict(prm={"seg_len": 0}), dict(prm={"seg_len": 4097}), dict(prm={"nseg": 0}),
               dict(prm={"p_lo": -1}), dict(prm={"p_lo": 2}), dict(prm={"nseg": 4}), dict(Nb=39), dict(prm={"min_used": 0}),
               dict(prm={"dz": 0.0}), dict(prm={"dz": nan}), dict(prm={"z0": inf}), dict(prm={"nz": 0}), dict(prm={"nz": 4097}),
               dict(prm={"dzT": 0.0}), dict(prm={"zT0": inf}), dict(prm={"nT": 0}), dict(prm={"St": 2}), dict(batch={"row_stride": 39}),
               dict(xi={"nlag": 0}), dict(xi={"nlag": -1}), dict(xi={"nlag": 14}), dict(xi={"sigma2_lss": -1e-3}),
               dict(xi={"sigma2_lss": nan}), dict(xi={"sigma2_lss": inf})):
        assert call(**kw) == -2, kw
    # the accepted values of the same arguments, on a call with nothing to do (B = 0: no device work is reached)
    assert call(B=0, prm={"St": 3}) == 0 and call(B=0, xi={"nlag": 13}, ws_bytes=1 << 30) == 0 and call(B=0, xi={"sigma2_lss": 0.0}) == 0
    for outs in ("p", "n", "s", "pn", "ns"):
        assert call(B=0, outs=outs) == 0, outs
    assert call(B=0, flags=0x400) == 0 and call(B=0, flags=0x400 | 0x20) == 0
    for flags in (0x1, 0x100, 0x200, 0x800, 0x80 | 0x8):
        assert call(flags=flags) == -5, flags
    need = h.qfa_xi_workspace_bytes(6, 3, 40, 13, 3, 4, 7)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3


def test_config_keys_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    from qfa_amd.cli import build_parser
    cfg = Cf.get_config()
    assert cfg.MODEL.XI_NLAGS == 0 and cfg.MODEL.XI_SIGMA2_LSS == 0.0
    assert {"MODEL.XI_NLAGS", "MODEL.XI_SIGMA2_LSS"} <= set(Cf.EXTRA_KEYS)
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.XI_NLAGS", "64", "MODEL.XI_SIGMA2_LSS", "0.05"])
    got = Cf.get_config(args)
    assert got.MODEL.XI_NLAGS == 64 and got.MODEL.XI_SIGMA2_LSS == 0.05
    sig = inspect.signature(model.QFA.xi)
    assert list(sig.parameters)[1:3] == ["trans", "ivar"]
    want = {"zabs": None, "zfac": None, "batch": None, "tbar_bins": None, "pixel_start": 0, "sigma2_lss": 0.0, "unit_weights": False,
            "bins": None, "stack": None, "return_segments": True, "dv": 1.0}
    for k, d in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d, k
    for k in ("tbar", "seg_len", "n_segments", "min_used", "n_lags"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is inspect.Parameter.empty, k
    sig = inspect.signature(model.QFA.flux_correlation)
    assert list(sig.parameters)[1:6] == ["dataloader", "z_min", "z_max", "n_zbins", "n_lags"]
    for k, prm in inspect.signature(model.QFA.flux_power).parameters.items():      # every keyword of flux_power, same defaults
        if prm.kind is inspect.Parameter.KEYWORD_ONLY:
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == prm.default, k


def test_cli_refuses_lags_without_segments_or_beyond_them_before_any_work(tmp_path):
    from qfa_amd import cli
    out = tmp_path / "out"
    base = ["--type", "predict", "--output_dir", str(out), "--catalog", str(tmp_path / "none.csv")]
    with pytest.raises(ValueError, match="XI_NLAGS"):
        cli.main(base + ["--opts", "MODEL.XI_NLAGS", "8", "MODEL.FOREST_NBINS", "10"])
    # LOGLAM_DELTA 2e-3 on 1030 .. 1600 A: 36 blue pixels, two segments of 18
    opts = ["DATA.LOGLAM_DELTA", "2e-3", "MODEL.FOREST_NBINS", "10", "MODEL.P1D_SEGMENTS", "2"]
    with pytest.raises(ValueError, match="XI_NLAGS"):
        cli.main(base + ["--opts"] + opts + ["MODEL.XI_NLAGS", "19"])
    with pytest.raises(ValueError, match="XI_NLAGS"):
        cli.main(base + ["--opts"] + opts + ["MODEL.XI_NLAGS", "-1"])
    with pytest.raises(ValueError, match="XI_SIGMA2_LSS"):
        cli.main(base + ["--opts"] + opts + ["MODEL.XI_NLAGS", "18", "MODEL.XI_SIGMA2_LSS", "-1.0"])
    assert not out.exists()
