"""The 1D flux power spectrum without a GPU: the boundary (header, exports, size functions, every argument check), the config keys
and the command line, P1DStack's arithmetic and the numpy port of the contract (tests/_p1d_ref.py) against numpy's FFT and on white
noise of known variance."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _p1d_ref as R
from conftest import REPO

NAMES = ("qfa_p1d_stack_doubles", "qfa_p1d_workspace_bytes", "qfa_p1d_f32")


def test_boundary_declares_and_exports_the_p1d_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_p1d_t" in txt and "#define QFA_ABI_VERSION 4" in txt and "QFA/model.py:160-180" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert _lib.lib().qfa_abi_version() == 4
    assert [f[0] for f in _lib.P1DParams._fields_] == ["zT0", "dzT", "nT", "St", "p_lo", "seg_len", "nseg", "min_used", "z0", "dz", "nz"]
    assert C.sizeof(_lib.P1DParams) == 44


def test_size_functions():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_p1d_stack_doubles(3, 7, 37) == 3 * 7 * (2 + 36)
    assert h.qfa_p1d_stack_doubles(1, 4096, 1) == 4096 * 2 and h.qfa_p1d_stack_doubles(2, 1, 4096) == 2 * 4098
    for a in ((0, 7, 37), (3, 0, 37), (3, 4097, 37), (3, 7, 0), (3, 7, 4097)):
        assert h.qfa_p1d_stack_doubles(*a) == 0, a
    ok = (12, 3, 100, 37, 2, 7)                                                    # R = B S, S, Nb, L, nseg, nz
    assert h.qfa_p1d_workspace_bytes(*ok) >= 37 * 8 + 12 * 2 * (18 + 2) * 4
    for i, bad in ((0, -3), (0, 13), (1, 0), (2, 73), (3, 0), (3, 4097), (3, 51), (4, 0), (4, 3), (5, 0), (5, 4097)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_p1d_workspace_bytes(*a) == 0, a
    assert h.qfa_p1d_workspace_bytes(0, 1, 1, 1, 1, 1) > 0                          # B = 0 is a shape the call accepts
    # the per-segment rows of a launch are capped: a hundred draws of the survey shape need no more than a few launches' worth
    assert h.qfa_p1d_workspace_bytes(4096 * 100, 100, 720, 240, 3, 64) < (80 << 20)


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=3, Nb=40, prm=None, flags=0, ws_bytes=None, null=(), batch=None, outs="pns", **kw):
        bs = _lib.Batch()
        bs.zabs = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        d = dict(zT0=2.0, dzT=0.1, nT=5, St=1, p_lo=1, seg_len=13, nseg=3, min_used=2, z0=2.0, dz=0.25, nz=4)
        d.update(prm or {})
        pp = _lib.P1DParams(**d)
        need = h.qfa_p1d_workspace_bytes(2 * 3, 3, 40, 13, 3, 4)
        a = lambda name, v: None if name in null else v
        return h.qfa_p1d_f32(a("trans", P), a("ivar", P), a("b", C.byref(bs)), a("tbar", P), B, S, Nb, a("p", C.byref(pp)), flags,
                             P if "p" in outs else None, P if "n" in outs else None, P if "s" in outs else None,
                             a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("trans", "ivar", "b", "tbar", "p", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1                                                     # all three outputs NULL
    assert call(batch={"zabs": None}) == -1                                        # neither zabs nor factors
    assert call(batch={"zabs": None, "zq1": 4096}) == -1 and call(batch={"pix_ratio": 4096}) == -1   # half of the factored form
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(S=0), dict(Nb=0), dict(prm={"seg_len": 0}), dict(prm={"seg_len": 4097}), dict(prm={"nseg": 0}),
               dict(prm={"p_lo": -1}), dict(prm={"p_lo": 2}), dict(prm={"seg_len": 14}), dict(prm={"nseg": 4}), dict(Nb=39),
               dict(prm={"min_used": 0}), dict(prm={"dz": 0.0}), dict(prm={"dz": -1.0}), dict(prm={"dz": nan}), dict(prm={"z0": inf}),
               dict(prm={"nz": 0}), dict(prm={"nz": 4097}), dict(prm={"dzT": 0.0}), dict(prm={"dzT": nan}), dict(prm={"zT0": inf}),
               dict(prm={"nT": 0}), dict(prm={"nT": 4097}), dict(prm={"St": 2}), dict(prm={"St": 0}), dict(batch={"row_stride": 39})):
        assert call(**kw) == -2, kw
    # the accepted values of the same arguments, on a call with nothing to do (B = 0: no device work is reached)
    assert call(B=0, prm={"St": 3}) == 0 and call(B=0, batch={"row_stride": 40}) == 0
    for flags in (0x1, 0x100, 0x200, 0x400, 0x80 | 0x8):
        assert call(flags=flags) == -5, flags
    need = h.qfa_p1d_workspace_bytes(6, 3, 40, 13, 3, 4)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(B=0) == 0                                                          # nothing to do and no overwrite: no device work


def test_config_keys_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    import qfa_amd
    from qfa_amd.cli import build_parser
    c = Cf.get_config()
    assert c.MODEL.P1D_SEGMENTS == 0 and c.MODEL.P1D_NZBINS == 4 and c.MODEL.P1D_MIN_USED_FRAC == 0.75
    for k in ("MODEL.P1D_SEGMENTS", "MODEL.P1D_NZBINS", "MODEL.P1D_MIN_USED_FRAC"):
        assert k in Cf.EXTRA_KEYS
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.P1D_SEGMENTS", "3", "MODEL.P1D_NZBINS", "6",
                                      "MODEL.P1D_MIN_USED_FRAC", "0.5", "MODEL.FOREST_NBINS", "15"])
    c = Cf.get_config(args)
    assert c.MODEL.P1D_SEGMENTS == 3 and c.MODEL.P1D_NZBINS == 6 and c.MODEL.P1D_MIN_USED_FRAC == 0.5 and c.MODEL.FOREST_NBINS == 15
    assert qfa_amd.P1DStack is model.P1DStack
    sig = inspect.signature(model.QFA.p1d)
    assert list(sig.parameters)[1:3] == ["trans", "ivar"]
    # (beyond the tail the issue lists: tbar_bins defaults to None -- a ForestStack carries its own -- and dv = 1.0 is the pixel
    # width the stack made from `bins` reports k and P in)
    want = {"zabs": None, "zfac": None, "batch": None, "tbar_bins": None, "pixel_start": 0, "bins": None, "stack": None,
            "return_segments": True, "dv": 1.0}
    for k, d in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d, k
    for k in ("tbar", "seg_len", "n_segments", "min_used"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is inspect.Parameter.empty, k
    sig = inspect.signature(model.QFA.flux_power)
    assert list(sig.parameters)[1:5] == ["dataloader", "z_min", "z_max", "n_zbins"]
    want = {"n_segments": 3, "seg_len": None, "min_used_frac": 0.75, "tbar": None, "tbar_nbins": 64, "n_samples": 0, "seed": 0,
            "batch_size": 4096, "cont_min": 0.0, "dv": None}
    for k, d in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d, k


def test_cli_refuses_p1d_without_forest_bins_before_any_work(tmp_path):
    """a configuration error: raised before the data are read, a device is touched or a file is predicted"""
    from qfa_amd import cli
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="P1D_SEGMENTS"):
        cli.main(["--type", "predict", "--output_dir", str(out), "--catalog", str(tmp_path / "none.csv"),
                  "--opts", "MODEL.P1D_SEGMENTS", "3"])
    assert not (out / "predict").exists()


@pytest.mark.parametrize("L", [1, 2, 5, 37, 64, 240])
def test_port_dft_equals_numpy_rfft(L):
    rng = np.random.default_rng(L)
    d = rng.normal(0, 1, (7, L))
    X = d @ R.dft_matrix(L)
    M = L // 2
    assert X.shape == (7, M)
    ref = np.fft.rfft(d, axis=1)[:, 1:M + 1]
    assert (np.abs(X - ref) <= 1e-12 * np.abs(d).sum(1)[:, None]).all()


def test_port_on_white_noise_of_known_variance():
    """T = 1 + sigma eps at tbar = 1 and ivar = 1 / sigma^2: <P_m> = sigma^2 = N for every mode -- the normalisation of P and N"""
    rng = np.random.default_rng(11)
    nsg, L, sigma = 20000, 64, 0.25
    trans = (1.0 + sigma * rng.normal(0, 1, (nsg, 1, L))).astype(np.float32)
    ivar = np.full((nsg, 1, L), 1.0 / sigma ** 2, np.float32)
    z = np.full((nsg, L), 2.5, np.float32)
    r = R.p1d(trans, ivar, z, np.ones((1, 3), np.float32), (2.0, 0.5, 3), 0, L, 1, L, (2.0, 1.0, 1))
    assert r["valid"].all() and (r["N"] == np.float32(sigma) ** 2).all() and (r["kz"] == 0).all()
    diff = r["P"][:, 0, 0, :] - r["N"][:, 0, 0, None]                              # (nsg, M)
    mean, se = diff.mean(0), diff.std(0, ddof=1) / np.sqrt(nsg)
    assert (np.abs(mean) <= 4 * se).all(), np.abs(mean / se).max()
    assert np.allclose(se[:-1], sigma ** 2 / np.sqrt(nsg), rtol=0.1)               # chi^2_2 / 2: the scatter equals the mean
    st = r["stack"][0, 0]
    assert st[0] == nsg and np.isclose(st[1], nsg * sigma ** 2) and np.allclose(st[2:2 + L // 2] / nsg - st[1] / nsg, mean)


def test_port_masks_bins_and_validity_by_hand():
    """L = 2, two segments from pixel 1 on: d = T / tb - 1 with tb looked up by z; an unused pixel is d = v = 0"""
    trans = np.array([[[9.0, 0.5, 1.5, np.nan, 0.25, 7.0]]], np.float32)
    ivar = np.array([[[1.0, 4.0, 16.0, 0.0, 4.0, 1.0]]], np.float32)
    z = np.array([[2.0, 2.1, 2.2, 2.3, 2.6, 2.7]], np.float32)
    tbar = np.array([[1.0, 0.5]], np.float32)                                      # bins [2, 2.5), [2.5, 3)
    r = R.p1d(trans, ivar, z, tbar, (2.0, 0.5, 2), 1, 2, 2, 1, (2.0, 0.5, 2))
    assert r["d"].tolist() == [[[[-0.5, 0.5], [0.0, -0.5]]]] and r["n_used"].tolist() == [[[2, 1]]]
    # X_1 = d_0 - d_1; P = X^2 / 2; N = sum v / 2 with v = 1 / (ivar tb^2)
    assert r["P"].tolist() == [[[[0.5], [0.125]]]] and r["N"].tolist() == [[[(0.25 + 0.0625) / 2, 1.0 / 2]]]
    assert r["kz"].tolist() == [[0, 1]]                                            # the central pixels: z = 2.2 and 2.6
    assert r["stack"].tolist() == [[[1.0, 0.15625, 0.5, 0.25], [1.0, 0.5, 0.125, 0.015625]]]
    r = R.p1d(trans, ivar, z, tbar, (2.0, 0.5, 2), 1, 2, 2, 2, (2.0, 0.5, 2))     # min_used = 2: the second segment leaves
    assert r["valid"].tolist() == [[[True, False]]] and r["P"][0, 0, 1, 0] == 0 and r["N"][0, 0, 1] == 0
    assert r["stack"][0, 1].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_p1d_stack_arithmetic():
    import torch
    from qfa_amd.model import P1DStack
    from qfa_amd._lib import QFAHipError
    # L = 4 (M = 2), two z-bins, two draws: [n | sum N | sum P_1, sum P_2 | sum P_1^2, sum P_2^2]
    buf = torch.tensor([[[4.0, 2.0, 8.0, 4.0, 20.0, 8.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]],
                        [[4.0, 2.0, 12.0, 4.0, 40.0, 4.0], [1.0, 1.0, 3.0, 2.0, 9.0, 4.0]]], dtype=torch.float64)
    st = P1DStack(buf, 2.0, 0.5, 2, 4, dv=2.0)
    assert st.S == 2 and st.M == 2 and st.bins == (2.0, 0.5, 2) and st.L == 4 and st.dv == 2.0
    assert st.z_centers.tolist() == [2.25, 2.75] and st.z_edges.tolist() == [2.0, 2.5, 3.0]
    assert np.allclose(st.k.numpy(), [2 * np.pi / 8, 4 * np.pi / 8])
    assert st.n.tolist() == [[4.0, 0.0], [4.0, 1.0]] and st.noise[:, 0].tolist() == [0.5, 0.5]
    assert st.power_raw[:, 0].tolist() == [[2.0, 1.0], [3.0, 1.0]] and torch.isnan(st.power_raw[0, 1]).all()
    assert st.power()[:, 0].tolist() == [[3.0, 1.0], [5.0, 1.0]]                   # (raw - noise) dv
    # err: sqrt((<P^2> - <P>^2) / (n - 1)) dv = sqrt((5 - 4) / 3) 2, sqrt((2 - 1) / 3) 2; NaN on a single segment
    assert np.allclose(st.err()[0, 0].numpy(), [2 / np.sqrt(3.0), 2 / np.sqrt(3.0)])
    assert np.allclose(st.err()[1, 0].numpy(), [2 * np.sqrt(1.0 / 3.0), 0.0]) and torch.isnan(st.err()[1, 1]).all()
    k = st.k.numpy()
    w2 = (np.sinc(k * 2.0 / (2 * np.pi)) * np.exp(-0.5 * (k * 3.0) ** 2)) ** 2
    assert np.allclose(st.window2(3.0).numpy(), w2) and np.allclose(st.power(3.0)[:, 0].numpy(), st.power()[:, 0].numpy() / w2)
    assert st.mean_over_draws[0].tolist() == [4.0, 1.0] and np.allclose(st.std_over_draws[0].numpy(), [np.sqrt(2.0), 0.0])
    twice = st.clone().add_(st)
    assert torch.equal(twice.buf, 2 * buf) and torch.equal(twice.power()[:, 0], st.power()[:, 0]) and torch.equal(st.buf, buf)
    assert st.draws(1, 2).S == 1 and st.draws(1, 2).buf.data_ptr() == buf[1:].data_ptr()
    with pytest.raises(QFAHipError):
        st.draws(0, 1).std_over_draws
    for other in (st.draws(0, 1), P1DStack(buf.clone(), 2.0, 0.25, 2, 4, dv=2.0), P1DStack(buf.clone(), 2.0, 0.5, 2, 5, dv=2.0),
                  P1DStack(buf.clone(), 2.0, 0.5, 2, 4, dv=1.0)):
        with pytest.raises(QFAHipError):
            st.add_(other)
    for bad in (buf.float(), buf[:, :, :5].contiguous(), buf[0]):
        with pytest.raises(QFAHipError):
            P1DStack(bad, 2.0, 0.5, 2, 4)
    with pytest.raises(QFAHipError):
        P1DStack(buf, 2.0, 0.0, 2, 4)
    assert P1DStack.zeros(3, 2.0, 0.1, 7, 37, 69.0, "cpu").buf.shape == (3, 7, 38)
