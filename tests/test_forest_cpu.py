"""Forest transmission without a GPU: the boundary (header, exports, size functions, every argument check), the config keys,
ForestStack's arithmetic and the numpy port of the contract (tests/_forest_ref.py) on a case worked by hand."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _forest_ref as R
from conftest import REPO

NAMES = ("qfa_forest_stack_doubles", "qfa_forest_workspace_bytes", "qfa_forest_f32")


def test_boundary_declares_and_exports_the_forest_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_forest_bins_t" in txt and "#define QFA_F_FOREST_UNIT_W 0x200u" in txt and "#define QFA_ABI_VERSION 4" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert _lib.F_FOREST_UNIT_W == 0x200 and _lib.lib().qfa_abi_version() == 4
    assert [f[0] for f in _lib.ForestBins._fields_] == ["z0", "dz", "nbin", "p_lo", "p_hi"] and C.sizeof(_lib.ForestBins) == 20


def test_size_functions():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_forest_stack_doubles(3, 7) == 84
    assert h.qfa_forest_stack_doubles(1, 4096) == 4 * 4096
    for S, nbin in ((0, 7), (-1, 7), (3, 0), (3, 4097)):
        assert h.qfa_forest_stack_doubles(S, nbin) == 0, (S, nbin)
    ok = (4, 3, 100, 40, 8, 7)
    assert h.qfa_forest_workspace_bytes(*ok) >= (8 + 1) * 40 * 4
    for i, bad in ((0, -1), (1, 0), (2, 0), (3, -1), (3, 101), (4, 0), (4, 33), (5, 0), (5, 4097)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_forest_workspace_bytes(*a) == 0, a
    assert h.qfa_forest_workspace_bytes(0, 1, 1, 0, 1, 1) > 0                     # B = 0, Nb = 0 are shapes the call accepts
    # the rows of partial sums grow with the table of a launch, and both forms (tables in LDS / in the workspace) are sized
    assert h.qfa_forest_workspace_bytes(4096, 1, 1913, 720, 8, 64) < h.qfa_forest_workspace_bytes(4096, 100, 1913, 720, 8, 64)
    assert h.qfa_forest_workspace_bytes(64, 2, 1913, 720, 8, 4096) > 4 * 4096 * 8


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=1, Npix=10, Nb=4, Nh=3, bins=(2.0, 0.1, 5, 0, 4), flags=0, ws_bytes=None, null=(), batch=None, outs="tis"):
        bs = _lib.Batch()
        bs.delta = bs.error = bs.zabs = bs.mask = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        fb = _lib.ForestBins(*bins)
        need = h.qfa_forest_workspace_bytes(max(B, 0), max(S, 1), max(Npix, 1), min(max(Nb, 0), max(Npix, 1)), min(max(Nh, 1), 32),
                                            min(max(bins[2], 1), 4096))
        a = lambda name, v: None if name in null else v
        return h.qfa_forest_f32(a("F", P), a("mu", P), a("b", C.byref(bs)), a("h", P), None, B, S, Npix, Nb, Nh, a("bins", C.byref(fb)),
                                0.0, flags, P if "t" in outs else None, P if "i" in outs else None, P if "s" in outs else None,
                                a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("F", "mu", "b", "h", "bins", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1                                                     # all three outputs NULL
    assert call(batch={"delta": None}) == -1 and call(batch={"error": None}) == -1
    assert call(batch={"zabs": None}) == -1                                        # blue pixels without zabs or factors
    assert call(batch={"zabs": None, "zq1": 4096}) == -1                           # half of the factored form
    for kw in (dict(B=-1), dict(S=0), dict(Npix=0), dict(Nb=-1), dict(Nb=11), dict(Nh=0), dict(Nh=33),
               dict(bins=(2.0, 0.0, 5, 0, 4)), dict(bins=(2.0, -0.1, 5, 0, 4)), dict(bins=(2.0, float("nan"), 5, 0, 4)),
               dict(bins=(float("inf"), 0.1, 5, 0, 4)), dict(bins=(2.0, 0.1, 0, 0, 4)), dict(bins=(2.0, 0.1, 4097, 0, 4)),
               dict(bins=(2.0, 0.1, 5, -1, 4)), dict(bins=(2.0, 0.1, 5, 3, 2)), dict(bins=(2.0, 0.1, 5, 0, 5)),
               dict(batch={"row_stride": 9})):
        assert call(**kw) == -2, kw
    for flags in (0x1, 0x100, 0x400, 0x80 | 0x8):
        assert call(flags=flags) == -5, flags
    need = h.qfa_forest_workspace_bytes(2, 1, 10, 4, 3, 5)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    # B = 0 and Nb = 0 without an overwrite do nothing at all: no device work, status 0
    assert call(B=0) == 0
    assert call(Nb=0, bins=(2.0, 0.1, 5, 0, 0), batch={"zabs": None}) == 0


def test_config_keys_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    from qfa_amd.cli import build_parser
    c = Cf.get_config()
    assert c.MODEL.FOREST is False and c.MODEL.FOREST_NBINS == 0
    assert c.MODEL.FOREST_ZMIN == 0.0 and c.MODEL.FOREST_ZMAX == 0.0
    for k in ("MODEL.FOREST", "MODEL.FOREST_ZMIN", "MODEL.FOREST_ZMAX", "MODEL.FOREST_NBINS"):
        assert k in Cf.EXTRA_KEYS
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.FOREST", "true", "MODEL.FOREST_ZMIN", "2",
                                      "MODEL.FOREST_ZMAX", "3.5", "MODEL.FOREST_NBINS", "15"])
    c = Cf.get_config(args)
    assert c.MODEL.FOREST is True and c.MODEL.FOREST_ZMIN == 2.0 and isinstance(c.MODEL.FOREST_ZMIN, float)
    assert c.MODEL.FOREST_ZMAX == 3.5 and c.MODEL.FOREST_NBINS == 15
    sig = inspect.signature(model.QFA.forest)
    assert list(sig.parameters)[1:5] == ["flux", "error", "zabs", "mask"]
    want = {"h": None, "hmean": None, "hcov": None, "n_samples": 0, "seed": 0, "offset": 0, "unc": None, "bins": None,
            "cont_min": 0.0, "pixel_range": None, "unit_weights": False, "stack": None, "zfac": None, "batch": None,
            "return_pixels": True}
    for k, d in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d, k
    assert list(inspect.signature(model.QFA.mean_transmission).parameters)[1:8] == [
        "dataloader", "z_min", "z_max", "n_bins", "n_samples", "seed", "batch_size"]
    assert inspect.signature(model.QFA.predict_to_npz).parameters["forest"].default is False


def test_forest_stack_arithmetic():
    import torch
    from qfa_amd.model import ForestStack
    from qfa_amd._lib import QFAHipError
    buf = torch.tensor([[[2.0, 4.0, 0.0], [1.0, 1.0, 0.0], [0.75, 0.5, 0.0], [3.0, 5.0, 0.0]],
                        [[2.0, 4.0, 0.0], [1.5, 3.0, 0.0], [1.25, 2.5, 0.0], [3.0, 5.0, 0.0]]], dtype=torch.float64)
    st = ForestStack(buf, 2.0, 0.5, 3)
    assert st.S == 2 and st.bins == (2.0, 0.5, 3)
    assert st.z_centers.tolist() == [2.25, 2.75, 3.25] and st.z_edges.tolist() == [2.0, 2.5, 3.0, 3.5]
    assert st.mean[:, :2].tolist() == [[0.5, 0.25], [0.75, 0.75]] and torch.isnan(st.mean[:, 2]).all()
    assert st.var[:, :2].tolist() == [[0.375 - 0.25, 0.125 - 0.0625], [0.625 - 0.5625, 0.625 - 0.5625]]
    assert st.n.tolist() == [[3.0, 5.0, 0.0], [3.0, 5.0, 0.0]]
    assert torch.equal(st.tau_eff[:, :2], -torch.log(st.mean[:, :2]))
    assert st.mean_over_draws[:2].tolist() == [0.625, 0.5]
    assert np.allclose(st.std_over_draws[:2].numpy(), [0.25 / np.sqrt(2.0), 0.5 / np.sqrt(2.0)])
    twice = st.clone().add_(st)
    assert torch.equal(twice.buf, 2 * buf) and torch.equal(twice.mean[:, :2], st.mean[:, :2]) and torch.equal(st.buf, buf)
    one = ForestStack(buf[:1].contiguous(), 2.0, 0.5, 3)
    with pytest.raises(QFAHipError):
        one.std_over_draws
    with pytest.raises(QFAHipError):
        one.add_(st)
    with pytest.raises(QFAHipError):
        st.add_(ForestStack(buf.clone(), 2.0, 0.25, 3))
    for bad in (buf.float(), buf[:, :3].contiguous(), buf[0]):
        with pytest.raises(QFAHipError):
            ForestStack(bad, 2.0, 0.5, 3)
    with pytest.raises(QFAHipError):
        ForestStack(buf, 2.0, 0.0, 3)
    assert ForestStack.zeros(4, 2.0, 0.1, 7, "cpu").buf.shape == (4, 4, 7)
    assert ForestStack.zeros(1, 2.0, 0.1, 7, "cpu").dz == float(np.float32(0.1))       # the float32 the kernel bins with


def test_port_on_three_pixels_worked_by_hand():
    """F = [[1], [0], [-1]], mu = [1, 2, 1], h = 0.5: c = [1.5, 2, 0.5].  flux = [0.75, 1, 0.25], sigma = [0.25, 0.5, 0.125], unc =
    [0.5, 0, 1]: T = [0.5, 0.5, 0.5]; den = [0.25 0.25 + 0.0625, 0.25, 0.25 1 + 0.015625] = [0.125, 0.25, 0.265625];
    iv = [2.25 / 0.125, 4 / 0.25, 0.25 / 0.265625] = [18, 16, 16 / 17].  z = [2.0, 2.25, 2.75] in bins of 0.5 from 2.0: k = [0, 0, 1]."""
    F = np.array([[1.0], [0.0], [-1.0]], np.float32)
    mu = np.array([1.0, 2.0, 1.0], np.float32)
    flux = np.array([[0.75, 1.0, 0.25]], np.float32)
    err = np.array([[0.25, 0.5, 0.125]], np.float32)
    unc = np.array([[0.5, 0.0, 1.0]], np.float32)
    z = np.array([[2.0, 2.25, 2.75]], np.float32)
    h = np.full((1, 1, 1), 0.5, np.float32)
    r = R.forest(F, mu, flux, err, z, None, h, unc, (2.0, 0.5, 2), 0.0)
    assert r["c"].tolist() == [[[1.5, 2.0, 0.5]]] and r["cabs"].tolist() == [[[1.5, 2.0, 1.5]]]
    assert r["T"].tolist() == [[[0.5, 0.5, 0.5]]] and r["iv"].tolist() == [[[18.0, 16.0, 16.0 / 17.0]]]
    assert r["use"].all() and r["k"].tolist() == [[0, 0, 1]]
    assert r["stack"].tolist() == [[[34.0, 16.0 / 17.0], [17.0, 8.0 / 17.0], [8.5, 4.0 / 17.0], [2.0, 1.0]]]
    # cont_min excludes by c > cont_min, the mask by a select; an excluded pixel is exactly 0 / 0 and leaves the stack
    r = R.forest(F, mu, flux, err, z, np.array([[True, False, True]]), h, unc, (2.0, 0.5, 2), 0.5)
    assert r["use"].tolist() == [[[True, False, False]]] and r["T"].tolist() == [[[0.5, 0.0, 0.0]]]
    assert r["stack"].tolist() == [[[18.0, 0.0], [9.0, 0.0], [4.5, 0.0], [1.0, 0.0]]]
    # unit weights, a pixel range, and bins whose edges the redshifts sit on: [2.25, 2.5) holds z = 2.25, z = 2.75 is the top edge
    r = R.forest(F, mu, flux, err, z, None, h, unc, (2.25, 0.25, 2), 0.0, unit_w=True, pixel_range=(0, 2))
    assert r["k"].tolist() == [[-1, 0, -1]] and r["stack"].tolist() == [[[1.0, 0.0], [0.5, 0.0], [0.25, 0.0], [1.0, 0.0]]]
    assert R.bin_index(np.array([np.nan, 2.0, 1.9999999, 3.0, 2.9999998], np.float32), 2.0, 0.5, 2).tolist() == [-1, 0, -1, -1, 1]
    assert R.z_factored([4.0], [0.875])[0, 0] == np.float32(2.5)
    # a NaN in h touches its own (b, s) only; junk under the mask changes nothing
    h2 = np.array([[[0.5], [np.nan]]], np.float32)
    r2 = R.forest(F, mu, flux, err, z, None, h2, unc, (2.0, 0.5, 2), 0.0)
    assert r2["use"][0, 0].all() and not r2["use"][0, 1].any() and (r2["stack"][1] == 0).all()
