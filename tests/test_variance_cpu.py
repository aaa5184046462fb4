"""The variance function without a GPU: the bin rule on bits (tests/_variance_ref.py and VarianceStack.v_edges), the boundary (header,
exports, size functions, argument checks), VarianceStack's closed-form fit on CPU tensors -- exactness on a hand-built stack and
recovery of (eta, sigma2_lss) from Gaussian pixels pushed through the port -- its algebra, and the config keys and command line."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _variance_ref as R
from conftest import REPO

NAMES = ("qfa_variance_stack_doubles", "qfa_variance_workspace_bytes", "qfa_variance_f32")
f32 = np.float32


def _bin_by_edges(v, edges):
    """the bin of v by comparison with the exact float64 edges: edge c <= v < edge c + 1, else -1"""
    v = np.asarray(v, np.float64)
    k = np.searchsorted(edges, v, side="right") - 1
    with np.errstate(invalid="ignore"):
        return np.where((v >= edges[0]) & (v < edges[-1]), k, -1)


@pytest.mark.parametrize("e_lo,n_oct,sub", [(-10, 12, 1), (-3, 1, 0), (-2, 4, 4), (-126, 2, 2), (125, 2, 0), (0, 64, 0), (-6, 7, 3)])
def test_bin_rule_on_bits(e_lo, n_oct, sub):
    import torch
    from qfa_amd.model import VarianceStack
    nv = n_oct << sub
    st = VarianceStack.zeros(1, 0.0, 1.0, 1, 8, e_lo, n_oct, sub)
    edges = st.v_edges.numpy()
    assert st.nv == nv and edges.shape == (nv + 1,) and np.array_equal(edges, R.v_edges(e_lo, n_oct, sub))
    assert edges[0] == 2.0 ** e_lo and edges[-1] == 2.0 ** (e_lo + n_oct) and (np.diff(edges) > 0).all()
    e32 = edges.astype(f32)
    assert np.array_equal(e32.astype(np.float64), edges)                               # every edge is a float32
    # every edge -- the powers of two among them -- and its float32 neighbours on both sides
    below, above = np.nextafter(e32, f32(0.0)), np.nextafter(e32, f32(np.inf))
    code = lambda v: np.where((R.v_code(v, e_lo, sub) >= 0) & (R.v_code(v, e_lo, sub) < nv), R.v_code(v, e_lo, sub), -1)
    assert np.array_equal(code(e32), np.append(np.arange(nv), -1))                     # an edge belongs to the bin above it
    assert np.array_equal(code(above), np.append(np.arange(nv), -1))
    assert np.array_equal(code(below), np.arange(-1, nv))
    # a dense sample across and beyond the range against the comparison with the edges
    rng = np.random.default_rng(5)
    v = np.exp2(rng.uniform(max(e_lo - 2, -126), min(e_lo + n_oct + 2, 127), 4000)).astype(f32)
    assert np.array_equal(code(v), _bin_by_edges(v, edges))
    # zero, denormals, inf, NaN and negative values fall in no bin
    tiny = np.finfo(f32).tiny
    junk = np.array([0.0, -0.0, tiny / 2, np.nextafter(f32(tiny), f32(0.0)), 1e-45, np.inf, -np.inf, np.nan, -1.0, -2.0 ** e_lo,
                     -np.float32(edges[1])], f32)
    with np.errstate(all="ignore"):
        assert (code(junk) == -1).all()


def test_boundary_declares_and_exports_the_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_var_t" in txt and "#define QFA_ABI_VERSION 4" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert [f[0] for f in _lib.VarParams._fields_] == ["e_lo", "n_oct", "sub", "d_max"] and C.sizeof(_lib.VarParams) == 16
    assert _lib.lib().qfa_abi_version() == 4


def test_size_functions():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_variance_stack_doubles(3, 7, 5) == 3 * 7 * (2 + 25) and h.qfa_variance_stack_doubles(1, 4096, 64) == 4096 * 322
    for a in ((0, 7, 5), (3, 0, 5), (3, 4097, 5), (3, 7, 0), (3, 7, 65), (3, 7, -1)):
        assert h.qfa_variance_stack_doubles(*a) == 0, a
    ok = (12, 3, 100, 37, 2, 7, 20)                                                # R = B S, S, Nb, L, nseg, nz, nv
    rows = 12 * 2 * (4 + 8 * 101)                                                  # code and [n_used | 5 nv] of every segment
    part = 3 * 7 * 102 * 8                                                         # one chunk's partials per (draw, z-bin)
    assert rows + part <= h.qfa_variance_workspace_bytes(*ok) <= rows + part + 32
    for i, bad in ((0, -3), (0, 13), (1, 0), (2, 73), (3, 0), (3, 4097), (3, 51), (4, 0), (4, 3), (5, 0), (5, 4097), (6, 0), (6, 65)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_variance_workspace_bytes(*a) == 0, a
    assert h.qfa_variance_workspace_bytes(12, 3, 100, 37, 2, 7, 64) > 0 and h.qfa_variance_workspace_bytes(12, 3, 100, 37, 2, 7, 1) > 0
    assert h.qfa_variance_workspace_bytes(0, 1, 1, 1, 1, 1, 1) > 0                   # B = 0 is a shape the call accepts
    assert h.qfa_variance_workspace_bytes(4096 * 100, 100, 720, 240, 3, 8, 28) < (80 << 20)


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=3, Nb=40, prm=None, var=None, flags=0, ws_bytes=None, null=(), batch=None, outs="ms"):
        bs = _lib.Batch()
        bs.zabs = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        d = dict(zT0=2.0, dzT=0.1, nT=5, St=1, p_lo=1, seg_len=13, nseg=3, min_used=2, z0=2.0, dz=0.25, nz=4)
        d.update(prm or {})
        pp = _lib.P1DParams(**d)
        q = dict(e_lo=-10, n_oct=10, sub=1, d_max=R.FLT_MAX)
        q.update(var or {})
        qq = _lib.VarParams(**q)
        need = h.qfa_variance_workspace_bytes(2 * 3, 3, 40, 13, 3, 4, 20)
        a = lambda name, v: None if name in null else v
        return h.qfa_variance_f32(a("trans", P), a("ivar", P), a("b", C.byref(bs)), a("tbar", P), B, S, Nb, a("p", C.byref(pp)),
                                  a("q", C.byref(qq)), flags, P if "m" in outs else None, P if "s" in outs else None,
                                  a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("trans", "ivar", "b", "tbar", "p", "q", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1 and call(batch={"zabs": None}) == -1
    assert call(batch={"zabs": None, "zq1": 4096}) == -1 and call(batch={"pix_ratio": 4096}) == -1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(S=0), dict(Nb=0), dict(prm={"seg_len": 0}), dict(prm={"seg_len": 4097}), dict(prm={"nseg": 0}),
               dict(prm={"p_lo": -1}), dict(prm={"p_lo": 2}), dict(prm={"nseg": 4}), dict(Nb=39), dict(prm={"min_used": 0}),
               dict(prm={"dz": 0.0}), dict(prm={"dz": nan}), dict(prm={"z0": inf}), dict(prm={"nz": 0}), dict(prm={"nz": 4097}),
               dict(prm={"dzT": 0.0}), dict(prm={"zT0": inf}), dict(prm={"nT": 0}), dict(prm={"St": 2}), dict(batch={"row_stride": 39}),
               dict(var={"n_oct": 0}), dict(var={"n_oct": -1}), dict(var={"n_oct": 33}), dict(var={"n_oct": 65, "sub": 0}),
               dict(var={"sub": -1}), dict(var={"sub": 5}), dict(var={"n_oct": 5, "sub": 4}), dict(var={"e_lo": -127}),
               dict(var={"e_lo": 118}), dict(var={"e_lo": 127, "n_oct": 1}), dict(var={"d_max": 0.0}), dict(var={"d_max": -1.0}),
               dict(var={"d_max": nan}), dict(var={"n_oct": 1 << 30, "sub": 2})):
        assert call(**kw) == -2, kw
    # the accepted values of the same arguments, on a call with nothing to do (B = 0: no device work is reached)
    assert call(B=0, prm={"St": 3}) == 0 and call(B=0, var={"n_oct": 4, "sub": 4}, ws_bytes=1 << 30) == 0
    assert call(B=0, var={"n_oct": 1, "sub": 0}) == 0 and call(B=0, var={"e_lo": -126}) == 0 and call(B=0, var={"e_lo": 117}) == 0
    assert call(B=0, var={"d_max": inf}) == 0 and call(B=0, var={"d_max": 1e-30}) == 0 and call(B=0, var={"n_oct": 64, "sub": 0, "e_lo": 0}, ws_bytes=1 << 30) == 0
    for outs in ("m", "s"):
        assert call(B=0, outs=outs) == 0, outs
    assert call(B=0, flags=0x80, outs="m") == 0 and call(B=0, flags=0x20) == 0 and call(B=0, flags=0xa0, outs="m") == 0
    for flags in (0x1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x80 | 0x8, 0x2000):
        assert call(flags=flags) == -5, flags
    need = h.qfa_variance_workspace_bytes(6, 3, 40, 13, 3, 4, 20)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3


def _hand_stack(x, y, e, n, e_lo, n_oct, sub):
    """a (1, 1) VarianceStack whose bins hold v_mean = x, var_delta = y (mean_delta = 0), var_err = e and n pixels each"""
    import torch
    from qfa_amd.model import VarianceStack
    nv = n_oct << sub
    st = VarianceStack.zeros(1, 0.0, 1.0, 1, 8, e_lo, n_oct, sub)
    buf = np.zeros(2 + 5 * nv)
    buf[0], buf[1] = 10.0, n.sum()
    buf[2:2 + nv], buf[2 + nv:2 + 2 * nv], buf[2 + 3 * nv:2 + 4 * nv] = n, n * x, n * y
    buf[2 + 4 * nv:] = n * (y * y + n * e * e)
    st.buf[0, 0] = torch.tensor(buf)
    return st


@pytest.mark.parametrize("epsilon", [False, True])
def test_fit_is_exact_on_a_hand_built_stack(epsilon):
    """var_delta = eta v + sigma2 (+ eps / v) exactly: the parameters come back within 64 x 2^-52 x cond(N) of the truth, relative to
    the parameter vector's norm -- N the weighted normal matrix as this test forms it from the stack's own v_mean and var_err; the
    stack carries y within a few ulp (sums of n y divided by n), which a solve amplifies by cond(N) at the most"""
    e_lo, n_oct, sub = -8, 8, 1
    nv = n_oct << sub
    edges = R.v_edges(e_lo, n_oct, sub)
    x = 0.5 * (edges[:-1] + edges[1:])
    eta, s2, eps = 1.25, 0.0625, 3e-4
    y = eta * x + s2 + (eps / x if epsilon else 0.0)
    e = 0.01 * y
    n = np.full(nv, 1000.0)
    n[3], n[7] = 99.0, 10.0                                                          # below min_count: left out
    st = _hand_stack(x, y, e, n, e_lo, n_oct, sub)
    ft = st.fit(min_count=100, epsilon=epsilon)
    use = n >= 100
    cols = [x[use], np.ones(use.sum())] + ([1.0 / x[use]] if epsilon else [])
    A = np.stack(cols, -1) / e[use, None]
    cond = np.linalg.cond(A.T @ A)
    truth = np.array([eta, s2] + ([eps] if epsilon else []))
    got = np.array([ft.eta[0, 0].item(), ft.sigma2_lss[0, 0].item()] + ([ft.eps[0, 0].item()] if epsilon else []))
    bar = 64.0 * 2.0 ** -52 * cond * np.linalg.norm(truth)
    print(f"epsilon {epsilon}: cond(N) = {cond:.3g}, max |dp| = {np.abs(got - truth).max():.3g}, bar = {bar:.3g}")
    assert (np.abs(got - truth) <= bar).all()
    P = len(truth)
    assert (ft.eps is None) == (not epsilon) and ft.n_bins[0, 0].item() == nv - 2 and ft.ndof[0, 0].item() == nv - 2 - P
    assert 0.0 <= ft.chi2[0, 0].item() < 1e-18
    cov = ft.cov[0, 0].numpy()
    want = np.linalg.inv(A.T @ A)
    assert cov.shape == (P, P) and np.allclose(cov, want, rtol=1e-6 * cond ** 0.5, atol=0.0) and np.array_equal(cov, cov.T)


def test_fit_cells_without_enough_bins_are_nan():
    import torch
    e_lo, n_oct, sub = -4, 4, 0
    x = 1.5 * R.v_edges(e_lo, n_oct, sub)[:-1]
    y = 1.1 * x + 0.05
    for n, eps, fine in ((np.array([500.0, 500, 500, 500]), False, True), (np.array([500.0, 500, 99, 99]), False, True),
                         (np.array([500.0, 99, 99, 99]), False, False), (np.array([500.0, 500, 99, 99]), True, False),
                         (np.array([0.0, 0, 0, 0]), False, False), (np.array([500.0, 500, 500, 99]), True, True)):
        st = _hand_stack(x, y, 0.02 * y, n, e_lo, n_oct, sub)
        ft = st.fit(min_count=100, epsilon=eps)
        vals = [ft.eta, ft.sigma2_lss, ft.chi2, ft.cov] + ([ft.eps] if eps else [])
        assert all(bool(torch.isfinite(t).all()) == fine for t in vals), (n, eps)
        assert ft.n_bins[0, 0].item() == (n >= 100).sum()
    # var_err = 0 leaves a bin out as well
    st = _hand_stack(x, y, np.array([0.0, 0.0, 0.0, 0.01]), np.full(4, 500.0), e_lo, n_oct, sub)
    assert st.fit().n_bins[0, 0].item() == 1 and torch.isnan(st.fit().eta).all()


def test_recovery_of_eta_and_sigma2_through_the_port():
    """Gaussian delta_F with var = eta v + sigma2_lss, v log-uniform on [2e-3, 2], 11 520 pixels through the port and fit(): within 4
    of the fit's own sigmas of the truth"""
    import torch
    from qfa_amd.model import VarianceStack
    eta, s2 = 1.2, 0.08
    B, Nb, L, nseg = 16, 720, 240, 3
    rng = np.random.default_rng(20261)
    ivar = (1.0 / np.exp(rng.uniform(np.log(2e-3), np.log(2.0), (B, 1, Nb)))).astype(f32)
    v = (f32(1.0) / ivar).astype(f32).astype(np.float64)                              # the port's v with tbar = 1
    trans = (1.0 + rng.standard_normal((B, 1, Nb)) * np.sqrt(eta * v + s2)).astype(f32)
    z = np.full((B, Nb), 2.25, f32)
    tbar, tb_bins, bins = np.ones((1, 4), f32), (2.0, 0.25, 4), (2.0, 0.5, 1)
    e_lo, n_oct, sub = -10, 12, 1
    ref = R.variance(trans, ivar, z, tbar, tb_bins, 0, L, nseg, 200, bins, e_lo, n_oct, sub)
    assert ref["valid"].all() and ref["stack"][0, 0, 0] == B * nseg and ref["stack"][0, 0, 1] == B * Nb
    st = VarianceStack(torch.tensor(ref["stack"]), *bins, L, e_lo, n_oct, sub)
    assert st.counts.sum().item() == B * Nb and st.out_of_range()[0, 0].item() == 0.0
    ft = st.fit(min_count=50)
    nb = int(ft.n_bins[0, 0].item())
    assert nb >= 10, nb
    cov = ft.cov[0, 0].numpy()
    dev = np.array([ft.eta[0, 0].item() - eta, ft.sigma2_lss[0, 0].item() - s2]) / np.sqrt(np.diag(cov))
    print(f"{nb} usable bins, deviations {dev[0]:+.2f} and {dev[1]:+.2f} sigma, chi2 {ft.chi2[0, 0].item():.1f} on {int(ft.ndof[0, 0].item())}")
    assert (np.abs(dev) <= 4.0).all()
    # the bins hold what their edges say
    vm = st.v_mean[0, 0].numpy()
    occ = st.counts[0, 0].numpy() > 0
    edges = st.v_edges.numpy()
    assert (vm[occ] >= edges[:-1][occ]).all() and (vm[occ] < edges[1:][occ]).all()


def test_stack_algebra():
    import torch
    from qfa_amd._lib import QFAHipError
    from qfa_amd.model import VarianceStack
    import qfa_amd
    assert qfa_amd.VarianceStack is VarianceStack
    mk = lambda **kw: VarianceStack.zeros(**{**dict(S=3, z0=2.0, dz=0.25, nz=4, L=20, e_lo=-8, n_oct=6, sub=1, d_max=None), **kw})
    a = mk()
    assert a.buf.shape == (3, 4, 2 + 5 * 12) and a.nv == 12 and a.S == 3 and a.L == 20 and a.d_max == R.FLT_MAX
    assert a.var_bins == (-8, 6, 1, R.FLT_MAX) and mk(d_max=0.1).d_max == float(f32(0.1))
    a.buf.copy_(torch.arange(a.buf.numel(), dtype=torch.float64).reshape(a.buf.shape))
    b = a.clone()
    assert b.same_layout(a) and torch.equal(b.add_(a).buf, 2 * a.buf)
    assert torch.equal(a.n_segments, a.buf[:, :, 0]) and torch.equal(a.n_pixels, a.buf[:, :, 1]) and torch.equal(a.counts, a.buf[:, :, 2:14])
    assert torch.equal(a.v_mean, a.buf[:, :, 14:26] / a.counts) and torch.equal(a.mean_delta, a.buf[:, :, 26:38] / a.counts)
    d = a.draws(1, 3)
    assert d.S == 2 and d.var_bins == a.var_bins and d.buf.data_ptr() == a.buf[1:].data_ptr()
    for other in (dict(S=2), dict(dz=0.5), dict(nz=3), dict(L=21), dict(e_lo=-7), dict(n_oct=3, sub=2), dict(d_max=2.0)):
        o = mk(**other)
        with pytest.raises(QFAHipError):
            a.add_(o)
        if "S" not in other:
            assert not a.same_layout(o), other
    for bad in (dict(n_oct=0), dict(n_oct=33), dict(sub=5), dict(sub=-1), dict(e_lo=-127), dict(e_lo=122), dict(d_max=0.0),
                dict(d_max=float("nan")), dict(L=0), dict(L=4097)):
        with pytest.raises(QFAHipError):
            mk(**bad)
    with pytest.raises(QFAHipError):
        VarianceStack.zeros(1, 2.0, 0.25, 4, 20, -8, 6).std_over_draws()
    e, s = a.std_over_draws(min_count=1)
    assert e.shape == s.shape == (4,)


def test_a_cpu_tensor_raises():
    import torch
    from qfa_amd import synthetic
    from qfa_amd._lib import QFAHipError
    from qfa_amd.model import QFA
    nb = 40
    with pytest.raises(QFAHipError):
        QFA(nb, 8, 2, torch.device("cpu"), model_params=synthetic.mock_parameters(nb + 8, nb, 2, seed=1)[0])
    m = object.__new__(QFA)                                   # (the statistics' own checks, without a device to build a model on)
    m.Nb, m.device, m._tau_callable, m.use_factored_z = nb, torch.device("cpu"), None, True
    tr = torch.ones((2, 1, nb))
    with pytest.raises(QFAHipError):
        m.variance_segments(tr, tr, zabs=torch.full((2, nb), 2.1), tbar=torch.ones(4), tbar_bins=(2.0, 0.1, 4), seg_len=20, n_segments=2,
                            min_used=10, e_lo=-8, n_oct=8, bins=(2.0, 0.1, 2))
    with pytest.raises(QFAHipError, match="n_oct"):
        m.variance_function(None, 2.0, 3.0, 2, n_oct=33)


def test_config_keys_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    from qfa_amd.cli import build_parser
    M = Cf.get_config().MODEL
    assert (M.VAR_NOCT, M.VAR_ELO, M.VAR_SUB, M.VAR_DMAX, M.VAR_MIN_COUNT) == (0, -12, 1, 0.0, 100)
    assert {"MODEL.VAR_NOCT", "MODEL.VAR_ELO", "MODEL.VAR_SUB", "MODEL.VAR_DMAX", "MODEL.VAR_MIN_COUNT"} <= set(Cf.EXTRA_KEYS)
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.VAR_NOCT", "10", "MODEL.VAR_ELO", "-9", "MODEL.VAR_SUB", "2",
                                      "MODEL.VAR_DMAX", "5", "MODEL.VAR_MIN_COUNT", "30"])
    got = Cf.get_config(args).MODEL
    assert (got.VAR_NOCT, got.VAR_ELO, got.VAR_SUB, got.VAR_DMAX, got.VAR_MIN_COUNT) == (10, -9, 2, 5.0, 30)
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(model.QFA.variance_segments)
    assert list(sig.parameters)[1:3] == ["trans", "ivar"]
    want = {"zabs": None, "zfac": None, "batch": None, "tbar": empty, "tbar_bins": None, "seg_len": empty, "n_segments": empty,
            "pixel_start": 0, "min_used": empty, "e_lo": empty, "n_oct": empty, "sub": 1, "d_max": None, "bins": None, "stack": None,
            "return_segments": False}
    assert list(sig.parameters)[3:] == list(want)
    for k, d in want.items():
        assert sig.parameters[k].kind is KW and sig.parameters[k].default == d, k
    sig = inspect.signature(model.QFA.variance_function)
    assert list(sig.parameters)[1:5] == ["dataloader", "z_min", "z_max", "n_zbins"]
    want = {"e_lo": -12, "n_oct": 14, "sub": 1, "d_max": None, "n_segments": 3, "seg_len": None, "min_used_frac": 0.75, "tbar": None,
            "tbar_nbins": 64, "n_samples": 0, "seed": 0, "batch_size": 4096, "cont_min": 0.0}
    assert list(sig.parameters)[5:] == list(want)
    for k, d in want.items():
        assert sig.parameters[k].kind is KW and sig.parameters[k].default == d, k
    assert "flux_correlation(sigma2_lss" in model.QFA.variance_function.__doc__


def test_cli_refuses_a_bad_variance_request_before_any_work(tmp_path):
    from qfa_amd import cli
    out = tmp_path / "out"
    base = ["--type", "predict", "--output_dir", str(out), "--catalog", str(tmp_path / "none.csv")]
    with pytest.raises(ValueError, match="VAR_NOCT.*P1D_SEGMENTS"):
        cli.main(base + ["--opts", "MODEL.VAR_NOCT", "8", "MODEL.FOREST_NBINS", "10"])
    opts = ["MODEL.FOREST_NBINS", "10", "MODEL.P1D_SEGMENTS", "2"]
    for bad in (["MODEL.VAR_NOCT", "33"], ["MODEL.VAR_NOCT", "-1"], ["MODEL.VAR_NOCT", "5", "MODEL.VAR_SUB", "4"]):
        with pytest.raises(ValueError, match="VAR_NOCT"):
            cli.main(base + ["--opts"] + opts + bad)
    for bad in ("5", "-1"):
        with pytest.raises(ValueError, match="VAR_SUB"):
            cli.main(base + ["--opts"] + opts + ["MODEL.VAR_NOCT", "2", "MODEL.VAR_SUB", bad])
    for bad in ("-127", "120"):
        with pytest.raises(ValueError, match="VAR_ELO"):
            cli.main(base + ["--opts"] + opts + ["MODEL.VAR_NOCT", "8", "MODEL.VAR_ELO", bad])
    with pytest.raises(ValueError, match="VAR_DMAX"):
        cli.main(base + ["--opts"] + opts + ["MODEL.VAR_NOCT", "8", "MODEL.VAR_DMAX", "-1.0"])
    with pytest.raises(ValueError, match="VAR_MIN_COUNT"):
        cli.main(base + ["--opts"] + opts + ["MODEL.VAR_NOCT", "8", "MODEL.VAR_MIN_COUNT", "0"])
    assert not out.exists()
