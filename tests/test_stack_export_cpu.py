"""What a stack class tells the rest of the Python side (qfa_amd/stacks.py), on CPU tensors: ``arrays()`` is what the command line
writes of it -- the key lists below are the files' as they were written before the stacks owned them -- and the static parameter check
refuses exactly what the C checks refuse (qfa_amd/csrc/qfa_p1d.hip), at the boundaries and not at their neighbours."""
import numpy as np
import pytest
import torch

from qfa_amd._lib import QFAHipError
from qfa_amd.stacks import ForestStack, P1DBandStack, P1DStack, PDFStack, VarianceStack, XiStack, _edges

NZ, L, DV = 2, 8, 69.0
Z = (2.0, 0.25, NZ)
EDGES = P1DBandStack.linear_k_edges(L, DV, 2)
MIN_COUNT = 3

# class -> (width of buf behind (S, nz), constructor arguments behind (buf, z0, dz, nz), keys for S = 1, keys added for S > 1,
# key -> the property or method it is documented to be)
STACKS = {
    ForestStack: (None, (), ["z_centers", "z_edges", "mean", "var", "n", "tau_eff", "sums"], [],
                  dict(z_centers=lambda s: s.z_centers, z_edges=lambda s: s.z_edges, mean=lambda s: s.mean, var=lambda s: s.var,
                       n=lambda s: s.n, tau_eff=lambda s: s.tau_eff, sums=lambda s: s.buf)),
    P1DStack: (2 + 2 * (L // 2), (L, DV),
               ["k", "z_centers", "z_edges", "power", "err", "power_raw", "noise", "n", "seg_len", "dv", "sums"], [],
               dict(k=lambda s: s.k, z_centers=lambda s: s.z_centers, z_edges=lambda s: s.z_edges, power=lambda s: s.power(),
                    err=lambda s: s.err(), power_raw=lambda s: s.power_raw, noise=lambda s: s.noise, n=lambda s: s.n, seg_len=lambda s: s.L,
                    dv=lambda s: s.dv, sums=lambda s: s.buf)),
    P1DBandStack: (1 + 2 + 4, (L, DV, EDGES), ["k_edges", "k_centers", "z_edges", "n", "mean", "cov"], ["cov_over_draws"],
                   dict(k_edges=lambda s: s.k_edges, k_centers=lambda s: s.k_centers, z_edges=lambda s: s.z_edges, n=lambda s: s.n,
                        mean=lambda s: s.mean, cov=lambda s: s.cov, cov_over_draws=lambda s: s.cov_over_draws)),
    XiStack: (2 + 5 * 3, (L, 3, DV),
              ["lags_kms", "z_centers", "z_edges", "xi", "xi_raw", "err", "n", "sum_w", "seg_len", "dv", "sums"], [],
              dict(lags_kms=lambda s: s.lags_kms, z_centers=lambda s: s.z_centers, z_edges=lambda s: s.z_edges, xi=lambda s: s.xi(),
                   xi_raw=lambda s: s.xi(subtract_noise=False), err=lambda s: s.err(), n=lambda s: s.n, sum_w=lambda s: s.sum_w,
                   seg_len=lambda s: s.L, dv=lambda s: s.dv, sums=lambda s: s.buf)),
    PDFStack: (2 + 3 + 9, (L, 0.0, 0.4, 3, False, True),
               ["z", "t_edges", "pdf", "err", "cov", "counts", "n_segments", "out_of_range"], ["std_over_draws", "total_cov"],
               dict(z=lambda s: s.z_centers, t_edges=lambda s: s.t_edges, pdf=lambda s: s.pdf(), err=lambda s: s.err(), cov=lambda s: s.cov(),
                    counts=lambda s: s.counts, n_segments=lambda s: s.n_segments, out_of_range=lambda s: s.out_of_range(),
                    std_over_draws=lambda s: s.std_over_draws, total_cov=lambda s: s.total_cov)),
    VarianceStack: (2 + 5 * 4, (L, -3, 2, 1),
                    ["z", "z_edges", "v_edges", "v_mean", "var_delta", "var_err", "mean_delta", "counts", "n_segments", "n_pixels",
                     "out_of_range", "seg_len", "sums", "eta", "sigma2_lss", "cov", "chi2", "ndof", "n_bins"],
                    ["eta_std_over_draws", "sigma2_lss_std_over_draws"],
                    dict(z=lambda s: s.z_centers, z_edges=lambda s: s.z_edges, v_edges=lambda s: s.v_edges, v_mean=lambda s: s.v_mean,
                         var_delta=lambda s: s.var_delta, var_err=lambda s: s.var_err, mean_delta=lambda s: s.mean_delta,
                         counts=lambda s: s.counts, n_segments=lambda s: s.n_segments, n_pixels=lambda s: s.n_pixels,
                         out_of_range=lambda s: s.out_of_range(), seg_len=lambda s: s.L, sums=lambda s: s.buf,
                         eta=lambda s: s.fit(min_count=MIN_COUNT).eta, sigma2_lss=lambda s: s.fit(min_count=MIN_COUNT).sigma2_lss,
                         cov=lambda s: s.fit(min_count=MIN_COUNT).cov, chi2=lambda s: s.fit(min_count=MIN_COUNT).chi2,
                         ndof=lambda s: s.fit(min_count=MIN_COUNT).ndof, n_bins=lambda s: s.fit(min_count=MIN_COUNT).n_bins,
                         eta_std_over_draws=lambda s: s.std_over_draws(min_count=MIN_COUNT)[0],
                         sigma2_lss_std_over_draws=lambda s: s.std_over_draws(min_count=MIN_COUNT)[1])),
}


def filled(cls, S):
    """a stack of ``cls`` on a seeded integer-valued buffer: every count >= 2 but the one of draw 0, z-bin 1, which is 1"""
    width, args = STACKS[cls][:2]
    shape = (S, 4, NZ) if cls is ForestStack else (S, NZ, width)
    buf = torch.tensor(np.random.default_rng(7 + S).integers(2, 40, shape).astype(np.float64))
    if cls is ForestStack:
        buf[0, 3, 1] = 1.0
    else:
        buf[0, 1, 0] = 1.0
    return cls(buf, *Z, *args)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("cls", list(STACKS), ids=lambda c: c.__name__)
def test_arrays_is_what_the_command_line_wrote(cls, S):
    st = filled(cls, S)
    _, _, keys, over, doc = STACKS[cls]
    got = st.arrays(min_count=MIN_COUNT) if cls is VarianceStack else st.arrays()
    assert list(got) == keys + (over if S > 1 else [])
    for k, v in got.items():
        want = doc[k](st)
        if isinstance(want, torch.Tensor):
            assert isinstance(v, np.ndarray) and v.dtype == np.float64 and np.array_equal(v, want.numpy(), equal_nan=True), k
        else:
            assert type(v) is type(want) and v == want, k
    # the error bars are there where two segments are and NaN where one is (a stack whose every cell is NaN would pass the above)
    bar = {P1DStack: "err", XiStack: "err", P1DBandStack: "cov", PDFStack: "cov"}.get(cls)
    if bar is not None:
        assert np.isnan(got[bar][0, 1]).all() and np.isfinite(got[bar][0, 0]).all(), bar


def test_variance_arrays_default_min_count_is_fit_s():
    st = filled(VarianceStack, 1)
    assert np.array_equal(st.arrays()["n_bins"], st.fit().n_bins.numpy()) and (st.arrays()["n_bins"] == 0).all()   # (counts < 100)
    assert (st.arrays(min_count=MIN_COUNT)["n_bins"] > 0).any()


def refused(check, *args, **kw):
    try:
        check(*args, **kw)
    except QFAHipError:
        return True
    return False


def test_flux_params_at_the_boundaries():
    nan, inf = float("nan"), float("inf")
    assert [refused(PDFStack.flux_params, 0.0, 0.1, nt) for nt in (0, 1, 64, 65)] == [True, False, False, True]
    assert [refused(PDFStack.flux_params, 0.0, dt, 10) for dt in (0.0, nan, inf, -0.1, 1e-3, 1e-46)] == [True, True, True, True, False, True]
    assert [refused(PDFStack.flux_params, t0, 0.1, 10) for t0 in (nan, -inf, 1e39, -5.0)] == [True, True, True, False]
    assert [refused(PDFStack.flux_params, 0.0, 0.1, 10, ivar_min=x) for x in (-1e-3, inf, nan, 0.0, 2.5)] == [True, True, True, False, False]
    # what comes back is what the kernel reads: float32 numbers, plain bools
    assert PDFStack.flux_params(0.1, 0.1, 7, 1, 0, 0.3) == (float(np.float32(0.1)), float(np.float32(0.1)), 7, True, False, float(np.float32(0.3)))
    for bad in (dict(n_tbins=65), dict(dt=0.0), dict(ivar_min=-1.0)):
        kw = {**dict(t0=0.0, dt=0.1, n_tbins=3, ivar_min=0.0), **bad}
        assert refused(PDFStack.zeros, 1, *Z, L, **kw)
        assert refused(PDFStack, torch.zeros((1, NZ, 14), dtype=torch.float64), *Z, L, **kw)
    assert refused(PDFStack.zeros, 1, *Z, 0, 0.0, 0.1, 3) and refused(PDFStack.zeros, 1, *Z, 4097, 0.0, 0.1, 3)


def test_var_params_at_the_boundaries():
    V = VarianceStack.var_params
    assert [refused(V, -8, 1, sub) for sub in (-1, 0, 4, 5)] == [True, False, False, True]
    assert [refused(V, -8, n_oct, sub) for n_oct, sub in ((64, 0), (65, 0), (4, 4), (5, 4), (0, 1), (-1, 1))] == \
        [False, True, False, True, True, True]                                       # n_oct << sub = 64, 65, 64, 80; n_oct < 1
    assert [refused(V, e_lo, 8, 1) for e_lo in (-127, -126, 119, 120)] == [True, False, False, True]   # e_lo + n_oct = 127, 128
    assert [refused(V, -8, 8, 1, d) for d in (0.0, -1.0, float("nan"), 1e-30, 1e39)] == [True, True, True, False, False]
    assert V(-8, 8, 1, 1e39)[3] == float("inf")                                      # (as the C check: d_max > 0 is all it asks)
    assert V(-8, 8, 1) == (-8, 8, 1, VarianceStack.FLT_MAX) and V(-8, 8, 1, 0.35) == (-8, 8, 1, float(np.float32(0.35)))
    st = VarianceStack.zeros(2, *Z, L, -8, 8, 1, 0.35)
    assert st.var_bins == V(-8, 8, 1, 0.35) and st.buf.shape == (2, NZ, 2 + 5 * 16)
    assert refused(VarianceStack.zeros, 1, *Z, L, -8, 33) and refused(VarianceStack.zeros, 1, *Z, L, -8, 8, 5)


def test_lag_params_at_the_boundaries():
    assert [refused(XiStack.lag_params, L, n) for n in (0, 1, L, L + 1)] == [True, False, False, True]
    assert XiStack.lag_params(L, np.int64(3)) == 3 and type(XiStack.lag_params(L, np.int64(3))) is int
    assert refused(XiStack.zeros, 1, *Z, L, L + 1, DV, "cpu") and XiStack.zeros(1, *Z, L, L, DV, "cpu").nlag == L
    assert refused(XiStack, torch.zeros((1, NZ, 2), dtype=torch.float64), *Z, L, 0, DV)


def test_band_edges_at_the_boundaries():
    up = lambda n: np.arange(1.0, n + 1.0)
    assert [refused(_edges, up(n)) for n in (1, 2, 65, 66)] == [True, False, False, True]
    assert refused(_edges, [1.0, 1.0]) and refused(_edges, [2.0, 1.0]) and refused(_edges, [1.0, float("nan")])
    assert refused(_edges, [1.0, float("inf")]) and _edges([1, 2.5]) == (1.0, 2.5)
    assert refused(P1DBandStack.zeros, 1, *Z, L, DV, up(66), "cpu") and P1DBandStack.zeros(1, *Z, L, DV, up(65), "cpu").nband == 64
