"""The pair-weighted line-of-sight correlation function of forest segments and its stack on the MI355X (QFA.xi / flux_correlation,
qfa_xi_f32) against the numpy port of the contract (tests/_xi_ref.py).

Bars (derived in tests/_xi_ref.py): per lag |dA_l| <= (L - l + 2) u sum_j |x_j x_{j+l}|, W_l the same with w, N0 (L + 3) u sum
|(w w) v|; the valid / invalid pattern is exact, the port working on the very trans / ivar the GPU read.  Stack: n 2^-53 sum |terms|
per entry against float64 sums of the GPU's own pairs / noise0, counts exact.  The inputs are those of tests/test_p1d.py: the
transmission and inverse variance QFA.forest writes for tests/test_forest.py's `geometry` (continuum in [0.5, 2], 20 % masks).

Achieved error / bar at the shapes of the first test: profiles/xi_accuracy.txt."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _p1d_ref as RP
import _xi_ref as R
from _segment_harness import (F_ZERO, TB_BINS, T, call_p1d, call_segment, case_shape, cli_predict_case, dev,  # noqa: F401 (dev: the fixture)
                              forest_case, loader_case, redshift_forms, refusals)

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
F_UNIT = 0x400


def call_x(dev, trans, ivar, tbar, prm, nlag, *, sigma2=0.0, **kw):
    """qfa_xi_f32 by hand on device tensors; prm = (p_lo, L, nseg, min_used, (z0, dz, nz)).  Returns pairs, noise0, stack (numpy)"""
    from qfa_amd import _lib
    nl = max(1, nlag)
    return call_segment("qfa_xi", dev, trans, ivar, tbar, prm, _lib.XiParams(nlag, sigma2), (("p", (2, nl), "float32"), ("n", (), "float32")),
                        size=(nlag,), stack_width=2 + 5 * nl, **kw)


def check_segments(pairs, noise0, ref, L, what):
    """every lag of every segment inside pair_bound, N0 inside noise0_bound, the valid pattern exact; returns the worst ratios"""
    valid = ref["valid"]
    W, A = pairs[:, :, :, 0].astype(np.float64), pairs[:, :, :, 1].astype(np.float64)
    assert np.array_equal(W[..., 0] != 0, valid), what                                 # (W_0 = sum w^2 > 0 on every valid segment)
    assert (pairs[~valid] == 0).all() and (noise0[~valid] == 0).all(), what
    eW, bW = np.abs(W - ref["W"]), R.pair_bound(ref["absW"], L)
    eA, bA = np.abs(A - ref["A"]), R.pair_bound(ref["absA"], L)
    eN, bN = np.abs(noise0.astype(np.float64) - ref["N0"]), R.noise0_bound(ref["absN0"], L)
    ratio = lambda e, b: float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    rs = (ratio(eW, bW), ratio(eA, bA), ratio(eN, bN))
    print(f"{what}: max |dW| / bar = {rs[0]:.3f}, max |dA| / bar = {rs[1]:.3f}, max |dN0| / bar = {rs[2]:.3f}")
    assert (eW <= bW).all(), (what, "W")
    assert (eA <= bA).all(), (what, "A")
    assert (eN <= bN).all(), (what, "N0")
    return rs


def check_stack(got, pairs, noise0, ref, nz, what):
    """against float64 sums of the GPU's own pairs / noise0 under the port's bins: n 2^-53 sum |terms|; counts exact"""
    own, own_abs = R.stack_of(pairs, noise0, ref["valid"], ref["kz"], nz)
    assert np.array_equal(got[:, :, 0], ref["stack"][:, :, 0]), (what, "counts")
    bar = got[:, :, :1] * U64 * own_abs
    err = np.abs(got - own)
    r = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{what}: max |d stack| / bar = {r:.3f}")
    assert (err <= bar).all(), (what, err.max())
    return r


CASES = [(1, 1, 1, 0, 1), (3, 2, 2, 1, 2), (17, 37, 3, 5, 37), (33, 64, 2, 0, 17), (16, 240, 3, 0, 120), (5, 667, 1, 3, 256),
         (4, 130, 1, 0, 63), (4, 130, 1, 0, 64), (4, 130, 1, 0, 65), (2, 4096, 1, 0, 5)]
BINS = (1.6, 0.45, 4)


@pytest.mark.parametrize("rows,L,nseg,p_lo,nlag", CASES)
def test_every_lag_of_every_segment_matches_the_port(dev, rows, L, nseg, p_lo, nlag):
    B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=seed)
    prm = (p_lo, L, nseg, min_used, BINS)
    trn, ivn = tr.cpu().numpy(), iv.cpu().numpy()
    for sigma2, unit in itertools.product((0.0, 0.1), (False, True)):
        ref = R.xi(trn, ivn, g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, BINS, nlag, sigma2, unit)
        pairs, noise0, stack = call_x(dev, tr, iv, tbar, prm, nlag, sigma2=sigma2, zabs=T(g["zabs"], dev),
                                      flags=F_ZERO | (F_UNIT if unit else 0))
        what = f"rows {rows} (B {B} S {S}) L {L} nseg {nseg} p_lo {p_lo} nlag {nlag} sigma2 {sigma2} unit {unit}"
        if L >= 37:
            assert ref["valid"].any() and (rows < 16 or not ref["valid"].all()), what
        check_segments(pairs, noise0, ref, L, what)
        check_stack(stack, pairs, noise0, ref, BINS[2], what)


@pytest.mark.parametrize("L", [37, 240])
def test_autocorrelation_identity_against_p1d(dev, L):
    """unit weights, no mask, nlag = L: L P_m = A_0 + 2 sum_{l >= 1} A_l cos(2 pi l m / L) for every mode of the shipped qfa_p1d_f32 --
    exact for the aperiodic autocorrelation; the cosine sum in float64 from the GPU's pairs"""
    rng = np.random.default_rng(70 + L)
    B, nseg, p_lo = 6, 2, 3
    nb = p_lo + nseg * L + 2
    trans = rng.uniform(0.2, 1.2, (B, 1, nb)).astype(np.float32)
    ivar = rng.uniform(10.0, 100.0, (B, 1, nb)).astype(np.float32)
    z = (rng.uniform(1.7, 2.0, (B, 1)) + np.linspace(0.0, 1.2, nb)[None, :]).astype(np.float32)
    tbar = rng.uniform(0.3, 0.9, (1, TB_BINS[2])).astype(np.float32)
    prm = (p_lo, L, nseg, L, BINS)
    tr, iv, zd = T(trans, dev), T(ivar, dev), T(z, dev)
    power, _, _ = call_p1d(dev, tr, iv, tbar, prm, zabs=zd)
    pairs, _, _ = call_x(dev, tr, iv, tbar, prm, L, zabs=zd, flags=F_ZERO | F_UNIT)
    rp = RP.p1d(trans, ivar, z, tbar, TB_BINS, p_lo, L, nseg, L, BINS)
    rx = R.xi(trans, ivar, z, tbar, TB_BINS, p_lo, L, nseg, L, BINS, L, 0.0, True)
    assert rp["valid"].all() and rx["valid"].all() and (pairs[:, :, :, 0, 0] == L).all()
    A = pairs[:, :, :, 1].astype(np.float64)                                           # (B, 1, nseg, L)
    l, mm = np.arange(1, L), np.arange(1, L // 2 + 1)
    cosm = np.cos(2.0 * np.pi * ((l[:, None] * mm[None, :]) % L) / L)                  # (L - 1, M)
    from_xi = (A[..., :1] + 2.0 * A[..., 1:] @ cosm) / L
    barA = R.pair_bound(rx["absA"], L)
    bar = RP.power_bound(rp, L) + (barA[..., :1] + 2.0 * barA[..., 1:].sum(-1, keepdims=True)) / L
    err = np.abs(power.astype(np.float64) - from_xi)
    print(f"L {L}: max |L P - autocorrelation| / bar = {(err / bar).max():.3f}")
    assert (err <= bar).all(), (err / bar).max()


def test_redshift_forms_give_identical_bits(dev):
    """zabs, the factored pair and the resident `rows` form on identical z: identical pairs, noise0 and stack"""
    B, S, nb, L, nseg, p_lo, nlag = 9, 2, 80, 37, 2, 4, 20
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=21)
    prm = (p_lo, L, nseg, 25, BINS)
    a, *others = (call_x(dev, tr, iv, tbar, prm, nlag, **kw) for kw in redshift_forms(dev, g, B, nb)[1])
    assert a[2][:, :, 0].sum() > 0
    for other in others:
        for x, y in zip(a, other):
            assert np.array_equal(x, y)


def test_repeats_draws_accumulation_and_null_outputs(dev):
    """two calls give the same bits; draw s of an S = 3 call is the call on that draw alone; ADD against QFA_F_ZERO_ACCUM; every
    subset of NULL outputs leaves the bits of the others.  More segments per draw than one chunk holds"""
    import torch
    B, S, nb, L, nseg, nlag = 50, 3, 64, 21, 3, 13
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=41)
    prm = (0, L, nseg, 15, BINS)
    z = T(g["zabs"], dev)
    ref = R.xi(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, 0, L, nseg, 15, BINS, nlag, 0.1)
    pairs, noise0, stack = call_x(dev, tr, iv, tbar, prm, nlag, sigma2=0.1, zabs=z)
    assert ref["stack"][:, :, 0].sum() > 64 * S and B * nseg > 2 * 64
    check_stack(stack, pairs, noise0, ref, BINS[2], "stack")
    again = call_x(dev, tr, iv, tbar, prm, nlag, sigma2=0.1, zabs=z)
    assert all(np.array_equal(x, y) for x, y in zip((pairs, noise0, stack), again))
    for s in range(S):
        one = call_x(dev, tr[:, s:s + 1].contiguous(), iv[:, s:s + 1].contiguous(), tbar[s:s + 1], prm, nlag, sigma2=0.1, zabs=z)
        assert np.array_equal(one[0][:, 0], pairs[:, s]) and np.array_equal(one[1][:, 0], noise0[:, s])
        assert np.array_equal(one[2][0], stack[s]), s
    full = {"p": pairs, "n": noise0, "s": stack}
    for outs in ("p", "n", "s", "pn", "ps", "ns"):
        got = dict(zip("pns", call_x(dev, tr, iv, tbar, prm, nlag, sigma2=0.1, zabs=z, outs=outs)))
        for k in "pns":
            assert (got[k] is None) == (k not in outs) and (k not in outs or np.array_equal(got[k], full[k])), (outs, k)
    # ADD: onto a stack that holds `stack` already -- the chunk partials are added onto it in chunk order
    acc = torch.tensor(stack, device=dev)
    added = call_x(dev, tr, iv, tbar, prm, nlag, sigma2=0.1, zabs=z, flags=0, stack=acc)[2]
    assert np.array_equal(added[:, :, 0], 2 * stack[:, :, 0])
    n = stack[:, :, :1]
    assert (np.abs(added - 2 * stack) <= 2 * n * U64 * 2 * np.abs(stack)).all() and not np.array_equal(added, stack)


def test_junk_under_the_mask_reaches_nothing(dev):
    """NaN, inf and -999 in trans under ivar == 0: the same bits as zeros in their place, and everything finite"""
    B, S, nb, L, nseg, nlag = 6, 1, 90, 40, 2, 40
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=51)
    prm = (3, L, nseg, 20, BINS)
    z = T(g["zabs"], dev)
    masked = (iv == 0)
    assert masked.any()
    junk = tr.clone()
    vals = T(np.array([np.nan, np.inf, -np.inf, -999.0], np.float32), dev)
    junk[masked] = vals[(masked.nonzero()[:, 2] % 4)]
    for sigma2, unit in ((0.0, False), (0.1, False), (0.0, True)):
        fl = F_ZERO | (F_UNIT if unit else 0)
        clean = call_x(dev, tr, iv, tbar, prm, nlag, sigma2=sigma2, zabs=z, flags=fl)
        dirty = call_x(dev, junk, iv, tbar, prm, nlag, sigma2=sigma2, zabs=z, flags=fl)
        assert clean[2][:, :, 0].sum() > 0
        for x, y in zip(clean, dirty):
            assert np.isfinite(y).all() and np.array_equal(x, y)


def test_every_refusal_returns_its_code_and_touches_nothing(dev):
    B, S, nb, L, nseg, nlag = 4, 1, 60, 20, 2, 10
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=61)
    z = T(g["zabs"], dev)
    prm = (0, L, nseg, 10, BINS)

    refused = refusals(lambda **kw: call_x(dev, tr, iv, tbar, **kw), prm=prm, nlag=nlag, sigma2=0.0, flags=F_ZERO, outs="pns", zabs=z)
    refused(-1, outs="")                                                              # all three outputs missing
    refused(-1, zabs=None)                                                            # no redshift at all
    refused(-1, zabs=None, zq1=T(g["zq1"], dev))                                      # half of the factored pair
    for bad in (0, -1, L + 1):
        refused(-2, nlag=bad)
    for bad in (-0.5, float("nan"), float("inf")):
        refused(-2, sigma2=bad)
    refused(-2, prm=(0, L, nseg, 0, BINS))                                            # min_used < 1
    refused(-2, prm=(21, L, nseg, 10, BINS))                                          # the segments pass Nb
    refused(-2, prm=(0, L, nseg, 10, (1.6, 0.0, 4)))                                  # dz = 0
    refused(-2, prm=(0, L, nseg, 10, (1.6, 0.45, 0)))                                 # nz = 0
    for flags in (0x1, 0x100, 0x200, 0x800, F_ZERO | 0x8):
        refused(-5, flags=flags)
    # x missing, and a workspace one byte short
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    bs = _lib.Batch()
    bs.zabs, bs.row_stride = z.data_ptr(), 0
    pp = _lib.P1DParams(TB_BINS[0], TB_BINS[1], TB_BINS[2], 1, 0, L, nseg, 10, BINS[0], BINS[1], BINS[2])
    xx = _lib.XiParams(nlag, 0.0)
    tb = T(tbar, dev).contiguous()
    out = torch.full((B, S, nseg, 2, nlag), -7.0, dtype=torch.float32, device=dev)
    need = lib.qfa_xi_workspace_bytes(B * S, S, nb, L, nseg, BINS[2], nlag)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    common = (C.c_void_p(tr.data_ptr()), C.c_void_p(iv.data_ptr()), C.byref(bs), C.c_void_p(tb.data_ptr()), B, S, nb, C.byref(pp))
    tail = (0, C.c_void_p(out.data_ptr()), None, None, C.c_void_p(ws.data_ptr()))
    assert lib.qfa_xi_f32(*common, None, *tail, need, None) == -1
    assert lib.qfa_xi_f32(*common, C.byref(xx), *tail, need - 1, None) == -3
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ------------------------------------------------------------------------------------------------------------ end to end
def sum_abs_bound(buf, nlag):
    """an upper bound of sum |terms| behind every entry of a stack (S, nz, 2 + 5 nlag), from the stack itself: the entries whose
    terms are >= 0 are their own; sum |A_l| <= sqrt(n sum A_l^2) and sum |A_l W_l| <= sqrt(sum A_l^2 sum W_l^2) (Cauchy-Schwarz)"""
    out = np.abs(buf).copy()
    n = buf[:, :, :1]
    W2, A2 = buf[:, :, 2 + 2 * nlag:2 + 3 * nlag], buf[:, :, 2 + 4 * nlag:]
    out[:, :, 2 + nlag:2 + 2 * nlag] = np.sqrt(n * A2) * (1 + 1e-9)
    out[:, :, 2 + 3 * nlag:2 + 4 * nlag] = np.sqrt(A2 * W2) * (1 + 1e-9)
    return out


def test_flux_correlation_of_a_loader(dev):
    import torch
    m, mk, wav = loader_case(dev)
    kw = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, seed=6, sigma2_lss=0.05)
    for S in (0, 3):
        a = m.flux_correlation(mk(96), 1.8, 3.4, 3, 10, n_samples=S, batch_size=96, **kw)
        c = m.flux_correlation(mk(96), 1.8, 3.4, 3, 10, n_samples=S, batch_size=40, **kw)
        assert a.S == max(1, S) and a.L == 24 and a.nlag == 10 and torch.equal(a.n, c.n) and a.n.sum() > 20 * a.S
        assert np.isclose(a.dv, 299792.458 * np.log(wav[1] / wav[0])) and np.allclose(a.lags_kms.cpu().numpy(), a.dv * np.arange(10))
        x, y = a.buf.cpu().numpy(), c.buf.cpu().numpy()
        # other calls, other chunks: two groupings of the same float64 terms, each within n 2^-53 sum |terms| of their exact sum
        assert (np.abs(x - y) <= 2 * x[:, :, :1] * U64 * sum_abs_bound(x, 10)).all(), S
        assert torch.isfinite(a.xi()[a.n > 1]).all() and torch.isfinite(a.err()[a.n > 1]).all()
    assert a.std_over_draws.shape == (3, 10)
    # xi by hand on the one slice, with a ForestStack for tbar, adds up to the same stack (S = 1), bit for bit
    dl = mk(96)
    one = m.flux_correlation(dl, 1.8, 3.4, 3, 10, batch_size=96, **kw)
    half = float(np.exp(0.5 * 25 * one.dv / 299792.458))
    tb1 = m.mean_transmission(dl, 2.8 / half - 1.0, 4.4 * half - 1.0, 8, batch_size=96)
    for _, inputs, _ in m._loader_slices(dl, 96):
        _, hm, _, _, unc = m.predict(**inputs)
        tr, iv, _ = m.forest(**inputs, hmean=hm, unc=unc)
        zin = {"batch": inputs["batch"]} if "batch" in inputs else {"zabs": inputs["zabs"]}
        pr, n0, st = m.xi(tr, iv, **zin, tbar=tb1, seg_len=24, n_segments=2, min_used=18, n_lags=10, sigma2_lss=0.05, bins=one.bins,
                          dv=one.dv)
    assert pr.shape == (96, 1, 2, 2, 10) and n0.shape == (96, 1, 2) and torch.equal(st.buf, one.buf)


def test_cli_predict_writes_flux_correlation_npz(dev, tmp_path):
    """predict mode with MODEL.XI_NLAGS: flux_correlation.npz next to flux_power.npz, with the documented keys"""
    from qfa_amd import cli
    c = cli_predict_case(dev, tmp_path)
    wav, nb = c.wav, c.nb
    out = tmp_path / "out"
    L = nb // 2
    nlag = min(12, L)
    argv = c.argv(out, "MODEL.N_SAMPLES", "2", "MODEL.XI_NLAGS", str(nlag), "MODEL.XI_SIGMA2_LSS", "0.02")
    assert cli.main(argv) == 0
    f, fp = np.load(out / "flux_correlation.npz"), np.load(out / "flux_power.npz")
    assert set(f.files) == {"lags_kms", "z_centers", "z_edges", "xi", "xi_raw", "err", "n", "sum_w", "seg_len", "dv", "sums"}
    assert int(f["seg_len"]) == L and f["sums"].shape == (2, 3, 2 + 5 * nlag) and f["lags_kms"].shape == (nlag,)
    assert f["xi"].shape == f["xi_raw"].shape == f["err"].shape == f["sum_w"].shape == (2, 3, nlag) and f["n"].shape == (2, 3)
    assert np.array_equal(f["n"], fp["n"]) and f["n"].sum() > 10                       # the segments flux_power stacked
    assert np.isclose(float(f["dv"]), float(fp["dv"])) and np.allclose(f["lags_kms"], float(f["dv"]) * np.arange(nlag))
    assert np.isfinite(f["xi"][f["n"] > 1]).all() and (f["xi_raw"][..., 0][f["n"] > 0] > 0).all()
