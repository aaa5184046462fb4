"""Forest transmission and its stack on the MI355X (QFA.forest / mean_transmission, qfa_forest_f32) against the numpy port of the
contract (tests/_forest_ref.py).

Per-pixel bars (tests/_forest_ref.py, trans_bound / ivar_bound):
  |dT|  <= |T|  ((Nh + 2) u cabs / |c| + 2 u)        the fma chain plus one division, u = 2^-24
  |div| <= |iv| (4 (Nh + 2) u cabs / |c| + 10 u)     c and T enter squared, four more roundings (derivation at ivar_bound)
and the `use` pattern matches exactly: the inputs keep every |c - cont_min| above the chain bound, which the test asserts on the
port.  Stack: N 2^-53 sum |terms| per entry against float64 sums of the GPU's own pixels (N - 1 non-trivial additions in any
order, the terms themselves formed alike), counts exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _forest_ref as R
from _segment_harness import T, dev, geometry, make_model  # noqa: F401 (dev: the fixture)
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
CONT_MIN = 0.05


def call_c(m, flux, error, h, bins, *, zabs=None, mask=None, zq1=None, ratio=None, rows=None, row_stride=0, unc=None,
           cont_min=CONT_MIN, flags=0, trans=None, ivar=None, stack=None, pixel_range=None, B=None):
    """qfa_forest_f32 by hand; returns the status"""
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    m._params_struct()
    bs = _lib.Batch()
    ptr = lambda t: None if t is None else t.data_ptr()
    bs.delta, bs.error, bs.zabs, bs.mask = ptr(flux), ptr(error), ptr(zabs), ptr(mask)
    bs.A_blue, bs.zq1, bs.pix_ratio, bs.rows, bs.row_stride = None, ptr(zq1), ptr(ratio), ptr(rows), int(row_stride)
    B = h.shape[0] if B is None else B
    S = h.shape[1]
    p_lo, p_hi = (0, m.Nb) if pixel_range is None else pixel_range
    fb = _lib.ForestBins(bins[0], bins[1], bins[2], p_lo, p_hi)
    need = lib.qfa_forest_workspace_bytes(B, S, m.Npix, m.Nb, m.Nh, bins[2])
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    st = lib.qfa_forest_f32(C.c_void_p(m.F.data_ptr()), C.c_void_p(m.mu.data_ptr()), C.byref(bs), C.c_void_p(h.data_ptr()),
                            C.c_void_p(ptr(unc)), B, S, m.Npix, m.Nb, m.Nh, C.byref(fb), cont_min, flags, C.c_void_p(ptr(trans)),
                            C.c_void_p(ptr(ivar)), C.c_void_p(ptr(stack)), C.c_void_p(ws.data_ptr()), need,
                            _lib.current_stream(m.device))
    torch.cuda.synchronize()
    return st


def check_pixels(got_T, got_iv, ref, nh, what):
    """the per-pixel bars of the module docstring on EVERY pixel, and the exact `use` pattern"""
    use = ref["use"]
    assert np.array_equal(got_iv != 0, use), what                                     # (iv > 0 on every used pixel)
    assert (got_T[~use] == 0).all() and (got_iv[~use] == 0).all(), what
    eT, eI = np.abs(got_T.astype(np.float64) - ref["T"]), np.abs(got_iv.astype(np.float64) - ref["iv"])
    bT, bI = R.trans_bound(ref, nh), R.ivar_bound(ref, nh)
    if use.any():
        print(f"{what}: max |dT| / bound = {(eT[use] / bT[use].clip(1e-300)).max():.3f}, max |div| / bound = {(eI[use] / bI[use]).max():.3f}")
    assert (eT <= bT).all(), (what, "trans")
    assert (eI <= bI).all(), (what, "ivar")


def check_stack(got, got_T, got_iv, ref, what, unit_w=False):
    """against float64 sums of the GPU's own pixels under the port's bins: N 2^-53 sum |terms|; counts exact"""
    own, own_abs = R.stack_of(got_T, got_iv, ref["use"], ref["k"], got.shape[2], unit_w)
    assert np.array_equal(got[:, 3], ref["stack"][:, 3]), (what, "counts")
    N = ref["stack"][:, 3][:, None, :]
    assert (np.abs(got - own) <= N * U64 * own_abs).all(), (what, np.abs(got - own).max())
    return own


SHAPES = [(1, 1), (3, 1), (5, 5), (257, 255), (1027, 1025), (300, 0)]
NHS = [1, 8, 9, 16, 17, 32]


@pytest.mark.parametrize("nh", NHS)
@pytest.mark.parametrize("npix,nb", SHAPES)
def test_values_and_stack_match_the_port(dev, npix, nb, nh):
    """every input form (zabs, factored, resident with shuffled rows and a padded stride), mask NULL and random, outputs offset by one
    float; B, S and nbin walk {1, 3, 65} x {1, 3} x {1, 7, 64} over the cases"""
    import torch
    i = SHAPES.index((npix, nb)) + NHS.index(nh)
    B, S, nbin = (1, 3, 65)[i % 3], (1, 3)[(i // 3) % 2], (1, 7, 64)[(i + i // 3) % 3]
    bins = (1.5, 2.1 / nbin, nbin)
    g = geometry(npix, nb, nh, B, S, seed=100 * npix + nh, masks=i % 2 == 0)
    m = make_model(dev, g, nb, npix - nb, nh)
    unc = g["unc"] if S == 1 else None
    refs = {"zabs": R.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zabs"], g["mask"], g["h"], unc, bins, CONT_MIN)}
    refs["factored"] = R.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zfac"], g["mask"], g["h"], unc, bins, CONT_MIN)
    refs["rows"] = refs["zabs"]
    r0 = refs["zabs"]
    if nb > 0:
        # c in [0.5, 2], and no continuum within the chain bound of cont_min: the use pattern is defined, no pixel is excused
        assert r0["c"].min() >= 0.5 and r0["c"].max() <= 2.0
        assert (np.abs(r0["c"] - CONT_MIN) > (nh + 2) * R.U * r0["cabs"]).all()
    # the resident form: rows of a larger, padded array in another order
    stride, N = npix + 5, B + 3
    rows = np.random.default_rng(5).permutation(N)[:B].astype(np.int32)
    fres, eres = (np.full((N, stride), np.nan, np.float32) for _ in range(2))
    mres = np.zeros((N, stride), bool)
    zres = np.full((N, max(nb, 1)), np.nan, np.float32)[:, :nb]
    fres[rows, :npix], eres[rows, :npix], zres[rows] = g["flux"], g["error"], g["zabs"]
    mres[rows, :npix] = True if g["mask"] is None else g["mask"]
    fl, er, h = T(g["flux"], dev), T(g["error"], dev), T(g["h"], dev)
    mk = None if g["mask"] is None else T(g["mask"], dev)
    forms = {"zabs": dict(flux=fl, error=er, mask=mk, zabs=T(g["zabs"], dev)),
             "factored": dict(flux=fl, error=er, mask=mk, zq1=T(g["zq1"], dev), ratio=T(g["ratio"], dev)),
             "rows": dict(flux=T(fres, dev), error=T(eres, dev), mask=T(mres, dev), zabs=T(np.ascontiguousarray(zres), dev),
                          rows=T(rows, dev), row_stride=stride)}
    n = B * S * nb
    for name, kw in forms.items():
        if nb == 0:
            kw = {k: v for k, v in kw.items() if k not in ("zabs", "zq1", "ratio")}
        bufs = [torch.full((n + 9,), -7.0, dtype=torch.float32, device=dev) for _ in range(2)]
        to, io = (b[1:1 + n] for b in bufs)                                       # offset by one float
        stack = torch.full((S, 4, nbin), 3.0, dtype=torch.float64, device=dev)
        st = call_c(m, kw.pop("flux"), kw.pop("error"), h, bins, unc=None if unc is None else T(unc, dev), trans=to, ivar=io,
                    stack=stack, flags=0x80, **kw)
        assert st == 0, name
        for b in bufs:
            rest = b.cpu().numpy()
            assert rest[0] == -7.0 and (rest[1 + n:] == -7.0).all(), name
        got = stack.cpu().numpy()
        if nb == 0:
            assert (got == 0).all(), name                                         # Nb = 0 under ZERO_ACCUM still zeroes the stack
            continue
        ref = refs[name]
        gT, gI = to.cpu().numpy().reshape(B, S, nb), io.cpu().numpy().reshape(B, S, nb)
        what = f"npix {npix} nb {nb} nh {nh} B {B} S {S} nbin {nbin} {name}"
        check_pixels(gT, gI, ref, nh, what)
        check_stack(got, gT, gI, ref, what)
        # and against the all-port stack, the per-pixel bars propagated (1.001: second order and the float64 summation)
        bT, bI, aT = R.trans_bound(ref, nh), R.ivar_bound(ref, nh), np.abs(ref["T"])
        tol = [bI, bI * aT + ref["iv"] * bT, bI * aT * aT + 2 * ref["iv"] * aT * bT]
        for q in range(3):
            prop, _ = R.stack_of(np.ones_like(bT), tol[q], ref["use"], ref["k"], nbin)
            assert (np.abs(got[:, q] - ref["stack"][:, q]) <= 1.001 * prop[:, 0] + 1e-300).all(), (what, q)


def small(dev, nh=8, B=3, S=1, npix=300, nb=113, seed=7, masks=True):
    g = geometry(npix, nb, nh, B, S, seed, masks)
    m = make_model(dev, g, nb, npix - nb, nh)
    t = {k: T(g[k], dev) for k in ("flux", "error", "zabs", "h", "unc", "zq1", "ratio")}
    t["mask"] = None if g["mask"] is None else T(g["mask"], dev)
    return g, m, t


def test_unused_pixel_is_exactly_zero(dev):
    """F = 0 and one mu[p] = 0.01 < cont_min: that pixel is unused, exactly 0 / 0, and leaves the stack"""
    g, m, t = small(dev, masks=False)
    import torch
    m.F = torch.zeros_like(m.F)
    mu = g["mu"].copy()
    mu[17] = 0.01
    m.mu = T(mu, dev)
    bins = (1.5, 0.3, 7)
    tr, iv, st = m.forest(t["flux"], t["error"], t["zabs"], None, h=t["h"], bins=bins, cont_min=CONT_MIN)
    assert (tr[:, :, 17] == 0).all() and (iv[:, :, 17] == 0).all()
    keep = np.arange(113) != 17
    assert (iv.cpu().numpy()[:, :, keep] > 0).all()
    ref = R.forest(np.zeros_like(g["p"]["F"]), mu, g["flux"], g["error"], g["zabs"], None, g["h"], None, bins, CONT_MIN)
    assert not ref["use"][:, :, 17].any() and np.array_equal(st.n.cpu().numpy(), ref["stack"][:, 3])


def test_junk_under_the_mask_and_nan_latent(dev):
    import torch
    g, m, t = small(dev, S=3, B=4)
    bins = (1.5, 0.3, 7)
    base = m.forest(t["flux"], t["error"], t["zabs"], t["mask"], h=t["h"], bins=bins, cont_min=CONT_MIN)
    for junk in (float("nan"), float("inf"), -999.0):
        f2 = torch.where(t["mask"], t["flux"], torch.full_like(t["flux"], junk))
        e2 = torch.where(t["mask"], t["error"], torch.full_like(t["error"], junk))
        got = m.forest(f2, e2, t["zabs"], t["mask"], h=t["h"], bins=bins, cont_min=CONT_MIN)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and torch.equal(got[2].buf, base[2].buf), junk
        assert torch.isfinite(got[2].buf).all()
    hn = t["h"].clone()
    hn[2, 1, 3] = float("nan")
    got = m.forest(t["flux"], t["error"], t["zabs"], t["mask"], h=hn, bins=bins, cont_min=CONT_MIN)
    assert (got[0][2, 1] == 0).all() and (got[1][2, 1] == 0).all()
    keep = torch.ones((4, 3), dtype=torch.bool, device=dev)
    keep[2, 1] = False
    assert torch.equal(got[0][keep], base[0][keep]) and torch.equal(got[1][keep], base[1][keep])
    assert torch.equal(got[2].buf[[0, 2]], base[2].buf[[0, 2]]) and torch.isfinite(got[2].buf).all()
    assert (got[2].n[1] < base[2].n[1]).any()


@pytest.mark.parametrize("nbin", [5, 64, 700])
def test_non_monotone_redshifts_and_bin_edges(dev, nbin):
    """zabs in random order (nbin = 700: the form whose tables live in the workspace), with values exactly on bin edges, below z0,
    at and above the top edge, and NaN"""
    g, m, t = small(dev, B=5, S=2, masks=True)
    rng = np.random.default_rng(3)
    z0, dz = np.float32(2.0), np.float32(1.0 / nbin if nbin != 5 else 0.25)
    top = z0 + dz * nbin
    z = rng.uniform(1.9, float(top) + 0.1, g["zabs"].shape).astype(np.float32)
    edges = (z0 + dz * np.arange(nbin + 1, dtype=np.float32)).astype(np.float32)
    z[:, :40] = rng.choice(edges, (5, 40))
    z[0, 40:46] = [np.nan, z0, np.nextafter(z0, np.float32(0)), top, np.nextafter(top, np.float32(0)), np.inf]
    bins = (float(z0), float(dz), nbin)
    ref = R.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], z, g["mask"], g["h"], None, bins, CONT_MIN)
    assert (ref["k"][:, :46] == -1).any() and (ref["k"] == nbin - 1).any() and (ref["k"] == 0).any()
    tr, iv, st = m.forest(t["flux"], t["error"], T(z, dev), t["mask"], h=t["h"], bins=bins, cont_min=CONT_MIN)
    gT, gI = tr.cpu().numpy(), iv.cpu().numpy()
    check_pixels(gT, gI, ref, 8, f"non-monotone nbin {nbin}")
    check_stack(st.buf.cpu().numpy(), gT, gI, ref, f"non-monotone nbin {nbin}")


def test_pixel_range_unit_weights_and_accumulation(dev):
    import torch
    g, m, t = small(dev, B=4, S=2)
    bins = (1.5, 0.3, 7)
    args = (t["flux"], t["error"], t["zabs"], t["mask"])
    tr, iv, st = m.forest(*args, h=t["h"], bins=bins, cont_min=CONT_MIN, pixel_range=(10, 77), unit_weights=True)
    ref = R.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zabs"], g["mask"], g["h"], None, bins, CONT_MIN, True, (10, 77))
    gT, gI = tr.cpu().numpy(), iv.cpu().numpy()
    check_pixels(gT, gI, ref, 8, "pixel_range")                                   # the range restricts the stack, not the pixels
    own = check_stack(st.buf.cpu().numpy(), gT, gI, ref, "pixel_range + unit weights", unit_w=True)
    assert np.array_equal(st.buf.cpu().numpy()[:, 0], own[:, 3])                  # sum of w = 1 is the count
    # two calls give the same bits; the call ADDS, QFA_F_ZERO_ACCUM overwrites
    a = m.forest(*args, h=t["h"], bins=bins, cont_min=CONT_MIN)[2]
    b = m.forest(*args, h=t["h"], bins=bins, cont_min=CONT_MIN)[2]
    assert torch.equal(a.buf, b.buf)
    m.forest(*args, h=t["h"], stack=b, cont_min=CONT_MIN, return_pixels=False)
    assert torch.equal(b.buf, a.buf + a.buf)
    raw = torch.full((2, 4, 7), 9.0, dtype=torch.float64, device=dev)
    assert call_c(m, t["flux"], t["error"], t["h"], bins, zabs=t["zabs"], mask=t["mask"], stack=raw) == 0
    assert torch.equal(raw, a.buf + 9.0)
    assert call_c(m, t["flux"], t["error"], t["h"], bins, zabs=t["zabs"], mask=t["mask"], stack=raw, flags=0x80) == 0
    assert torch.equal(raw, a.buf)
    assert call_c(m, t["flux"], t["error"], t["h"], bins, zabs=t["zabs"], mask=t["mask"], stack=raw, flags=0x80, B=0) == 0
    assert (raw == 0).all()                                                       # B = 0 under ZERO_ACCUM zeroes the stack


def test_split_in_spectra_and_in_draws(dev):
    """one call over B = 65 against 32 + 33 added, and S = 3 against three S = 1 calls on the slices of h: the same sums within the
    summation bound N 2^-53 sum |terms| (bit-equal pixels)"""
    import torch
    g, m, t = small(dev, B=65, S=3, npix=300, nb=113, seed=11)
    bins = (1.5, 2.1 / 64, 64)
    tr, iv, st = m.forest(t["flux"], t["error"], t["zabs"], t["mask"], h=t["h"], bins=bins, cont_min=CONT_MIN)
    ref = R.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zabs"], g["mask"], g["h"], None, bins, CONT_MIN)
    _, own_abs = R.stack_of(tr.cpu().numpy(), iv.cpu().numpy(), ref["use"], ref["k"], 64)
    tol = ref["stack"][:, 3][:, None, :] * U64 * own_abs
    parts = None
    for a, b in ((0, 32), (32, 65)):
        sl = lambda x: x[a:b].contiguous()
        trp, ivp, parts = m.forest(sl(t["flux"]), sl(t["error"]), sl(t["zabs"]), sl(t["mask"]), h=sl(t["h"]), cont_min=CONT_MIN,
                                   stack=parts, bins=bins)
        assert torch.equal(trp, tr[a:b]) and torch.equal(ivp, iv[a:b])
    assert (np.abs(parts.buf.cpu().numpy() - st.buf.cpu().numpy()) <= tol).all()
    assert torch.equal(parts.n, st.n)
    for s in range(3):
        trs, ivs, one = m.forest(t["flux"], t["error"], t["zabs"], t["mask"], h=t["h"][:, s:s + 1].contiguous(), bins=bins,
                                 cont_min=CONT_MIN)
        assert torch.equal(trs[:, 0], tr[:, s]) and torch.equal(ivs[:, 0], iv[:, s])
        assert (np.abs(one.buf.cpu().numpy()[0] - st.buf.cpu().numpy()[s]) <= tol[s]).all()
        assert torch.equal(one.n[0], st.n[s])


# ------------------------------------------------------------------------------------------------------------ Python surface
def batch_case(dev, npix=300, nh=8, B=10, seed=8):
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=100 + seed)
    m = make_model(dev, {"p": p, "mu": mu}, nb, nr, nh)
    return m, b, wav, nb, tuple(T(b[k], dev) for k in ("flux", "error", "zabs", "mask"))


def test_forest_with_each_way_of_giving_the_latent(dev):
    import torch
    m, b, wav, nb, inputs = batch_case(dev)
    B, S, bins = 10, 4, (1.8, 0.1, 17)
    _, hm, hc, _, unc = m.predict(*inputs)
    # none of them: predict first, its unc at S = 1
    auto = m.forest(*inputs, bins=bins)
    mean = m.forest(*inputs, hmean=hm, unc=unc, bins=bins)
    assert auto[0].shape == (B, 1, nb) and all(torch.equal(x, y) for x, y in zip(auto[:2], mean[:2]))
    assert torch.equal(auto[2].buf, mean[2].buf)
    assert not torch.equal(m.forest(*inputs, hmean=hm, bins=bins)[1], mean[1])     # unc enters ivar
    assert torch.equal(m.forest(*inputs, hmean=hm, bins=bins)[0], mean[0])        # ... not T
    assert torch.equal(m.forest(*inputs, hmean=hm, hcov=hc, unc=unc, bins=bins)[2].buf, mean[2].buf)   # n_samples = 0: the mean
    # draws: bit-equal to sample_latent + a call by hand
    h = m.sample_latent(hm, hc, S, seed=5, offset=40)
    drawn = m.forest(*inputs, hmean=hm, hcov=hc, n_samples=S, seed=5, offset=40, bins=bins)
    given = m.forest(*inputs, h=h, bins=bins)
    auto_s = m.forest(*inputs, n_samples=S, seed=5, offset=40, bins=bins)
    to, io = (torch.empty((B, S, nb), dtype=torch.float32, device=dev) for _ in range(2))
    so = torch.zeros((S, 4, 17), dtype=torch.float64, device=dev)
    fb = (drawn[2].z0, drawn[2].dz, 17)
    assert call_c(m, inputs[0], inputs[1], h, fb, zabs=inputs[2], mask=inputs[3], trans=to, ivar=io, stack=so, cont_min=0.0) == 0
    for got in (drawn, given, auto_s):
        assert torch.equal(got[0], to) and torch.equal(got[1], io) and torch.equal(got[2].buf, so)
    assert drawn[2].S == S and drawn[2].std_over_draws.shape == (17,) and drawn[2].mean_over_draws.shape == (17,)
    # stack only / pixels only
    assert m.forest(*inputs, h=h, bins=bins, return_pixels=False)[:2] == (None, None)
    assert m.forest(*inputs, h=h)[2] is None
    # the factored form and a resident batch give the same bits as each other
    from qfa_amd import synthetic
    from qfa_amd.resident import ResidentBatch
    zf = (T(1.0 + b["zqso"], dev), T((wav[:nb] / synthetic.LYA).astype(np.float32), dev))
    ff = m.forest(inputs[0], inputs[1], None, inputs[3], h=h, bins=bins, zfac=zf)
    rb = ResidentBatch(inputs[0], None, inputs[1], inputs[3], zf[0], zf[1], T(np.arange(B, dtype=np.int32), dev), 300, nb)
    fr = m.forest(batch=rb, h=h, bins=bins)
    assert torch.equal(ff[0], fr[0]) and torch.equal(ff[2].buf, fr[2].buf)
    from qfa_amd._lib import QFAHipError
    for kw in (dict(h=h, hmean=hm), dict(hcov=hc), dict(hmean=hm, n_samples=2), dict(h=h, n_samples=3), dict(h=h, bins=(2.0, 0.0, 4)),
               dict(h=h, pixel_range=(5, nb + 1)), dict(h=h, return_pixels=False), dict(h=h, unc=unc[:, :-1]),
               dict(h=h, stack=auto[2])):
        with pytest.raises(QFAHipError):
            m.forest(*inputs, **kw)


class _ListLoader(object):
    """the reference's per-spectrum dataloader contract: loader[i] = (flux, error, zabs, mask, path)"""

    def __init__(self, inputs):
        self.inputs = inputs

    def __len__(self):
        return self.inputs[0].shape[0]

    def __getitem__(self, i):
        return tuple(x[i] for x in self.inputs) + (f"spec{i:03d}",)


def test_mean_transmission_does_not_depend_on_batch_size(dev):
    import torch
    from qfa_amd.dataloader import DeviceDataloader
    m, b, wav, nb, inputs = batch_case(dev, B=23, seed=9)
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, batch_size=6, device=dev, shuffle=False)
    for S in (0, 3):
        a = m.mean_transmission(dl, 1.8, 3.5, 17, n_samples=S, seed=4, batch_size=6)
        c = m.mean_transmission(dl, 1.8, 3.5, 17, n_samples=S, seed=4, batch_size=4096)
        assert a.S == max(1, S) and torch.equal(a.n, c.n) and a.n.sum() > 0
        x, y = a.buf.cpu().numpy(), c.buf.cpu().numpy()
        # both are sums of the same terms in another order: within N 2^-53 sum |terms| of each other; the terms of w and w T^2 are
        # positive, and sum |w T| <= sqrt(sum w  sum w T^2) (Cauchy-Schwarz)
        asum = np.stack([y[:, 0], np.sqrt(y[:, 0] * y[:, 2]) * (1 + 1e-9), y[:, 2]], 1)
        assert (np.abs(x - y)[:, :3] <= y[:, 3:4] * U64 * asum).all(), S
    # the per-spectrum contract walks the same spectra: the zabs kernels against the loader's factored form, same counts
    lst = m.mean_transmission(_ListLoader(tuple(x for x in (T(b["flux"], dev), T(b["error"], dev), T(b["zabs"], dev), T(b["mask"], dev)))),
                              1.8, 3.5, 17, batch_size=5)
    assert lst.S == 1 and abs(float(lst.n.sum() - m.mean_transmission(dl, 1.8, 3.5, 17).n.sum())) <= 2      # (a z on an edge may move)


def test_predict_to_npz_forest_keys_and_unchanged_defaults(dev, tmp_path):
    m, b, wav, nb, inputs = batch_case(dev)
    loader = _ListLoader(inputs)
    w1 = m.predict_to_npz(loader, str(tmp_path / "f"), batch_size=4, forest=True)
    w0 = m.predict_to_npz(loader, str(tmp_path / "d"), batch_size=4)
    assert w1 == w0 and len(w0) == 10
    _, hm, _, _, unc = m.predict(*inputs)
    tr, iv, _ = m.forest(*inputs, hmean=hm, unc=unc)
    for i, name in enumerate(w0):
        a, z = np.load(str(tmp_path / "f" / name)), np.load(str(tmp_path / "d" / name))
        assert sorted(z.files) == ["cont", "hcov", "hmean", "ll", "uncertainty"]
        assert sorted(a.files) == sorted(z.files + ["transmission", "transmission_ivar"])
        assert a["transmission"].shape == (nb,) and a["transmission_ivar"].shape == (nb,)
        assert np.array_equal(a["transmission"], tr[i, 0].cpu().numpy()) and np.array_equal(a["transmission_ivar"], iv[i, 0].cpu().numpy())
        for k in z.files:
            assert np.array_equal(a[k], z[k], equal_nan=True), k


def test_graph_capture_replays_the_eager_bits(dev):
    import torch
    g, m, t = small(dev, B=5, S=3)
    bins = (1.5, 0.3, 7)
    eager = m.forest(t["flux"], t["error"], t["zabs"], t["mask"], h=t["h"], bins=bins, cont_min=CONT_MIN)   # (workspace allocated)
    to, io = (torch.zeros_like(eager[0]) for _ in range(2))
    so = torch.zeros_like(eager[2].buf)
    from qfa_amd import _lib
    need = _lib.lib().qfa_forest_workspace_bytes(5, 3, m.Npix, m.Nb, m.Nh, 7)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    m._params_struct()
    bs = _lib.Batch()
    bs.delta, bs.error, bs.zabs, bs.mask = (t[k].data_ptr() for k in ("flux", "error", "zabs", "mask"))
    fb = _lib.ForestBins(eager[2].z0, eager[2].dz, 7, 0, m.Nb)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        st = _lib.lib().qfa_forest_f32(C.c_void_p(m.F.data_ptr()), C.c_void_p(m.mu.data_ptr()), C.byref(bs),
                                       C.c_void_p(t["h"].data_ptr()), None, 5, 3, m.Npix, m.Nb, m.Nh, C.byref(fb), CONT_MIN, 0x80,
                                       C.c_void_p(to.data_ptr()), C.c_void_p(io.data_ptr()), C.c_void_p(so.data_ptr()),
                                       C.c_void_p(ws.data_ptr()), need, _lib.current_stream(dev))
    assert st == 0
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(to, eager[0]) and torch.equal(io, eager[1]) and torch.equal(so, eager[2].buf)


def test_transmission_on_the_committed_sdss_fixture(dev):
    """T from predict's own hmean against numpy on the downloaded hmean, on tests/golden/sdss_spectrum.npz + model_parameters.npz
    (zabs and the mask of that spectrum: g1_g2_predict.npz)"""
    import torch
    from oracle import qfa_oracle as O
    from qfa_amd import QFA
    p, mu = O.load_params_npz(os.path.join(GOLDEN, "model_parameters.npz"))
    spec = np.load(os.path.join(GOLDEN, "sdss_spectrum.npz"))
    gold = np.load(os.path.join(GOLDEN, "g1_g2_predict.npz"))
    flux, error = (np.asarray(spec[k], np.float32).reshape(1, -1) for k in ("flux", "error"))
    zabs, mask = np.asarray(gold["zabs"], np.float32).reshape(1, -1), np.asarray(gold["mask_full"], bool).reshape(1, -1)
    nb, npix, nh = zabs.shape[1], flux.shape[1], p["F"].shape[1]
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    m.mu = T(mu, dev)
    inputs = (T(flux, dev), T(error, dev), T(zabs, dev), T(mask, dev))
    _, hm, _, _, unc = m.predict(*inputs)
    tr, iv, st = m.forest(*inputs, hmean=hm, unc=unc, bins=(float(zabs.min()) - 0.01, 0.05, 40), cont_min=CONT_MIN)
    ref = R.forest(p["F"], mu, flux, error, zabs, mask, hm.cpu().numpy().reshape(1, 1, nh), unc.cpu().numpy(), (st.z0, st.dz, 40),
                   CONT_MIN)
    assert (np.abs(ref["c"] - CONT_MIN) > (nh + 2) * R.U * ref["cabs"]).all() and ref["use"].sum() > 100
    check_pixels(tr.cpu().numpy(), iv.cpu().numpy(), ref, nh, "sdss fixture")
    check_stack(st.buf.cpu().numpy(), tr.cpu().numpy(), iv.cpu().numpy(), ref, "sdss fixture")


# ------------------------------------------------------------------------------------------------------------ data parallel
def _dp_case():
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(220)
    p, mu = synthetic.mock_parameters(220, nb, 4, seed=8)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 11, seed=81)
    return p, mu, wav, nb, nr, b


def _worker_forest(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from qfa_amd import QFA
    from qfa_amd.dataloader import DeviceDataloader
    dev = torch.device("cuda:0")
    p, mu, wav, nb, nr, b = _dp_case()
    m = QFA(nb, nr, 4, dev, model_params=p)
    m.mu = torch.tensor(mu, dtype=torch.float32, device=dev)
    m.enable_data_parallel()
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, batch_size=4, device=dev, shuffle=False, rank=rank, world=world)
    st = m.mean_transmission(dl, 1.8, 3.5, 9, n_samples=2, seed=3, batch_size=4)
    if rank == 0:
        q.put(st.buf.cpu().numpy())
    dist.destroy_process_group()


def test_two_ranks_all_reduce_to_the_single_process_stack(dev):
    import torch
    import torch.multiprocessing as mp
    from qfa_amd import QFA
    from qfa_amd.dataloader import DeviceDataloader
    from test_data_parallel import _collect
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker_forest, args=(r, 2, port, q)) for r in range(2)]
    [pr.start() for pr in procs]
    got = _collect(procs, q, 300)
    [pr.join(60) for pr in procs]
    assert all(pr.exitcode == 0 for pr in procs)
    p, mu, wav, nb, nr, b = _dp_case()
    m = QFA(nb, nr, 4, dev, model_params=p)
    m.mu = torch.tensor(mu, dtype=torch.float32, device=dev)
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, batch_size=4, device=dev, shuffle=False)
    m.mu = torch.tensor(mu, dtype=torch.float32, device=dev)
    one = m.mean_transmission(dl, 1.8, 3.5, 9, n_samples=2, seed=3, batch_size=4).buf.cpu().numpy()
    assert np.array_equal(got[:, 3], one[:, 3]) and one[:, 3].sum() > 0
    rb = dl.rows_batch(0, 11)[0]
    _, hm, hc, _, _ = m.predict(batch=rb)
    bins = (1.8, (3.5 - 1.8) / 9, 9)
    tr, iv, st = m.forest(batch=rb, hmean=hm, hcov=hc, n_samples=2, seed=3, bins=bins)
    assert torch.equal(st.n, torch.tensor(one[:, 3], device=dev))
    k = R.bin_index(R.z_factored(rb.zq1.cpu().numpy(), rb.pix_ratio.cpu().numpy()), st.z0, st.dz, 9)
    iv = iv.cpu().numpy()
    _, asum = R.stack_of(tr.cpu().numpy(), iv, iv != 0, k, 9)
    assert (np.abs(got - one) <= one[:, 3:4] * U64 * asum).all()
