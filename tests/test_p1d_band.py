"""Band powers of the P1D and their covariance stack on the MI355X (QFA.p1d_bands / band_power, qfa_p1d_band_f32) against the numpy
port (tests/_p1d_band_ref.py) working from the power / noise qfa_p1d_f32 returns on the same inputs -- the existing call's bits, not
a second DFT.

Bars (derived in tests/_p1d_band_ref.py): Q_a within (n_a + 2) 2^-53 sum_m |w_m| (|P_m| + |N|); sum Q_a and sum Q_a Q_b within
(n + 3) 2^-53 sum |terms| plus the propagated bar of Q; counts, zeros of invalid segments and the symmetry of the matrix exact.
Inputs: tests/test_p1d.py's forest_case (20 % masks), NaN put under every unused pixel."""
import os
import sys

import numpy as np
import pytest

import _p1d_band_ref as RB
import _p1d_ref as R
from conftest import REPO
from _segment_harness import (F_SYNC as SYNC, F_ZERO as ZERO, TB_BINS, T, call_p1d as call_c, call_segment, cli_predict_case, dev,  # noqa: F401 (dev: the fixture)
                              forest_case, loader_case, redshift_forms, tbar_range, two_ranks)

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53


def masked_case(dev, B, S, nb, seed):
    """forest_case with NaN under every unused pixel: nothing under the mask may reach an output"""
    import torch
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed)
    tr = torch.where(iv > 0, tr, torch.full_like(tr, float("nan"))).contiguous()
    return g, m, tr, iv, tbar


def call_band(dev, trans, ivar, tbar, prm, band, weight, sub, *, flags=ZERO | SYNC, **kw):
    """qfa_p1d_band_f32 by hand; prm = (p_lo, L, nseg, min_used, (z0, dz, nz)); band (M,) ints, weight (M,) or None.  Returns
    (bandpower, stack) as numpy"""
    import torch
    from qfa_amd import _lib
    nband = int(max(np.max(band, initial=0), 0)) + 1 if not isinstance(band, tuple) else band[1]
    band = band[0] if isinstance(band, tuple) else band
    bd = torch.tensor(np.append(np.asarray(band, np.int32), np.int32(-1)), device=dev)          # (never empty: L = 1 has M = 0)
    wd = None if weight is None else torch.tensor(np.append(np.asarray(weight, np.float32), np.float32(0)), device=dev)
    qq = _lib.P1DBandParams(nband, bd.data_ptr(), None if wd is None else wd.data_ptr(), sub)
    return call_segment("qfa_p1d_band", dev, trans, ivar, tbar, prm, qq, (("b", (nband,), "float64"),), size=(nband,),
                        stack_width=1 + nband + nband * nband, flags=flags, **kw)


def reference(dev, g, tr, iv, tbar, prm, band, nband, weight, sub):
    """the port on the bits qfa_p1d_f32 writes for the same inputs; validity and z-bins from the port of that contract"""
    p_lo, L, nseg, min_used, bins = prm
    power, noise, _ = call_c(dev, tr, iv, tbar, prm, zabs=T(g["zabs"], dev), outs="pn")
    with np.errstate(all="ignore"):
        r = R.p1d(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, bins)
    assert np.array_equal(noise != 0, r["valid"])
    Q, dQ = RB.band_q(power, noise, band, weight, sub, nband)
    stack, bar = RB.stack_of(Q, dQ, r["valid"], r["kz"], bins[2])
    return {"power": power, "noise": noise, "valid": r["valid"], "kz": r["kz"], "Q": Q, "dQ": dQ, "stack": stack, "bar": bar}


def check(bp, stack, ref, nband, what):
    """bandpower and stack inside their bars; counts, invalid rows and the symmetry exact.  Prints the worst fraction of each bar"""
    assert (bp[~ref["valid"]] == 0).all() and not np.signbit(bp[~ref["valid"]]).any(), what
    eQ = np.abs(bp - ref["Q"])
    assert (eQ <= ref["dQ"]).all(), (what, "Q", (eQ / ref["dQ"].clip(1e-300)).max())
    assert np.array_equal(stack[:, :, 0], ref["stack"][:, :, 0]), (what, "counts")
    eS = np.abs(stack - ref["stack"])
    assert (eS <= ref["bar"]).all(), (what, "stack", (eS / ref["bar"].clip(1e-300)).max())
    mat = stack[:, :, 1 + nband:].reshape(stack.shape[:2] + (nband, nband))
    assert np.array_equal(mat, mat.transpose(0, 1, 3, 2)), (what, "symmetry")
    fq = (eQ / ref["dQ"].clip(1e-300))[ref["dQ"] > 0].max(initial=0.0)
    fs = (eS / ref["bar"].clip(1e-300))[ref["bar"] > 0].max(initial=0.0)
    print(f"p1d_band accuracy: {what}: max |dQ| / bar = {fq:.4f}, max |d stack| / bar = {fs:.4f}")


def band_for(L, nband):
    """the band arrays of the cases: (band (M,), nband)"""
    M = L // 2
    if L == 37 and nband == 5:        # band 2 empty, modes 1 and 12 in no band (-1 and 9), band 0 not contiguous
        return np.array([-1, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 9, 4, 4, 4, 4, 4, 0], np.int32), 5
    if nband == M:                    # one mode per band, in another order than the modes
        return np.random.default_rng(L).permutation(M).astype(np.int32), nband
    return ((np.arange(M) * nband) // max(M, 1)).astype(np.int32), nband


def chunk():
    from qfa_amd import _lib
    return _lib.lib().qfa_p1d_band_chunk_segments()


# rows, S, L, nseg, nband, nz, weighted, subtract_noise; the last: segments per draw = two chunks and a ragged tail
CASES = [(15, 1, 1, 2, 1, 1, False, 1), (1, 1, 13, 3, 1, 7, True, 1), (15, 3, 37, 2, 5, 7, True, 1), (17, 1, 128, 1, 64, 1, False, 0),
         (17, 1, 240, 2, 17, 7, True, 1), ("2 chunks + 5", 2, 13, 1, 3, 7, True, 0)]


@pytest.mark.parametrize("rows,S,L,nseg,nband,nz,weighted,sub", CASES)
def test_bandpower_and_stack_match_the_port(dev, rows, S, L, nseg, nband, nz, weighted, sub):
    B = (2 * chunk() + 5) if isinstance(rows, str) else rows // S
    nb = 2 + nseg * L + 3
    g, m, tr, iv, tbar = masked_case(dev, B, S, nb, seed=2000 + L + nband)
    min_used = max(1, int(np.ceil(0.78 * L)))
    bins = (2.3, 0.5, 1) if nz == 1 else (2.0, 0.12, 7)                            # z lies in [1.54, 3.5]: segments fall outside both
    prm = (2, L, nseg, min_used, bins)
    band, nband = band_for(L, nband)
    weight = None
    if weighted:
        weight = np.random.default_rng(L).uniform(0.5, 2.0, L // 2).astype(np.float32)
        weight[::5] *= -1                                                          # (signs too: the bar sums |w|)
    ref = reference(dev, g, tr, iv, tbar, prm, band, nband, weight, sub)
    bp, stack = call_band(dev, tr, iv, tbar, prm, (band, nband), weight, sub, zabs=T(g["zabs"], dev))
    what = f"rows {rows} S {S} L {L} nseg {nseg} nband {nband} nz {nz}"
    inbin = ref["valid"] & (ref["kz"] >= 0)[:, None, :]
    if L > 1 and B * nseg >= 15:                                                   # both sides of min_used and of the bins
        assert ref["valid"].any() and not ref["valid"].all() and inbin.any() and (ref["valid"] & ~inbin).any(), what
    if L == 1:
        assert (bp == 0).all() and (stack[:, :, 1:] == 0).all() and stack[:, :, 0].sum() == inbin.sum() > 0   # M = 0: n still counted
    if L == 37:
        assert (bp[..., 2] == 0).all()                                             # the empty band
    check(bp, stack, ref, nband, what)


def test_one_mode_per_band_is_the_existing_stack(dev):
    """L = 128, band m = mode m, no weights, noise kept: n is P1DStack's n exactly, sum Q_a and the diagonal of sum Q Q^T are
    qfa_p1d_f32's sum P and sum P^2 within the bar of two float64 sums of n terms in different orders: 2 n 2^-53 sum |terms|"""
    B, S, L, nseg = 40, 2, 128, 2
    g, m, tr, iv, tbar = masked_case(dev, B, S, 2 + nseg * L, seed=51)
    prm = (1, L, nseg, 100, (1.7, 0.2, 7))
    M = L // 2
    z = T(g["zabs"], dev)
    _, _, old = call_c(dev, tr, iv, tbar, prm, zabs=z, flags=ZERO, outs="s")
    bp, new = call_band(dev, tr, iv, tbar, prm, (np.arange(M, dtype=np.int32), M), None, 0, zabs=z)
    n = old[:, :, :1]
    assert np.array_equal(new[:, :, 0], old[:, :, 0]) and n.sum() > 30
    sP, sPP = old[:, :, 2:2 + M], old[:, :, 2 + M:]
    assert (np.abs(new[:, :, 1:1 + M] - sP) <= 2 * n * U64 * sP).all()
    diag = np.diagonal(new[:, :, 1 + M:].reshape(S, 7, M, M), axis1=2, axis2=3)
    assert (np.abs(diag - sPP) <= 2 * n * U64 * sPP).all()
    power, _, _ = call_c(dev, tr, iv, tbar, prm, zabs=z, outs="pn")
    assert np.array_equal(bp, power.astype(np.float64))                            # Q_a = 0 + 1 (P_a - 0 N) = P_a to the bit


def test_redshift_forms_give_identical_bits(dev):
    B, S, nb, L, nseg, p_lo = 9, 2, 80, 37, 2, 4
    g, m, tr, iv, tbar = masked_case(dev, B, S, nb, seed=21)
    prm = (p_lo, L, nseg, 25, (1.6, 0.45, 4))
    band = band_for(L, 5)
    a, *others = (call_band(dev, tr, iv, tbar, prm, band, None, 1, **kw) for kw in redshift_forms(dev, g, B, nb)[1][:3])
    assert a[1][:, :, 0].sum() > 0
    for other in others:
        for x, y in zip(a, other):
            assert np.array_equal(x, y)


def test_adds_overwrites_repeats_and_leaves_p1d_alone(dev):
    """ADD against QFA_F_ZERO_ACCUM, either output alone, a repeated call, and qfa_p1d_f32 before and after a band call (the two
    share the model's workspace in QFA; here each call brings its own, and the bits of the existing call may not move)"""
    import torch
    B, S, nb, L, nseg = 50, 2, 64, 21, 3
    g, m, tr, iv, tbar = masked_case(dev, B, S, nb, seed=41)
    bins = (1.6, 0.45, 4)
    prm = (0, L, nseg, 15, bins)
    z = T(g["zabs"], dev)
    band = band_for(L, 4)
    before = call_c(dev, tr, iv, tbar, prm, zabs=z, flags=ZERO)
    bp, stack = call_band(dev, tr, iv, tbar, prm, band, None, 1, zabs=z)
    after = call_c(dev, tr, iv, tbar, prm, zabs=z, flags=ZERO)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert stack[:, :, 0].sum() > chunk() * S                                      # more than one chunk per draw
    again = call_band(dev, tr, iv, tbar, prm, band, None, 1, zabs=z)
    assert np.array_equal(again[0], bp) and np.array_equal(again[1], stack)
    only_s = call_band(dev, tr, iv, tbar, prm, band, None, 1, zabs=z, outs="s")
    only_b = call_band(dev, tr, iv, tbar, prm, band, None, 1, zabs=z, outs="b")
    assert only_s[0] is None and np.array_equal(only_s[1], stack) and only_b[1] is None and np.array_equal(only_b[0], bp)
    acc = torch.tensor(stack, device=dev)
    added = call_band(dev, tr, iv, tbar, prm, band, None, 1, zabs=z, flags=SYNC, stack=acc)[1]
    assert np.array_equal(added[:, :, 0], 2 * stack[:, :, 0]) and not np.array_equal(added, stack)
    # the sum continues from what the stack held: the held value is within `bar` of the port's, the new terms bring their own
    # `bar`, and every one of the at most n additions that round now rounds a partial sum of at most twice sum |terms|: 2 bar more
    ref = reference(dev, g, tr, iv, tbar, prm, band[0], band[1], None, 1)
    assert (np.abs(stack - ref["stack"]) <= ref["bar"]).all()
    assert (np.abs(added - 2 * ref["stack"]) <= 4 * ref["bar"]).all()
    mat = added[:, :, 5:].reshape(S, 4, 4, 4)
    assert np.array_equal(mat, mat.transpose(0, 1, 3, 2))
    # B = 0: nothing happens without the flag, zeros under it
    held = torch.full_like(acc, 5.0)
    kw = dict(zabs=z, outs="s", stack=held, nrows=0)
    assert np.array_equal(call_band(dev, tr, iv, tbar, prm, band, None, 1, flags=SYNC, **kw)[1], np.full(acc.shape, 5.0))
    assert (call_band(dev, tr, iv, tbar, prm, band, None, 1, flags=ZERO | SYNC, **kw)[1] == 0).all()


def test_draw_s_of_a_call_is_the_call_on_that_draw_alone(dev):
    B, S, nb, L, nseg = 70, 3, 100, 48, 2
    g, m, tr, iv, tbar = masked_case(dev, B, S, nb, seed=31)
    prm = (2, L, nseg, 36, (1.6, 0.45, 4))
    z = T(g["zabs"], dev)
    band = band_for(L, 6)
    w = np.linspace(0.5, 1.5, L // 2).astype(np.float32)
    for tb in (tbar, tbar[1:2]):
        bp, stack = call_band(dev, tr, iv, tb, prm, band, w, 1, zabs=z)
        assert stack[:, :, 0].sum() > chunk()
        for s in range(S):
            one = call_band(dev, tr[:, s:s + 1].contiguous(), iv[:, s:s + 1].contiguous(), tb[s:s + 1] if tb.shape[0] == S else tb, prm,
                            band, w, 1, zabs=z)
            assert np.array_equal(one[0][:, 0], bp[:, s]) and np.array_equal(one[1][0], stack[s]), s


BP_KW = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, seed=6)


def _edges(dv):
    from qfa_amd.model import P1DBandStack
    return P1DBandStack.linear_k_edges(24, dv, 4)


def test_band_power_of_a_loader(dev):
    """band_power against the port on the concatenated batches (p1d on the whole loader in one call gives P and N), two batch sizes
    within the float64 summation bar, and flux_power's bits untouched by the shared loop"""
    import torch
    m, mk, wav = loader_case(dev)
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    edges = _edges(dv)
    for S in (0, 3):
        a = m.band_power(mk(96), 1.8, 3.4, 3, edges, n_samples=S, batch_size=96, **BP_KW)
        c = m.band_power(mk(96), 1.8, 3.4, 3, edges, n_samples=S, batch_size=40, **BP_KW)
        fp = m.flux_power(mk(96), 1.8, 3.4, 3, n_samples=S, batch_size=96, **BP_KW)
        assert a.S == max(1, S) and a.nband == 4 and torch.equal(a.n, c.n) and torch.equal(a.n, fp.n) and a.n.sum() > 20 * a.S
        x, y = a.buf.cpu().numpy(), c.buf.cpu().numpy()
        n = x[:, :, :1]
        # the same terms in another grouping: (n + 3) 2^-53 sum |terms| each, and sum |terms| <= sqrt(sum Q_a^2 sum Q_b^2)
        d = np.sqrt(np.diagonal(x[:, :, 5:].reshape(a.S, 3, 4, 4), axis1=2, axis2=3))
        sabs = np.concatenate([n, np.sqrt(n) * d, (d[..., :, None] * d[..., None, :]).reshape(a.S, 3, 16)], -1)
        assert (np.abs(x - y) <= 2 * (n + 3) * U64 * sabs).all(), S
        # the band means are flux_power's P1D averaged over the band's modes (float32 weights: 1e-6)
        band, count = a.band_map()
        P = fp.power().cpu().numpy()
        want = np.stack([P[:, :, band == k].mean(-1) for k in range(4)], -1)
        ok = (a.n > 1).cpu().numpy()
        assert np.allclose(a.mean.cpu().numpy()[ok], want[ok], rtol=1e-5, atol=1e-6 * np.abs(want[ok]).max())
        assert torch.isfinite(a.cov[a.n > 1]).all() and (torch.diagonal(a.cov, dim1=2, dim2=3)[a.n > 1] > 0).all()
    assert a.cov_over_draws.shape == (3, 4, 4) and a.total_cov.shape == (3, 4, 4)
    # against the port: one slice by hand, bandpower of every segment from p1d's own power / noise
    dl = mk(96)
    one = m.band_power(dl, 1.8, 3.4, 3, edges, batch_size=96, **BP_KW)
    half = float(np.exp(0.5 * 25 * dv / 299792.458))
    tb1 = m.mean_transmission(dl, 2.8 / half - 1.0, 4.4 * half - 1.0, 8, batch_size=96)
    for _, inputs, _ in m._loader_slices(dl, 96):
        _, hm, _, _, unc = m.predict(**inputs)
        tr, iv, _ = m.forest(**inputs, hmean=hm, unc=unc)
        zin = {"batch": inputs["batch"]} if "batch" in inputs else {"zabs": inputs["zabs"]}
        kw = dict(tbar=tb1, seg_len=24, n_segments=2, min_used=18, bins=one.bins, dv=dv)
        pw, ns, pst = m.p1d(tr, iv, **zin, **kw)
        bp, st = m.p1d_bands(tr, iv, **zin, **kw, k_edges=edges, return_segments=True)
        pw2, ns2, pst2 = m.p1d(tr, iv, **zin, **kw)                                # the shared workspace does no harm
    assert torch.equal(pw, pw2) and torch.equal(ns, ns2) and torch.equal(pst.buf, pst2.buf)
    assert torch.equal(st.buf, one.buf) and bp.shape == (96, 1, 2, 4)
    band, _ = RB.band_map(24, dv, edges)
    Q, dQ = RB.band_q(pw.cpu().numpy(), ns.cpu().numpy(), band, RB.weights(24, dv, edges), 1, 4)
    assert (np.abs(bp.cpu().numpy() - Q) <= dQ).all()
    valid = ns.cpu().numpy() != 0
    # the z of the central pixels as the call formed it: the slice's zabs, or the loader's factors through one fma
    z = zin["zabs"].cpu().numpy() if "zabs" in zin else R.z_factored(dl._zq1_dev.cpu().numpy(), dl._pix_ratio.cpu().numpy())
    kzs = R.bin_index(z[:, np.arange(2) * 24 + 12], *one.bins)
    port, bar = RB.stack_of(Q, dQ, valid, kzs, 3)
    got = one.buf.cpu().numpy()
    assert np.array_equal(port[:, :, 0], got[:, :, 0]) and (np.abs(got - port) <= bar).all()
    print(f"p1d_band accuracy: band_power of a loader: max |d stack| / bar = {(np.abs(got - port) / bar.clip(1e-300))[bar > 0].max():.4f}")


# ------------------------------------------------------------------------------------------------------------ data parallel
DP_KW = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, n_samples=2, seed=6, batch_size=40)


def _worker_band_power(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    m, mk, wav = loader_case(dev, rank=rank, world=world)
    m.enable_data_parallel()
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    tb = m.mean_transmission(mk(40), *tbar_range(dv), 8, n_samples=2, seed=6, batch_size=40)
    ps = m.band_power(mk(40), 1.8, 3.4, 3, _edges(dv), tbar=tb, **DP_KW)
    if rank == 0:
        q.put(np.concatenate([ps.buf.cpu().numpy().ravel(), tb.buf.cpu().numpy().ravel()]))
    dist.destroy_process_group()


def test_two_ranks_all_reduce_to_the_single_process_stack(dev):
    """band_power on two ranks against one process, both forming the contrast with the same all-reduced <T>: the stacks are sums
    of the same terms in another grouping"""
    import torch
    from qfa_amd.model import ForestStack
    got = two_ranks(_worker_band_power, 33500)
    m, mk, wav = loader_case(dev)
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    n1 = 2 * 3 * 21
    two, tbuf = got[:n1].reshape(2, 3, 21), got[n1:].reshape(2, 4, 8)
    z_lo, z_hi = tbar_range(dv)
    tb = ForestStack(torch.tensor(tbuf, device=dev), z_lo, (z_hi - z_lo) / 8, 8)
    one = m.band_power(mk(40), 1.8, 3.4, 3, _edges(dv), tbar=tb, **DP_KW).buf.cpu().numpy()
    assert np.array_equal(two[:, :, 0], one[:, :, 0]) and one[:, :, 0].sum() > 40
    n = one[:, :, :1]
    d = np.sqrt(np.diagonal(one[:, :, 5:].reshape(2, 3, 4, 4), axis1=2, axis2=3))
    sabs = np.concatenate([n, np.sqrt(n) * d, (d[..., :, None] * d[..., None, :]).reshape(2, 3, 16)], -1)
    assert (np.abs(two - one) <= 2 * (n + 3) * U64 * sabs).all()


def test_cli_predict_writes_flux_power_bands_npz(dev, tmp_path):
    from qfa_amd import cli
    c = cli_predict_case(dev, tmp_path)
    for S, out in ((2, tmp_path / "out2"), (0, tmp_path / "out0")):
        argv = c.argv(out, "MODEL.N_SAMPLES", str(S), "MODEL.P1D_NBANDS", "5")
        assert cli.main(argv) == 0
        f, old = np.load(out / "flux_power_bands.npz"), np.load(out / "flux_power.npz")
        keys = {"k_edges", "k_centers", "z_edges", "n", "mean", "cov"} | ({"cov_over_draws"} if S > 1 else set())
        assert set(f.files) == keys
        Sd = max(1, S)
        assert f["k_edges"].shape == (6,) and f["k_centers"].shape == (5,) and f["z_edges"].shape == (4,)
        assert f["n"].shape == (Sd, 3) and f["mean"].shape == (Sd, 3, 5) and f["cov"].shape == (Sd, 3, 5, 5)
        assert np.array_equal(f["n"], old["n"]) and f["n"].sum() > 10 and np.isfinite(f["cov"][f["n"] > 1]).all()
        assert np.array_equal(f["cov"], f["cov"].transpose(0, 1, 3, 2), equal_nan=True)
        assert f["k_edges"][0] < old["k"][0] and old["k"][-1] < f["k_edges"][-1]
        if S > 1:
            assert f["cov_over_draws"].shape == (3, 5, 5)
