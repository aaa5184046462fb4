"""The 1D flux power spectrum of forest segments and its stack on the MI355X (QFA.p1d / flux_power, qfa_p1d_f32) against the numpy
port of the contract (tests/_p1d_ref.py).

Bars (derived in tests/_p1d_ref.py): per mode |dP_m| <= (2 |X_m| e + e^2) / L + 4 u P_m with e = (2L + 8) u sum_j |d_j|; noise
(L + 4) u N; the valid / invalid pattern is exact, the port working on the very trans / ivar the GPU read.  Stack: N 2^-53 sum
|terms| per entry against float64 sums of the GPU's own power / noise, counts exact.  The inputs are the transmission and inverse
variance QFA.forest writes for tests/test_forest.py's `geometry` (continuum in [0.5, 2], 20 % masks)."""
import os
import sys

import numpy as np
import pytest

import _p1d_ref as R
from conftest import REPO
from _segment_harness import (TB_BINS, T, call_p1d as call_c, cli_predict_case, dev, forest_case, loader_case,  # noqa: F401 (dev: the fixture)
                              make_model, redshift_forms, tbar_range, two_ranks)

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53


def check_segments(power, noise, ref, L, what):
    """every mode of every segment inside power_bound, noise inside noise_bound, the valid pattern exact"""
    valid = ref["valid"]
    assert np.array_equal(noise != 0, valid), what                                    # (N > 0 on every valid segment)
    assert (power[~valid] == 0).all() and (noise[~valid] == 0).all(), what
    eP, bP = np.abs(power.astype(np.float64) - ref["P"]), R.power_bound(ref, L)
    eN, bN = np.abs(noise.astype(np.float64) - ref["N"]), R.noise_bound(ref, L)
    if valid.any() and L > 1:
        print(f"{what}: max |dP| / bound = {(eP[valid] / bP[valid].clip(1e-300)).max():.3f}, "
              f"max |dN| / bound = {(eN[valid] / bN[valid]).max():.3f}")
    assert (eP <= bP).all(), (what, "power")
    assert (eN <= bN).all(), (what, "noise")


def check_stack(got, power, noise, ref, nz, what):
    """against float64 sums of the GPU's own power / noise under the port's bins: N 2^-53 sum |terms|; counts exact"""
    own, own_abs = R.stack_of(power, noise, ref["valid"], ref["kz"], nz)
    assert np.array_equal(got[:, :, 0], ref["stack"][:, :, 0]), (what, "counts")
    assert (np.abs(got - own) <= got[:, :, :1] * U64 * own_abs).all(), (what, np.abs(got - own).max())


CASES = [(1, 1, 1, 0), (3, 2, 2, 1), (17, 37, 3, 5), (33, 64, 2, 0), (16, 240, 3, 0), (5, 667, 1, 3)]


@pytest.mark.parametrize("rows,L,nseg,p_lo", CASES)
def test_every_mode_of_every_segment_matches_the_port(dev, rows, L, nseg, p_lo):
    S = 3 if rows % 3 == 0 and rows > 3 else 1
    B, nb = rows // S, p_lo + nseg * L + 3                                            # pixels are left over after the last segment
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=1000 + L)
    min_used = max(1, int(np.ceil(0.78 * L)))                                         # (20 % masks: segments on both sides of it)
    bins = (1.6, 0.45, 4)
    prm = (p_lo, L, nseg, min_used, bins)
    ref = R.p1d(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, bins)
    power, noise, stack = call_c(dev, tr, iv, tbar, prm, zabs=T(g["zabs"], dev))
    what = f"rows {rows} (B {B} S {S}) L {L} nseg {nseg} p_lo {p_lo}"
    if L >= 37:
        assert ref["valid"].any() and (rows < 16 or not ref["valid"].all()), what
    check_segments(power, noise, ref, L, what)
    check_stack(stack, power, noise, ref, bins[2], what)


def test_redshift_forms_give_identical_bits(dev):
    """zabs, the factored pair and the resident `rows` form on identical z: identical power, noise and stack"""
    B, S, nb, L, nseg, p_lo = 9, 2, 80, 37, 2, 4
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=21)
    prm = (p_lo, L, nseg, 25, (1.6, 0.45, 4))
    a, *others = (call_c(dev, tr, iv, tbar, prm, **kw) for kw in redshift_forms(dev, g, B, nb)[1])
    assert a[2][:, :, 0].sum() > 0
    for other in others:
        for x, y in zip(a, other):
            assert np.array_equal(x, y)


def test_min_used_masks_junk_and_bins(dev):
    """L = 8, one segment per spectrum from pixel 1 on, min_used = 5, unit tbar except two bins that hold 0 and NaN"""
    L, nb, min_used = 8, 10, 5
    rng = np.random.default_rng(5)
    B = 7
    trans = rng.uniform(0.2, 1.2, (B, 1, nb)).astype(np.float32)
    ivar = rng.uniform(10.0, 100.0, (B, 1, nb)).astype(np.float32)
    z = np.tile(np.linspace(2.0, 2.09, nb, dtype=np.float32), (B, 1))                  # one tbar bin [2, 2.125) unless moved
    ivar[0, 0, 1:5] = 0                                                               # 0: min_used - 1 pixels used
    ivar[1, 0, 1:4] = 0                                                               # 1: exactly min_used
    ivar[2, 0, :] = 0                                                                 # 2: every pixel masked
    ivar[3, 0, 2:4] = 0                                                               # 3: junk under ivar == 0
    trans[3, 0, 2], trans[3, 0, 3] = np.nan, -999.0
    z[4] += 0.25                                                                      # 4: pixels in the bin that holds 0
    z[5] += 0.375                                                                     # 5: ... that holds NaN
    z[6] += 1.0                                                                       # 6: valid, zc outside the stack's bins
    tbar = np.ones((1, TB_BINS[2]), np.float32)
    tbar[0, 6], tbar[0, 7] = 0.0, np.nan                                              # [2.25, 2.375), [2.375, 2.5)
    bins = (2.0, 0.25, 2)
    prm = (1, L, 1, min_used, bins)
    ref = R.p1d(trans, ivar, z, tbar, TB_BINS, 1, L, 1, min_used, bins)
    assert ref["n_used"][:, 0, 0].tolist() == [4, 5, 0, 6, 0, 0, 8] and ref["kz"][:, 0].tolist() == [0, 0, 0, 0, 1, 1, -1]
    power, noise, stack = call_c(dev, T(trans, dev), T(ivar, dev), tbar, prm, zabs=T(z, dev))
    assert np.isfinite(power).all() and np.isfinite(noise).all() and np.isfinite(stack).all()
    check_segments(power, noise, ref, L, "edge cases")
    for b in (0, 2, 4, 5):
        assert (power[b] == 0).all() and noise[b, 0, 0] == 0, b
    for b in (1, 3, 6):
        assert (power[b] > 0).any() and noise[b, 0, 0] > 0, b
    assert stack[0, :, 0].tolist() == [2.0, 0.0] and (stack[0, 1] == 0).all()          # 1 and 3 are stacked, 6 is not
    check_stack(stack, power, noise, ref, 2, "edge cases")
    # the junk changes nothing: the same bits with zeros in its place
    clean = trans.copy()
    clean[3, 0, 2:4] = 0
    again = call_c(dev, T(clean, dev), T(ivar, dev), tbar, prm, zabs=T(z, dev))
    assert all(np.array_equal(x, y) for x, y in zip((power, noise, stack), again))


def test_draws_use_their_own_row_of_tbar(dev):
    """S = 3 with St = 3 and St = 1: draw s uses row s (or the one row), and its stack is bit for bit the stack of a call on that
    draw's rows alone"""
    B, S, nb, L, nseg = 20, 3, 100, 48, 2
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=31)
    prm = (2, L, nseg, 36, (1.6, 0.45, 4))
    z = T(g["zabs"], dev)
    for tb in (tbar, tbar[1:2]):
        power, noise, stack = call_c(dev, tr, iv, tb, prm, zabs=z)
        ref = R.p1d(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tb, TB_BINS, 2, L, nseg, 36, prm[4])
        check_segments(power, noise, ref, L, f"St = {tb.shape[0]}")
        assert stack[:, :, 0].sum() > 0
        for s in range(S):
            one = call_c(dev, tr[:, s:s + 1].contiguous(), iv[:, s:s + 1].contiguous(), tb[s:s + 1] if tb.shape[0] == S else tb, prm, zabs=z)
            assert np.array_equal(one[0][:, 0], power[:, s]) and np.array_equal(one[1][:, 0], noise[:, s])
            assert np.array_equal(one[2][0], stack[s]), s
    assert not np.array_equal(call_c(dev, tr, iv, tbar, prm, zabs=z)[0][:, 0], call_c(dev, tr, iv, tbar[1:2], prm, zabs=z)[0][:, 0])


def test_stack_adds_overwrites_and_repeats(dev):
    """more segments per draw than one scan of the reducer covers; ADD against QFA_F_ZERO_ACCUM; any subset of the outputs; two
    calls give the same bits"""
    import torch
    B, S, nb, L, nseg = 50, 2, 64, 21, 3
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=41)
    bins = (1.6, 0.45, 4)
    prm = (0, L, nseg, 15, bins)
    z = T(g["zabs"], dev)
    ref = R.p1d(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, 0, L, nseg, 15, bins)
    power, noise, stack = call_c(dev, tr, iv, tbar, prm, zabs=z)
    assert ref["stack"][:, :, 0].sum() > 64 * S
    check_stack(stack, power, noise, ref, bins[2], "stack")
    again = call_c(dev, tr, iv, tbar, prm, zabs=z)
    assert all(np.array_equal(x, y) for x, y in zip((power, noise, stack), again))
    only = call_c(dev, tr, iv, tbar, prm, zabs=z, outs="s")                           # rows through the workspace: the same sums
    assert only[0] is None and only[1] is None and np.array_equal(only[2], stack)
    pn = call_c(dev, tr, iv, tbar, prm, zabs=z, outs="pn")
    assert pn[2] is None and np.array_equal(pn[0], power) and np.array_equal(pn[1], noise)
    # ADD: onto a stack that holds `stack` already -- the sum continues from it, segment by segment
    acc = torch.tensor(stack, device=dev)
    added = call_c(dev, tr, iv, tbar, prm, zabs=z, flags=0, stack=acc)[2]
    assert np.array_equal(added[:, :, 0], 2 * stack[:, :, 0])
    n = stack[:, :, :1]
    assert (np.abs(added - 2 * stack) <= 2 * n * U64 * 2 * stack).all() and not np.array_equal(added, stack)


def test_injected_cosine(dev):
    """d_j = a cos(2 pi j m0 / L) exactly at unit tbar: P_m0 = a^2 L / 4, every other mode 0, inside power_bound"""
    L, m0, nb = 64, 5, 70
    amps = np.array([0.5, 0.01, 2.0], np.float32)
    j = np.arange(L)
    d = (amps[:, None].astype(np.float64) * np.cos(2 * np.pi * ((j * m0) % L) / L)[None, :]).astype(np.float32)
    trans = np.ones((3, 1, nb), np.float32)
    trans[:, 0, 3:3 + L] = (d + np.float32(1.0)).astype(np.float32)
    ivar = np.full((3, 1, nb), 25.0, np.float32)
    z = np.full((3, nb), 2.05, np.float32)
    tbar = np.ones((1, TB_BINS[2]), np.float32)
    bins = (2.0, 0.25, 2)
    ref = R.p1d(trans, ivar, z, tbar, TB_BINS, 3, L, 1, L, bins)
    power, noise, _ = call_c(dev, T(trans, dev), T(ivar, dev), tbar, (3, L, 1, L, bins), zabs=T(z, dev))
    bound = R.power_bound(ref, L)[:, 0, 0]                                            # (3, M)
    dd = ref["d"][:, 0, 0]                                                            # what T - 1 is in float32
    exact = np.abs(dd @ R.dft_matrix(L)) ** 2 / L
    want = np.zeros_like(exact)
    want[:, m0 - 1] = amps.astype(np.float64) ** 2 * L / 4
    # (1 + d) - 1 in float32 moves d by at most u (1 + |d|) per pixel: the port's own distance from the ideal signal is inside
    # 2 |X| L u (1 + a) / L + ... -- asserted on the port, so that the GPU is held to power_bound of the ideal values plus that
    slack = np.abs(exact - want)
    assert (slack <= (2 * np.sqrt(want * L) + 1) * (1 + amps[:, None]) * L * R.U / L + 1e-300 + 4 * R.U * want).all()
    got = power[:, 0, 0].astype(np.float64)
    assert (np.abs(got - want) <= bound + slack).all(), np.abs(got - want).max()
    assert (np.abs(got[:, m0 - 1] - want[:, m0 - 1]) <= 1e-5 * want[:, m0 - 1]).all()
    assert (noise[:, 0, 0] == np.float32(1.0) / np.float32(25.0)).all()


def test_flux_power_of_a_loader(dev):
    import torch
    m, mk, wav = loader_case(dev)
    kw = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, seed=6)
    for S in (0, 4):
        a = m.flux_power(mk(96), 1.8, 3.4, 3, n_samples=S, batch_size=96, **kw)
        c = m.flux_power(mk(96), 1.8, 3.4, 3, n_samples=S, batch_size=40, **kw)
        assert a.S == max(1, S) and a.L == 24 and a.M == 12 and torch.equal(a.n, c.n) and a.n.sum() > 20 * a.S
        assert np.isclose(a.dv, 299792.458 * np.log(wav[1] / wav[0]))
        x, y = a.buf.cpu().numpy(), c.buf.cpu().numpy()
        assert (np.abs(x - y) <= 1e-12 * np.abs(y)).all(), S
        assert torch.isfinite(a.power()[a.n > 1]).all() and torch.isfinite(a.err()[a.n > 1]).all()
    assert a.std_over_draws.shape == (3, 12) and (a.std_over_draws[a.n[0] > 1] > 0).all()
    # draw s of <T> is draw s of T: flux_power given the mean transmission of the same seeds returns the same bits ...
    half = float(np.exp(0.5 * 25 * a.dv / 299792.458))
    tb = m.mean_transmission(mk(96), 2.8 / half - 1.0, 4.4 * half - 1.0, 8, n_samples=4, seed=6, batch_size=96)
    assert tb.S == 4 and torch.equal(m.flux_power(mk(96), 1.8, 3.4, 3, n_samples=4, batch_size=96, tbar=tb, **kw).buf, a.buf)
    # ... and of another seed does not
    tb2 = m.mean_transmission(mk(96), 2.8 / half - 1.0, 4.4 * half - 1.0, 8, n_samples=4, seed=7, batch_size=96)
    assert not torch.equal(m.flux_power(mk(96), 1.8, 3.4, 3, n_samples=4, batch_size=96, tbar=tb2, **kw).buf, a.buf)
    # p1d by hand on one slice, with a ForestStack for tbar, adds up to the same stack (S = 1)
    dl = mk(96)
    one = m.flux_power(dl, 1.8, 3.4, 3, batch_size=96, **kw)
    tb1 = m.mean_transmission(dl, 2.8 / half - 1.0, 4.4 * half - 1.0, 8, batch_size=96)
    for _, inputs, _ in m._loader_slices(dl, 96):
        _, hm, _, _, unc = m.predict(**inputs)
        tr, iv, _ = m.forest(**inputs, hmean=hm, unc=unc)
        zin = {"batch": inputs["batch"]} if "batch" in inputs else {"zabs": inputs["zabs"]}
        pw, ns, st = m.p1d(tr, iv, **zin, tbar=tb1, seg_len=24, n_segments=2, min_used=18, bins=one.bins, dv=one.dv)
    assert pw.shape == (96, 1, 2, 12) and ns.shape == (96, 1, 2) and torch.equal(st.buf, one.buf)


# ------------------------------------------------------------------------------------------------------------ data parallel
FP_KW = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, n_samples=2, seed=6, batch_size=40)


def _worker_flux_power(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    m, mk, wav = loader_case(dev, rank=rank, world=world)
    m.enable_data_parallel()
    ps = m.flux_power(mk(40), 1.8, 3.4, 3, **FP_KW)                                   # its own <T>, all-reduced, then its own sums
    tb = m.mean_transmission(mk(40), *tbar_range(ps.dv), 8, n_samples=2, seed=6, batch_size=40)
    if rank == 0:
        q.put(np.concatenate([ps.buf.cpu().numpy().ravel(), tb.buf.cpu().numpy().ravel()]))
    dist.destroy_process_group()


def test_two_ranks_all_reduce_to_the_single_process_stack(dev):
    """flux_power on two ranks (each walks its shard with global row numbers, then P1DStack.all_reduce) against one process.  The
    mean transmission is handed over, so that both sides form the contrast with the same float32 <T>: the stacks are then sums of
    the same terms in another grouping"""
    import torch
    from qfa_amd.model import ForestStack
    got = two_ranks(_worker_flux_power, 31500)
    m, mk, wav = loader_case(dev)
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    n1 = 2 * 3 * (2 + 2 * 12)
    two, tbuf = got[:n1].reshape(2, 3, 26), got[n1:].reshape(2, 4, 8)
    z_lo, z_hi = tbar_range(dv)
    tb = ForestStack(torch.tensor(tbuf, device=dev), z_lo, (z_hi - z_lo) / 8, 8)
    one = m.flux_power(mk(40), 1.8, 3.4, 3, tbar=tb, **FP_KW).buf.cpu().numpy()
    assert np.array_equal(two[:, :, 0], one[:, :, 0]) and one[:, :, 0].sum() > 40
    assert (np.abs(two - one) <= 1e-12 * np.abs(one)).all()


def test_cli_predict_writes_flux_power_npz(dev, tmp_path):
    """predict mode with MODEL.P1D_SEGMENTS: flux_power.npz next to mean_transmission.npz, formed with that file's stack"""
    import torch
    from qfa_amd import cli
    from qfa_amd.model import ForestStack
    c = cli_predict_case(dev, tmp_path)
    wav, npix, nb, b, names, p, mu = c.wav, c.npix, c.nb, c.b, c.names, c.p, c.mu
    out = tmp_path / "out"
    argv = c.argv(out, "MODEL.N_SAMPLES", "2")
    assert cli.main(argv) == 0
    f, t = np.load(out / "flux_power.npz"), np.load(out / "mean_transmission.npz")
    L = nb // 2
    assert int(f["seg_len"]) == L and f["sums"].shape == (2, 3, 2 + 2 * (L // 2)) and f["k"].shape == (L // 2,)
    assert f["power"].shape == f["err"].shape == f["power_raw"].shape == (2, 3, L // 2) and f["n"].shape == f["noise"].shape == (2, 3)
    assert np.isclose(float(f["dv"]), 299792.458 * np.log(wav[1] / wav[0])) and f["n"].sum() > 10
    assert np.allclose(f["z_edges"], np.float32(1.6) + np.float32(2.0 / 3) * np.arange(4))
    assert np.isfinite(f["power"][f["n"] > 1]).all()
    # the same stack from the library, handed the sums the command line wrote for <T>
    from qfa_amd.dataloader import DeviceDataloader
    dl = DeviceDataloader(b["flux"].astype(np.float64).astype(np.float32), b["error"].astype(np.float64).astype(np.float32),
                          b["zqso"], wav, 500, dev, tau="becker", mode="predict", paths=names)
    m2 = make_model(dev, {"p": p, "mu": mu}, nb, npix - nb, 4)
    tb = ForestStack(torch.tensor(t["sums"], device=dev), 1.6, 2.0 / 10, 10)
    ps = m2.flux_power(dl, 1.6, 3.6, 3, n_segments=2, min_used_frac=0.6, tbar=tb, n_samples=2, seed=0)
    mine = ps.buf.cpu().numpy()
    assert np.array_equal(mine[:, :, 0], f["sums"][:, :, 0]) and np.allclose(mine, f["sums"], rtol=1e-9, atol=0.0)
