"""GPU tests of the sightline bootstrap (include/qfa_hip.h: qfa_segment_codes_f32, qfa_bootstrap_f64; QFA.segment_codes,
segment_bootstrap, bootstrap) against the numpy restatement tests/_bootstrap_ref.py.

The bar of every float comparison is the bound of a float64 sum in any order, n_terms 2^-52 sum w |x| per element: the products w x are
exact, nothing else enters.  int32 rows must be bit-exact.  Achieved (profiles/bootstrap_accuracy.txt): the kernel adds in the
reference's order, so float32 and int32 rows give its bits (ratio 0); float64 rows, whose product w x the kernel's fma does not round
and numpy's does, reach 0.030 of the bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _bootstrap_ref as ref
from _segment_harness import (F_ZERO, TB_BINS, T, call_p1d, cli_predict_case, dev, forest_case, make_model, redshift_forms,  # noqa: F401
                              two_ranks)
from conftest import REPO

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
DT = {"float32": np.float32, "float64": np.float64, "int32": np.int32}


def run_boot(dev, rows, codes, nz, R, seed=7, off=0, flags=F_ZERO, boot=None):
    """qfa_bootstrap_f64 by hand; rows (B, S, nseg, W) and codes (B, S, nseg) numpy; returns boot (S, R, nz, 1 + W) numpy"""
    import torch
    from qfa_amd import _lib
    h = _lib.lib()
    B, S, nseg, W = rows.shape
    tr = torch.tensor(rows, device=dev).contiguous()
    tc = torch.tensor(np.asarray(codes, np.int32), device=dev).contiguous()
    out = torch.full((S, R, nz, 1 + W), 3.0, dtype=torch.float64, device=dev) if boot is None else torch.tensor(boot, device=dev)
    need = h.qfa_bootstrap_workspace_bytes(B, S, nseg, W, nz, R)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = h.qfa_bootstrap_f64(C.c_void_p(tr.data_ptr()), _lib.ROW_TYPES[rows.dtype.name], C.c_void_p(tc.data_ptr()), B, S, nseg, W, nz, R,
                             seed, off, flags, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), need, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert st == 0, st
    return out.cpu().numpy()


def make_rows(B, S, nseg, W, nz, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "int32":
        rows = rng.integers(-50, 4096, (B, S, nseg, W)).astype(np.int32)
    else:
        rows = (rng.normal(0, 1, (B, S, nseg, W)) * 10.0 ** rng.integers(-3, 4, (B, S, nseg, 1))).astype(DT[dtype])
    codes = rng.integers(-1, nz, (B, S, nseg)).astype(np.int32)
    return rows, codes


def ratio_to_bound(got, want, terms, absum):
    bound = terms[:, None, :, None] * U * absum
    err = np.abs(got - want)
    assert (err <= bound).all(), (err.max(), bound.max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nan_to_num(err / bound, nan=0.0).max())


# (B, nseg, S, W, nz, R, dtype, row_offset): B nseg = 1, 63, 64, 65, 130; W = 1, 2, 7, 17; nz = 1, 3; R = 1, 3, 4, 5, 16, 17
CASES = [(1, 1, 1, 1, 1, 1, "float32", 0), (21, 3, 1, 2, 3, 3, "float64", 0), (64, 1, 3, 7, 3, 4, "int32", (1 << 32) + 5),
         (13, 5, 1, 17, 1, 5, "float32", (1 << 32) + 5), (65, 2, 3, 7, 3, 16, "float64", 5), (130, 1, 1, 2, 3, 17, "int32", 0),
         (32, 2, 3, 17, 3, 17, "float32", 9)]
RATIOS = {}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_boot_against_the_reference(dev, case):
    B, nseg, S, W, nz, R, dtype, off = case
    rows, codes = make_rows(B, S, nseg, W, nz, dtype, 100 + B)
    got = run_boot(dev, rows, codes, nz, R, seed=0x1234567890, off=off)
    want, terms, absum = ref.bootstrap(rows, codes, nz, R, 0x1234567890, off)
    if dtype == "int32":
        assert np.array_equal(got, want)
    RATIOS[case] = ratio_to_bound(got, want, terms, absum)
    print("bootstrap ratio to bound", case, RATIOS[case], "max so far", max(RATIOS.values()))
    # adding onto what boot holds: the same call without QFA_F_ZERO_ACCUM continues the chain
    base = np.random.default_rng(3).integers(0, 5, got.shape).astype(np.float64)
    again = run_boot(dev, rows, codes, nz, R, seed=0x1234567890, off=off, flags=0, boot=base)
    want2, _, _ = ref.bootstrap(rows, codes, nz, R, 0x1234567890, off, boot=base)
    assert (np.abs(again - want2) <= (terms[:, None, :, None] * U) * (absum + np.abs(base))).all()


def test_codes_all_minus_one_and_non_finite_rows_reach_nothing(dev):
    rows, codes = make_rows(20, 3, 3, 7, 3, "float32", 5)
    got = run_boot(dev, rows, np.full_like(codes, -1), 3, 5)
    assert (got == 0.0).all()
    bad = rows.copy()
    bad[codes == -1] = np.nan
    bad[0, 0, 0] = np.inf if codes[0, 0, 0] == -1 else bad[0, 0, 0]
    assert np.array_equal(run_boot(dev, bad, codes, 3, 5), run_boot(dev, rows, codes, 3, 5))
    wild = codes.copy()
    wild[codes == -1] = 3                                        # any code outside 0 .. nz - 1 is in no bin
    assert np.array_equal(run_boot(dev, bad, wild, 3, 5), run_boot(dev, rows, codes, 3, 5))


@pytest.mark.parametrize("dtype", ["float32", "int32"])
def test_cut_replicate_draw_and_run_independence(dev, dtype):
    B, S, nseg, W, nz = 50, 3, 3, 7, 3
    rows, codes = make_rows(B, S, nseg, W, nz, dtype, 11)
    one = run_boot(dev, rows, codes, nz, 17, off=40)
    assert np.array_equal(run_boot(dev, rows, codes, nz, 17, off=40), one)                         # two runs: the same bits
    half = run_boot(dev, rows[:23], codes[:23], nz, 17, off=40)
    two = run_boot(dev, rows[23:], codes[23:], nz, 17, off=63, flags=0, boot=half)
    want, terms, absum = ref.bootstrap(rows, codes, nz, 17, 7, 40)
    ratio_to_bound(two, want, terms, absum)
    if dtype == "int32":
        assert np.array_equal(two, one)
    assert np.array_equal(two, one)                              # (stronger than the bound: every element is one chain in segment order)
    assert np.array_equal(run_boot(dev, rows, codes, nz, 5, off=40), one[:, :5])                  # replicate r does not depend on R
    for s in range(S):                                                                             # draw s does not depend on S
        assert np.array_equal(run_boot(dev, rows[:, s:s + 1].copy(), codes[:, s:s + 1].copy(), nz, 17, off=40)[0], one[s])
    assert not np.array_equal(run_boot(dev, rows, codes, nz, 17, off=41), one)                     # the row offset is in the weight


# ------------------------------------------------------------------------------------------------------------ codes
def test_codes_against_p1d(dev):
    import torch
    from qfa_amd import _lib
    B, S, nb, L, nseg, p_lo = 24, 3, 100, 30, 3, 4
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, 77)
    zf, forms = redshift_forms(dev, g, B, nb)
    h = _lib.lib()
    for bins in ((1.0, 1.0, 3), (2.0, 0.5, 3)):                  # every z inside the bins; bins that leave segments out
        for form in forms:
            prm = (p_lo, L, nseg, 24, bins)
            power, noise, stack = call_p1d(dev, tr, iv, tbar, prm, **form)
            codes = torch.full((B, S, nseg), -9, dtype=torch.int32, device=dev)
            tb = T(tbar, dev).reshape(-1, TB_BINS[2]).contiguous()
            bs = _lib.Batch()
            addr = lambda k: form[k].data_ptr() if k in form else None
            bs.zabs, bs.zq1, bs.pix_ratio, bs.rows, bs.row_stride = addr("zabs"), addr("zq1"), addr("ratio"), addr("rows"), 0
            pp = _lib.P1DParams(TB_BINS[0], TB_BINS[1], TB_BINS[2], S, p_lo, L, nseg, 24, bins[0], bins[1], bins[2])
            st = h.qfa_segment_codes_f32(C.c_void_p(tr.data_ptr()), C.c_void_p(iv.data_ptr()), C.byref(bs), C.c_void_p(tb.data_ptr()),
                                         B, S, nb, C.byref(pp), C.c_void_p(codes.data_ptr()), _lib.current_stream(dev))
            torch.cuda.synchronize()
            assert st == 0
            cd = codes.cpu().numpy()
            assert ((cd >= -1) & (cd < bins[2])).all()
            if bins[0] == 1.0:
                assert np.array_equal(cd >= 0, noise > 0) and (cd >= 0).any() and (cd < 0).any()
            else:
                assert ((cd >= 0) <= (noise > 0)).all() and ((cd < 0) & (noise > 0)).any()
            hist = np.stack([np.bincount(cd[:, s][cd[:, s] >= 0], minlength=bins[2]) for s in range(S)])
            assert np.array_equal(hist, stack[:, :, 0]) and hist.sum() > 0
    # the method on the model: the same codes through `segment_codes`
    mine = m.segment_codes(tr, iv, zfac=(forms[1]["zq1"], forms[1]["ratio"]), tbar=T(tbar, dev), tbar_bins=TB_BINS, seg_len=L,
                           n_segments=nseg, pixel_start=p_lo, min_used=24, bins=(2.0, 0.5, 3))
    assert mine.dtype == torch.int32 and np.array_equal(mine.cpu().numpy(), cd)


# ------------------------------------------------------------------------------------------------------------ end to end
def boot_loader_case(dev, n=48, npix=300, nb=144, **dl_kw):
    """(model, mk(batch_size) -> a fresh DeviceDataloader of the same ``n`` synthetic spectra with 10 % dead pixels)"""
    from qfa_amd import synthetic
    from qfa_amd.dataloader import DeviceDataloader
    wav = 10 ** (np.log10(synthetic.LYA) + (np.arange(npix) - nb + 0.5) * 4e-4)
    p, mu = synthetic.mock_parameters(npix, nb, 4, seed=3)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, n, seed=33, masks=False)
    dead = np.random.default_rng(4).random((n, npix)) < 0.1
    flux, err = np.where(dead, np.float32(-999.0), b["flux"]), np.where(dead, np.float32(-999.0), b["error"])
    m = make_model(dev, {"p": p, "mu": mu}, nb, npix - nb, 4)
    return m, lambda bs: DeviceDataloader(flux, err, b["zqso"], wav, batch_size=bs, device=dev, shuffle=False, **dl_kw)


Z = (1.5, 4.5, 3)                                                # bins of the loader tests: every synthetic quasar lies inside
STATS = {"p1d": ("flux_power", {}), "bands": ("band_power", None), "xi": ("flux_correlation", {"n_lags": 5}),
         "pdf": ("flux_pdf", {"n_tbins": 8, "t_max": 1.2}), "variance": ("variance_function", {"e_lo": -12, "n_oct": 14})}


def test_bootstrap_of_a_loader(dev):
    import torch
    from qfa_amd.stacks import BootstrapStack, P1DBandStack
    m, mk = boot_loader_case(dev)
    dl = mk(48)
    dv = 299792.458 * float(np.log(dl.wav_grid[1] / dl.wav_grid[0]))
    half = float(np.exp(0.5 * 49 * dv / 299792.458))
    tb = m.mean_transmission(dl, (1.0 + Z[0]) / half - 1.0, (1.0 + Z[1]) * half - 1.0, 8, n_samples=2, seed=6, batch_size=48)
    shared = dict(n_segments=3, min_used_frac=0.75, n_samples=2, seed=6, tbar=tb)
    for name, (method, own) in STATS.items():
        own = dict(k_edges=P1DBandStack.linear_k_edges(48, dv, 4)) if own is None else own
        plain = getattr(m, method)(mk(48), *Z, batch_size=48, **own, **shared)
        stack, boot = m.bootstrap(mk(48), name, *Z, 9, boot_seed=5, batch_size=48, **own, **shared)
        assert torch.equal(stack.buf, plain.buf), name                                # the statistic itself: bit-equal
        assert isinstance(boot, BootstrapStack) and (boot.S, boot.R, boot.nz, boot.seed) == (2, 9, 3, 5) and boot.bins == stack.bins
        stack16, boot16 = m.bootstrap(mk(16), name, *Z, 9, boot_seed=5, batch_size=16, **own, **shared)
        assert torch.equal(stack16.n if hasattr(stack16, "n") else stack16.n_segments, plain.n if hasattr(plain, "n") else plain.n_segments)
        # the rows of a segment and the weight of a spectrum do not depend on the cut, and every sum is one chain in segment
        # order: the same bits (inside the issue's bound n_terms 2^-52 sum w |x|, trivially; exact for "pdf" as it must be)
        assert torch.equal(boot16.buf, boot.buf), name
        # sum w over the replicates of the segments of a bin: each weight has mean 1
        nseg_bin = (plain.n if hasattr(plain, "n") else plain.n_segments)
        assert boot.n.shape == (2, 9, 3) and nseg_bin.sum() > 40 and abs(float(boot.n.mean(1).sum() / nseg_bin.sum()) - 1.0) < 0.5
        est, cov = boot.estimates(), boot.cov()
        assert est.shape[:3] == (2, 9, 3) and cov.shape == (2, 3, est.shape[3], est.shape[3])
        assert tuple(boot.cov(across_z=True).shape) == (2, 3 * est.shape[3], 3 * est.shape[3])


def _worker_bootstrap(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    m, mk = boot_loader_case(dev, rank=rank, world=world)
    m.enable_data_parallel()
    tb = m.mean_transmission(mk(16), 1.3, 4.8, 8, batch_size=16)
    out = [tb.buf.cpu().numpy().ravel()]
    for name in ("p1d", "pdf"):
        own = {"n_tbins": 8, "t_max": 1.2} if name == "pdf" else {}
        stack, boot = m.bootstrap(mk(16), name, *Z, 6, boot_seed=5, batch_size=16, n_segments=3, tbar=tb, **own)
        out += [stack.buf.cpu().numpy().ravel(), boot.buf.cpu().numpy().ravel()]
    if rank == 0:
        q.put(np.concatenate(out))
    dist.destroy_process_group()


def test_two_ranks_give_the_one_rank_boot(dev):
    import torch
    from qfa_amd.model import ForestStack
    got = two_ranks(_worker_bootstrap, 37500)
    m, mk = boot_loader_case(dev)
    tb = ForestStack(torch.tensor(got[:32].reshape(1, 4, 8), device=dev), 1.3, 3.5 / 8, 8)
    at = 32
    for name in ("p1d", "pdf"):
        own = {"n_tbins": 8, "t_max": 1.2} if name == "pdf" else {}
        stack, boot = m.bootstrap(mk(16), name, *Z, 6, boot_seed=5, batch_size=16, n_segments=3, tbar=tb, **own)
        one_s, one_b = stack.buf.cpu().numpy(), boot.buf.cpu().numpy()
        two_s = got[at:at + one_s.size].reshape(one_s.shape)
        two_b = got[at + one_s.size:at + one_s.size + one_b.size].reshape(one_b.shape)
        at += one_s.size + one_b.size
        nseg_bin = one_s[:, :, 0]
        assert np.array_equal(two_s[:, :, 0], nseg_bin) and nseg_bin.sum() > 40
        if name == "pdf":
            assert np.array_equal(two_b, one_b)
        else:                                                    # rows of p1d are >= 0: sum w |x| is the element itself
            assert (np.abs(two_b - one_b) <= nseg_bin[:, None, :, None] * U * np.abs(one_b)).all()
            assert np.array_equal(two_b[..., 0], one_b[..., 0])


def test_bootstrap_error_bar_agrees_with_the_segment_scatter(dev):
    """one segment per spectrum, no posterior draws: the segments ARE the sightlines, so the bootstrap variance of the mean power
    must be P1DStack.err()^2 up to the sampling error of a variance from R replicates, 4 sqrt(2 / (R - 1)) = 28 % on the median over
    the modes.  (The numpy reference alone, exponential power, 2 000 spectra, three seeds: median ratio 0.99 .. 1.03.)"""
    import torch
    R = 400
    m, mk = boot_loader_case(dev, n=2000, npix=120, nb=64)
    stack, boot = m.bootstrap(mk(2000), "p1d", 1.5, 4.5, 1, R, boot_seed=3, batch_size=2000, n_segments=1, seg_len=64)
    assert float(stack.n[0, 0]) > 1500
    vb = boot.err(fn=lambda sums: sums[..., 2:] / sums[..., :1] * stack.dv)[0, 0] ** 2          # the mean power, as err() has it: noise in
    vs = stack.err()[0, 0] ** 2
    ratio = float(torch.median(vb / vs))
    print("bootstrap variance / segment-scatter variance, median over modes:", ratio)
    assert abs(ratio - 1.0) <= 4.0 * np.sqrt(2.0 / (R - 1))


def test_cli_predict_writes_bootstrap_npz(dev, tmp_path):
    from qfa_amd import cli
    c = cli_predict_case(dev, tmp_path)
    out = tmp_path / "out"
    argv = c.argv(out, "MODEL.BOOT_N", "8", "MODEL.BOOT_SEED", "3", "MODEL.P1D_NBANDS", "3", "MODEL.XI_NLAGS", "4", "MODEL.PDF_NBINS", "6",
                  "MODEL.VAR_NOCT", "14", "MODEL.VAR_MIN_COUNT", "5")
    assert cli.main(argv) == 0
    L = c.nb // 2
    widths = {"flux_power": L // 2, "flux_power_bands": 3, "flux_correlation": 4, "flux_pdf": 6, "variance_function": 28}
    for stem, n in widths.items():
        assert (out / (stem + ".npz")).exists(), stem
        f = np.load(out / (stem + "_bootstrap.npz"))
        assert {"estimates", "cov", "n_boot", "seed"} <= set(f.files), stem
        assert int(f["n_boot"]) == 8 and int(f["seed"]) == 3
        assert f["estimates"].shape == (1, 8, 3, n) and f["cov"].shape == (1, 3, n, n), stem
        filled = f["n"].min(1) > 1                               # (S, nz): every replicate holds segments there
        assert filled.any(), stem
        if stem != "variance_function":
            assert np.isfinite(f["cov"][filled]).all(), stem
            continue
        for s, kz in zip(*np.nonzero(filled)):                   # a variance bin without pixels has no estimate: the bins every replicate fills
            ok = (f["sums"][s, :, kz, 1:1 + n] > 0).all(0)
            assert ok.any() and np.isfinite(f["cov"][s, kz][np.ix_(ok, ok)]).all(), (s, kz)
