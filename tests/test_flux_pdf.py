"""The flux PDF of forest segments and its covariance stack on the MI355X (QFA.flux_pdf_segments / flux_pdf, qfa_flux_pdf_f32)
against the numpy port of the contract (tests/_flux_pdf_ref.py).

The contract is float32 per pixel and integer from there on, and the port works on the very trans / ivar the GPU read: every
comparison of `hist` and `stack` is exact equality, no tolerance, no pixel left out.  Only PDFStack.cov() -- float64 arithmetic on the
stack -- has a bar, derived in the port.  The inputs are those of tests/test_p1d.py: the transmission and inverse variance
QFA.forest writes for tests/test_forest.py's `geometry` (continuum in [0.5, 2], 20 % masks)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _flux_pdf_ref as R
import _p1d_ref as RP
from _segment_harness import (F_ZERO, TB_BINS, T, call_segment, case_shape, cli_predict_case, dev, forest_case,  # noqa: F401 (dev: the fixture)
                              loader_case, make_model, redshift_forms, refusals)

pytestmark = pytest.mark.gpu
F_REL, F_CLAMP = 0x800, 0x1000
BINS = (1.6, 0.45, 4)
T_LO, T_HI = 0.2, 1.4                                         # the geometry's T leaves pixels on both sides of it
# (rows, L, nseg, p_lo, nt): the 64-pixel walk at L = 63 / 64 / 65 via the neighbours, lane nt - 1 at nt = 64, a chunk not filled
CASES = [(1, 1, 1, 0, 1), (3, 2, 2, 1, 2), (17, 37, 3, 5, 20), (33, 64, 2, 0, 63), (33, 65, 2, 0, 64), (16, 240, 3, 0, 20),
         (5, 667, 1, 3, 21), (2, 4096, 1, 0, 64)]


def median_ivar(ivar):
    """the median inverse variance of the unmasked pixels of a case (0 without any)"""
    pos = ivar[ivar > 0]
    return float(np.median(pos)) if pos.size else 0.0


def call_pdf(dev, trans, ivar, tbar, prm, pdf, **kw):
    """qfa_flux_pdf_f32 by hand on device tensors; prm = (p_lo, L, nseg, min_used, (z0, dz, nz)), pdf = (t0, dt, nt, ivar_min).
    Returns hist, stack (numpy)"""
    from qfa_amd import _lib
    nt = max(1, min(64, int(pdf[2])))
    return call_segment("qfa_flux_pdf", dev, trans, ivar, tbar, prm, _lib.PDFParams(*pdf), (("h", (nt,), "int32"),), size=(int(pdf[2]),),
                        stack_width=2 + nt + nt * nt, **kw)


def check_exact(hist, stack, ref, nt, what):
    """hist and stack equal the port's integers entry for entry; invalid segments hold 0; the matrix is symmetric"""
    assert np.array_equal(hist, ref["hist"]), (what, "hist")
    assert (hist[~ref["valid"]] == 0).all(), (what, "invalid segments")
    assert np.array_equal(stack, ref["stack"].astype(np.float64)), (what, "stack")
    M = stack[:, :, 2 + nt:].reshape(stack.shape[0], stack.shape[1], nt, nt)
    assert np.array_equal(M, np.swapaxes(M, 2, 3)), (what, "symmetry")


def assert_not_vacuous(ref, rows, L, nt, clamp, split, what):
    """asserted on the port's output: the case exercises what it is there for"""
    if L < 37:
        return
    valid, st = ref["valid"], ref["stack"]
    assert valid.any() and (rows < 16 or not valid.all()), what
    assert (ref["hist"].sum((0, 1, 2)) > 0).sum() >= 3, (what, "occupied bins")
    if not clamp:
        assert ref["hist"].sum() < ref["n_cnt"].sum(), (what, "out_of_range")
    if split:
        assert (ref["n_cnt"][valid] < ref["n_used"][valid]).any(), (what, "ivar_min")
    assert st[:, :, 0].sum() > 0, what


@pytest.mark.parametrize("rows,L,nseg,p_lo,nt", CASES)
def test_counts_and_stack_equal_the_port(dev, rows, L, nseg, p_lo, nt):
    B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=seed)
    prm = (p_lo, L, nseg, min_used, BINS)
    trn, ivn = tr.cpu().numpy(), iv.cpu().numpy()
    t0, dt = np.float32(T_LO), np.float32((T_HI - T_LO) / nt)
    z = T(g["zabs"], dev)
    for clamp, rel, imin in itertools.product((False, True), (False, True), (0.0, median_ivar(ivn))):
        ref = R.flux_pdf(trn, ivn, g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, BINS, t0, dt, nt, rel, clamp, imin)
        hist, stack = call_pdf(dev, tr, iv, tbar, prm, (t0, dt, nt, imin), zabs=z,
                               flags=F_ZERO | (F_REL if rel else 0) | (F_CLAMP if clamp else 0))
        what = f"rows {rows} (B {B} S {S}) L {L} nseg {nseg} p_lo {p_lo} nt {nt} clamp {clamp} relative {rel} ivar_min {imin}"
        assert_not_vacuous(ref, rows, L, nt, clamp, imin > 0, what)
        print(f"{what}: {int(ref['hist'].sum())} of {int(ref['n_cnt'].sum())} counted pixels in a bin, "
              f"{int(ref['stack'][:, :, 0].sum())} segments stacked")
        check_exact(hist, stack, ref, nt, what)


@pytest.mark.parametrize("rows,L,nseg,p_lo,nt", CASES[3:5])
def test_redshift_forms_equal_the_port(dev, rows, L, nseg, p_lo, nt):
    """zabs, the factored pair and the resident `rows` form of both on identical z: each equals the port"""
    B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=seed)
    prm = (p_lo, L, nseg, min_used, BINS)
    t0, dt = np.float32(T_LO), np.float32((T_HI - T_LO) / nt)
    zf, forms = redshift_forms(dev, g, B, nb)
    ref = R.flux_pdf(tr.cpu().numpy(), iv.cpu().numpy(), zf, tbar, TB_BINS, p_lo, L, nseg, min_used, BINS, t0, dt, nt, True, True)
    assert_not_vacuous(ref, rows, L, nt, True, False, "forms")
    for kw in forms:
        hist, stack = call_pdf(dev, tr, iv, tbar, prm, (t0, dt, nt, 0.0), flags=F_ZERO | F_REL | F_CLAMP, **kw)
        check_exact(hist, stack, ref, nt, sorted(kw))


def test_bin_edges_by_hand(dev):
    """trans written by the test: every exact edge t0 + a dt (a = -1 .. 25), the float32 neighbours of three edges, +inf and a huge
    value on used pixels, NaN / inf / -inf under ivar = 0.  An edge belongs to the bin above it; nothing under the mask is counted;
    +inf reaches the top bin only under clamp"""
    t0, dt, nt = np.float32(-0.25), np.float32(0.0625), 24
    edges = (t0 + np.arange(-1, 26, dtype=np.float32) * dt).astype(np.float32)         # (exact: multiples of 2^-4)
    near = np.concatenate([[np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))] for e in edges[[1, 2, 3]]])
    vals = np.concatenate([edges, near.astype(np.float32), np.array([np.inf, 3e38], np.float32)])
    junk = np.array([np.nan, np.inf, -np.inf], np.float32)
    L = len(vals) + len(junk)
    trans = np.concatenate([vals, junk]).astype(np.float32)[None, None, :]
    ivar = np.concatenate([np.full(len(vals), 4.0, np.float32), np.zeros(len(junk), np.float32)])[None, None, :]
    z = np.full((1, L), 2.05, np.float32)
    tbar = np.ones((1, TB_BINS[2]), np.float32)
    prm = (0, L, 1, 1, (2.0, 0.25, 2))
    want = {}
    # by hand: edge a (a = -1 .. 25) sits in bin a; the neighbours of edges 0, 1, 2 in bins a - 1 and a (below them |x| >= x - t0, so
    # that x - t0 is exact and the neighbour below an edge stays below it)
    a_of = np.concatenate([np.arange(-1, 26), [-1, 0, 0, 1, 1, 2], [10 ** 9, 10 ** 9]])
    for clamp in (False, True):
        k = np.where((a_of >= 0) & (a_of < nt), a_of, -1)
        if clamp:
            k = np.where(a_of < 0, 0, np.where(a_of >= nt, nt - 1, k))
        want[clamp] = np.bincount(k[k >= 0], minlength=nt)
    assert want[False].sum() == 24 + 5 and want[True].sum() == len(vals) and want[True][nt - 1] == want[False][nt - 1] + 4
    assert want[True][0] == want[False][0] + 2
    for clamp in (False, True):
        ref = R.flux_pdf(trans, ivar, z, tbar, TB_BINS, 0, L, 1, 1, prm[4], t0, dt, nt, False, clamp)
        assert np.array_equal(ref["hist"][0, 0, 0], want[clamp]) and ref["n_cnt"][0, 0, 0] == len(vals)      # the port, by hand
        for rel in (False, True):                                                     # (tbar = 1: T / tb = T)
            hist, stack = call_pdf(dev, T(trans, dev), T(ivar, dev), tbar, prm, (t0, dt, nt, 0.0), zabs=T(z, dev),
                                   flags=F_ZERO | (F_CLAMP if clamp else 0) | (F_REL if rel else 0))
            assert np.array_equal(hist[0, 0, 0], want[clamp]), (clamp, rel)
            assert stack[0, 0, 0] == 1 and stack[0, 0, 1] == len(vals) and np.array_equal(stack[0, 0, 2:2 + nt], want[clamp])
            assert np.array_equal(stack[0, 0, 2 + nt:].reshape(nt, nt), np.outer(want[clamp], want[clamp])) and (stack[0, 1] == 0).all()


def test_accumulation_and_independence(dev):
    """ADD against QFA_F_ZERO_ACCUM, draw s of an S = 3 call against a call on that draw alone, B cut in two calls that add into one
    stack, hist-only and stack-only calls: all exact.  More segments per draw than one chunk holds"""
    import torch
    B, S, nb, L, nseg, nt = 50, 3, 64, 21, 3, 12
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=41)
    prm = (0, L, nseg, 15, BINS)
    pdf = (np.float32(T_LO), np.float32((T_HI - T_LO) / nt), nt, 0.0)
    z = T(g["zabs"], dev)
    ref = R.flux_pdf(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, 0, L, nseg, 15, BINS, *pdf[:3], False, True)
    assert ref["stack"][:, :, 0].sum() > 64 * S and B * nseg > 2 * 64
    hist, stack = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=z, flags=F_ZERO | F_CLAMP)
    check_exact(hist, stack, ref, nt, "whole")
    for s in range(S):
        one = call_pdf(dev, tr[:, s:s + 1].contiguous(), iv[:, s:s + 1].contiguous(), tbar[s:s + 1], prm, pdf, zabs=z,
                       flags=F_ZERO | F_CLAMP)
        assert np.array_equal(one[0][:, 0], hist[:, s]) and np.array_equal(one[1][0], stack[s]), s
    h_only = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=z, flags=F_ZERO | F_CLAMP, outs="h")
    s_only = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=z, flags=F_ZERO | F_CLAMP, outs="s")
    assert h_only[1] is None and s_only[0] is None and np.array_equal(h_only[0], hist) and np.array_equal(s_only[1], stack)
    # ADD onto a pre-filled stack, exactly; QFA_F_ZERO_ACCUM overwrites the same filling
    fill = np.arange(stack.size, dtype=np.float64).reshape(stack.shape)
    added = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=z, flags=F_CLAMP, stack=torch.tensor(fill, device=dev))[1]
    assert np.array_equal(added, fill + stack)
    over = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=z, flags=F_ZERO | F_CLAMP, stack=torch.tensor(fill, device=dev))[1]
    assert np.array_equal(over, stack)
    # B cut in two calls (not on a chunk boundary) that add into one stack
    acc = torch.zeros(stack.shape, dtype=torch.float64, device=dev)
    for lo, hi in ((0, 17), (17, B)):
        call_pdf(dev, tr[lo:hi].contiguous(), iv[lo:hi].contiguous(), tbar, prm, pdf, zabs=z[lo:hi].contiguous(), flags=F_CLAMP, stack=acc)
    assert np.array_equal(acc.cpu().numpy(), stack)


def test_the_host_cuts_a_call_into_launches_without_changing_the_result(dev):
    """4096 z-bins and 32 flux bins: a chunk's partial rows take 9 MB of the 64 MB a launch aims at, so that the 1200 segments of
    this call -- 19 chunks -- need several launches (the workspace the size function reports holds fewer chunks than the call has).
    The stack equals the port's all the same"""
    from qfa_amd import _lib
    B, S, nb, L, nseg, nt, nz = 400, 1, 64, 21, 3, 32, 4096
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=43)
    bins = (1.6, np.float32(1.8 / nz), nz)
    prm = (0, L, nseg, 15, bins)
    pdf = (np.float32(T_LO), np.float32((T_HI - T_LO) / nt), nt, 0.0)
    need = _lib.lib().qfa_flux_pdf_workspace_bytes(B * S, S, nb, L, nseg, nz, nt)
    row = S * nz * (2 + nt + nt * (nt + 1) // 2) * 4                                   # a chunk's partials
    assert 0 < need < (B * nseg + 63) // 64 * row                                     # fewer chunks than the call has: several launches
    ref = R.flux_pdf(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, 0, L, nseg, 15, bins, *pdf[:3], False, True)
    assert ref["stack"][:, :, 0].sum() > 300 and (ref["stack"][:, :, 0] > 0).sum() > 100
    hist, stack = call_pdf(dev, tr, iv, tbar, prm, pdf, zabs=T(g["zabs"], dev), flags=F_ZERO | F_CLAMP, ws_bytes=need)
    check_exact(hist, stack, ref, nt, "launches")


def test_every_refusal_returns_its_code_and_touches_nothing(dev):
    B, S, nb, L, nseg, nt = 4, 1, 60, 20, 2, 10
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=61)
    z = T(g["zabs"], dev)
    prm = (0, L, nseg, 10, BINS)
    pdf = (0.0, 0.1, nt, 0.0)

    refused = refusals(lambda **kw: call_pdf(dev, tr, iv, tbar, **kw), prm=prm, pdf=pdf, flags=F_ZERO, outs="hs", zabs=z)
    refused(-1, outs="")                                                              # both outputs missing
    refused(-1, zabs=None)                                                            # no redshift at all
    refused(-1, zabs=None, zq1=T(g["zq1"], dev))                                      # half of the factored pair
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.1, 0, 0.0), (0.0, 0.1, 65, 0.0), (0.0, 0.1, -1, 0.0), (0.0, 0.0, nt, 0.0), (0.0, -0.1, nt, 0.0),
                (0.0, nan, nt, 0.0), (0.0, inf, nt, 0.0), (nan, 0.1, nt, 0.0), (-inf, 0.1, nt, 0.0), (0.0, 0.1, nt, -1e-3),
                (0.0, 0.1, nt, nan), (0.0, 0.1, nt, inf)):
        refused(-2, pdf=bad)
    refused(-2, prm=(0, L, nseg, 0, BINS))                                            # min_used < 1
    refused(-2, prm=(21, L, nseg, 10, BINS))                                          # the segments pass Nb
    refused(-2, prm=(0, L, nseg, 10, (1.6, 0.0, 4)))                                  # dz = 0
    refused(-2, prm=(0, L, nseg, 10, (1.6, 0.45, 0)))                                 # nz = 0
    for flags in (0x1, 0x100, 0x200, 0x400, F_ZERO | 0x8, 0x2000):
        refused(-5, flags=flags)
    need = call_ws(B, S, nb, L, nseg, nt)
    refused(-3, ws_bytes=need - 1)
    # q missing
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    bs = _lib.Batch()
    bs.zabs, bs.row_stride = z.data_ptr(), 0
    pp = _lib.P1DParams(TB_BINS[0], TB_BINS[1], TB_BINS[2], 1, 0, L, nseg, 10, BINS[0], BINS[1], BINS[2])
    tb = T(tbar, dev).contiguous()
    out = torch.full((B, S, nseg, nt), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert lib.qfa_flux_pdf_f32(C.c_void_p(tr.data_ptr()), C.c_void_p(iv.data_ptr()), C.byref(bs), C.c_void_p(tb.data_ptr()), B, S, nb,
                                C.byref(pp), None, 0, C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), need, None) == -1
    torch.cuda.synchronize()
    assert (out == -7).all()


def call_ws(B, S, nb, L, nseg, nt):
    from qfa_amd import _lib
    return _lib.lib().qfa_flux_pdf_workspace_bytes(B * S, S, nb, L, nseg, BINS[2], nt)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_flux_pdf_of_a_loader(dev):
    import torch
    m, mk, wav = loader_case(dev)
    kw = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, seed=6, t_min=0.0, t_max=1.2)
    for S in (0, 3):
        a = m.flux_pdf(mk(96), 1.8, 3.4, 3, 12, n_samples=S, batch_size=96, **kw)
        c = m.flux_pdf(mk(96), 1.8, 3.4, 3, 12, n_samples=S, batch_size=40, **kw)
        assert a.S == max(1, S) and a.L == 24 and a.nt == 12 and a.clamp and not a.relative and a.n_segments.sum() > 20 * a.S
        assert torch.equal(a.buf, c.buf), S                                           # integers: no rounding to allow for
        ok = a.n_segments > 1
        assert torch.isfinite(a.pdf()[ok]).all() and torch.isfinite(a.cov()[ok]).all() and (a.out_of_range()[ok] == 0).all()
        assert torch.allclose((a.pdf()[ok] * a.dt).sum(-1), torch.ones_like(a.n_pixels[ok]), rtol=1e-13)
    assert a.std_over_draws.shape == (3, 12) and a.total_cov.shape == (3, 12, 12)
    # tbar = None against a passed ForestStack from mean_transmission with the documented arguments
    dl = mk(96)
    one = m.flux_pdf(dl, 1.8, 3.4, 3, 12, batch_size=96, **kw)
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    half = float(np.exp(0.5 * 25 * dv / 299792.458))
    tb1 = m.mean_transmission(dl, 2.8 / half - 1.0, 4.4 * half - 1.0, 8, batch_size=96)
    assert torch.equal(m.flux_pdf(dl, 1.8, 3.4, 3, 12, batch_size=96, tbar=tb1, **kw).buf, one.buf)
    # the resident loader form against the tensor form of the same rows, and both against the loader's stack
    rb = dl.rows_batch(0, 96)[0]
    _, hm, _, _, unc = m.predict(batch=rb)
    tr, iv, _ = m.forest(batch=rb, hmean=hm, unc=unc)
    skw = dict(tbar=tb1, seg_len=24, n_segments=2, min_used=18, t_min=0.0, t_max=1.2, n_tbins=12, clamp=True, bins=one.bins)
    h1, s1 = m.flux_pdf_segments(tr, iv, batch=rb, **skw)
    _, zfac = rb.materialize(raw_flux=True)
    h2, s2 = m.flux_pdf_segments(tr, iv, zfac=zfac, **skw)
    assert h1.shape == (96, 1, 2, 12) and h1.dtype == torch.int32 and torch.equal(h1, h2) and torch.equal(s1.buf, s2.buf)
    assert torch.equal(s1.buf, one.buf)
    # stack= must match in flux bins, flags and ivar_min
    from qfa_amd._lib import QFAHipError
    for other in (dict(n_tbins=11), dict(t_max=1.3), dict(clamp=False), dict(relative=True), dict(ivar_min=0.5), dict(seg_len=23)):
        with pytest.raises(QFAHipError):
            m.flux_pdf_segments(tr, iv, batch=rb, **{**skw, "bins": None, **other}, stack=s1)


def test_cov_on_the_device_against_the_brute_force(dev):
    """PDFStack.cov() on the device against the segment-by-segment sum over the call's own hist, within the port's bar"""
    from qfa_amd.model import PDFStack
    import torch
    B, S, nb, L, nseg, nt = 40, 3, 80, 37, 2, 9
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=71)
    t0, dt = np.float32(T_LO), np.float32((T_HI - T_LO) / nt)
    hist, stack = call_pdf(dev, tr, iv, tbar, (3, L, nseg, 25, BINS), (t0, dt, nt, 0.0), zabs=T(g["zabs"], dev), flags=F_ZERO | F_CLAMP)
    ref = R.flux_pdf(tr.cpu().numpy(), iv.cpu().numpy(), g["zabs"], tbar, TB_BINS, 3, L, nseg, 25, BINS, t0, dt, nt, False, True)
    st = PDFStack(torch.tensor(stack, device=dev), *BINS, L, t0, dt, nt, False, True)
    got = st.cov().cpu().numpy()
    want = R.cov_bruteforce(hist, ref["valid"], ref["kz"], BINS[2], dt)
    bar, scaled = R.cov_bar(stack, nt, dt)
    ok = np.isfinite(want)
    assert ok.any() and np.array_equal(ok, np.isfinite(got))
    print(f"cov: max |d cov| / bar = {(np.abs(got - want)[ok] / bar[ok].clip(1e-300)).max():.3f}")
    assert (np.abs(got - want)[ok] <= bar[ok]).all()
    rows_bar = np.nansum((st.n_segments.cpu().numpy()[:, :, None, None] + 32.0 + nt) * R.U64 * scaled, axis=-1)
    rows_ok = ok.all(-1)
    assert (np.abs(got.sum(-1))[rows_ok] <= rows_bar[rows_ok]).all()


def test_cli_predict_writes_flux_pdf_npz(dev, tmp_path):
    """predict mode with MODEL.PDF_NBINS: flux_pdf.npz next to flux_power.npz with the documented keys and shapes; its counts are
    the in-range counted pixels the port finds on the same loader"""
    import torch
    from qfa_amd import cli
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.model import ForestStack
    c = cli_predict_case(dev, tmp_path)
    wav, npix, nb, b, names, p, mu = c.wav, c.npix, c.nb, c.b, c.names, c.p, c.mu
    out = tmp_path / "out"
    argv = c.argv(out, "MODEL.N_SAMPLES", "2", "MODEL.PDF_NBINS", "12", "MODEL.PDF_TMAX", "1.2", "MODEL.PDF_CLAMP", "False")
    assert cli.main(argv) == 0
    f, fp, t = np.load(out / "flux_pdf.npz"), np.load(out / "flux_power.npz"), np.load(out / "mean_transmission.npz")
    assert set(f.files) == {"z", "t_edges", "pdf", "err", "cov", "counts", "n_segments", "out_of_range", "std_over_draws", "total_cov"}
    assert f["z"].shape == (3,) and f["t_edges"].shape == (13,) and f["pdf"].shape == f["err"].shape == f["counts"].shape == (2, 3, 12)
    assert f["cov"].shape == (2, 3, 12, 12) and f["n_segments"].shape == f["out_of_range"].shape == (2, 3)
    assert f["std_over_draws"].shape == (3, 12) and f["total_cov"].shape == (3, 12, 12)
    assert np.array_equal(f["n_segments"], fp["n"]) and f["n_segments"].sum() > 10     # the segments flux_power stacked
    assert np.allclose(f["t_edges"], np.float32(0.0) + np.float64(np.float32(0.1)) * np.arange(13))
    # the port on the same loader: the transmission of the same draws, the mean transmission the command line wrote
    dl = DeviceDataloader(b["flux"].astype(np.float64).astype(np.float32), b["error"].astype(np.float64).astype(np.float32),
                          b["zqso"], wav, 500, dev, tau="becker", mode="predict", paths=names)
    m2 = make_model(dev, {"p": p, "mu": mu}, nb, npix - nb, 4)
    tb = ForestStack(torch.tensor(t["sums"], device=dev), 1.6, 2.0 / 10, 10)
    L = nb // 2
    min_used = max(1, int(np.ceil(0.6 * L)))
    total = 0
    for s, inputs, _ in m2._loader_slices(dl, 4096):
        _, hm, hc, _, _ = m2.predict(**inputs)
        h = m2.sample_latent(hm, hc, 2, seed=0, offset=s)
        tr, iv, _ = m2.forest(**inputs, h=h)
        if "batch" in inputs:
            _, zfac = inputs["batch"].materialize(raw_flux=True)
            zf = RP.z_factored(zfac[0].cpu().numpy(), zfac[1].cpu().numpy())
        else:
            zf = inputs["zabs"].cpu().numpy()
        ref = R.flux_pdf(tr.cpu().numpy(), iv.cpu().numpy(), zf, tb.mean.to(torch.float32).cpu().numpy(), tb.bins, 0, L, 2, min_used,
                         (np.float32(1.6), np.float32(2.0 / 3), 3), np.float32(0.0), np.float32(1.2 / 12), 12, False, False)
        total += int(ref["stack"][:, :, 2:14].sum())
    assert f["counts"].sum() == total > 0
