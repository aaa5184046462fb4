"""The variance function of forest segments and its (v-bin, z) stack on the MI355X (QFA.variance_segments / variance_function,
qfa_variance_f32) against the numpy port of the contract (tests/_variance_ref.py).

The port works on the very trans / ivar the GPU read.  Every count (n_a, n_seg, n_used) is compared for equality; every float sum
within (terms) 2^-52 sum |term| of the port -- the bound on any order of summation derived in the port's docstring, not a measured
tolerance.  The inputs are those of tests/test_p1d.py: the transmission and inverse variance QFA.forest writes for
tests/test_forest.py's `geometry` (continuum in [0.5, 2], 20 % masks)."""
import numpy as np
import pytest

import _p1d_ref as RP
import _variance_ref as R
from _segment_harness import F_SYNC, F_ZERO, TB_BINS, T, call_segment, case_shape, dev, forest_case, loader_case, redshift_forms, refusals  # noqa: F401

pytestmark = pytest.mark.gpu
BINS = (1.6, 0.45, 4)
# (rows, L, nseg, p_lo): one wave's walk at L = 63 / 64 / 65, the block's at 240 (one trip, 16 idle lanes), 667 and 4096 (three and
# sixteen trips), rows that leave the only chunk of 64 unfilled (17 x 3 = 51, 11 x 2 = 22, 16 x 3 = 48 segments per draw; more than one
# chunk, the last unfilled: test_accumulation_independence_and_the_cut, 150 segments per draw)
CASES = [(1, 1, 1, 0), (3, 2, 2, 1), (17, 37, 3, 5), (33, 63, 2, 0), (33, 64, 2, 0), (33, 65, 2, 0), (48, 240, 3, 0), (5, 667, 1, 3),
         (2, 4096, 1, 0)]
# (n_oct, sub): nv = 1, 6 and 64
VBINS = [(1, 0), (3, 1), (4, 4)]


def call_var(dev, trans, ivar, tbar, prm, var, **kw):
    """qfa_variance_f32 by hand on device tensors; prm = (p_lo, L, nseg, min_used, (z0, dz, nz)), var = (e_lo, n_oct, sub, d_max).
    Returns moments, stack (numpy)"""
    from qfa_amd import _lib
    nv = var[1] << var[2] if 0 <= var[2] <= 4 and 1 <= var[1] <= 64 else 1
    nv = max(1, min(64, nv))
    return call_segment("qfa_variance", dev, trans, ivar, tbar, prm, _lib.VarParams(*var), (("m", (5, nv), "float64"),), size=(nv,),
                        stack_width=2 + 5 * nv, **kw)


def check(mom, stack, ref, what, extra_stack_bar=0.0):
    """counts equal the port's, float sums within the port's bar, invalid segments exactly 0"""
    nv = ref["nv"]
    mb, sb = R.bars(ref)
    if mom is not None:
        assert np.array_equal(mom[..., 0, :], ref["moments"][..., 0, :]), (what, "n_a")
        assert (mom[~ref["valid"]] == 0).all(), (what, "invalid segments")
        err = np.abs(mom - ref["moments"])
        print(f"{what}: moments max err / bar = {(err[mb > 0] / mb[mb > 0]).max() if (mb > 0).any() else 0.0:.3f}")
        assert (err <= mb).all(), (what, "moments", float((err - mb).max()))
    if stack is not None:
        assert np.array_equal(stack[:, :, :2 + nv], ref["stack"][:, :, :2 + nv]), (what, "n_seg / n_used / n_a")
        err = np.abs(stack - ref["stack"])
        sb = sb + extra_stack_bar
        print(f"{what}: stack max err / bar = {(err[sb > 0] / sb[sb > 0]).max() if (sb > 0).any() else 0.0:.3f}")
        assert (err <= sb).all(), (what, "stack", float((err - sb).max()))


def assert_not_vacuous(ref, rows, L, nv, what):
    """asserted on the port's output: the case exercises what it is there for"""
    if L < 37:
        return
    valid, st = ref["valid"], ref["stack"]
    assert valid.any() and (rows < 16 or not valid.all()), (what, "invalid segments")
    assert (ref["moments"][..., 0, :].sum((0, 1, 2)) > 0).sum() >= min(3, nv), (what, "occupied bins")
    assert st[:, :, 2:2 + nv].sum() < st[:, :, 1].sum(), (what, "pixels outside the bins")
    assert st[:, :, 0].sum() > 0, what


def reference(g_z, trn, ivn, tbar, prm, n_oct, sub, d_max=None):
    """the port with e_lo chosen from its own v; returns (ref, var tuple)"""
    p_lo, L, nseg, min_used, bins = prm
    probe = R.variance(trn, ivn, g_z, tbar, TB_BINS, p_lo, L, nseg, min_used, bins, -126, 1, 0)
    e_lo = R.choose_bins(probe["v_all"], n_oct)
    ref = R.variance(trn, ivn, g_z, tbar, TB_BINS, p_lo, L, nseg, min_used, bins, e_lo, n_oct, sub, d_max)
    return ref, (e_lo, n_oct, sub, R.FLT_MAX if d_max is None else d_max)


@pytest.mark.parametrize("rows,L,nseg,p_lo", CASES)
def test_moments_and_stack_against_the_port(dev, rows, L, nseg, p_lo):
    B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=seed)
    prm = (p_lo, L, nseg, min_used, BINS)
    trn, ivn = tr.cpu().numpy(), iv.cpu().numpy()
    z = T(g["zabs"], dev)
    for (n_oct, sub), tb in zip(VBINS, (tbar, tbar[:1], tbar)):                       # (tbar with S rows and with one)
        ref, var = reference(g["zabs"], trn, ivn, tb, prm, n_oct, sub)
        what = f"rows {rows} (B {B} S {S}) L {L} nseg {nseg} p_lo {p_lo} nv {ref['nv']} e_lo {var[0]} tbar rows {tb.shape[0]}"
        assert_not_vacuous(ref, rows, L, ref["nv"], what)
        mom, stack = call_var(dev, tr, iv, tb, prm, var, zabs=z)
        check(mom, stack, ref, what)
        again = call_var(dev, tr, iv, tb, prm, var, zabs=z)
        assert np.array_equal(again[0], mom) and np.array_equal(again[1], stack), (what, "two runs")


@pytest.mark.parametrize("rows,L,nseg,p_lo", [CASES[4], CASES[6]])
def test_redshift_forms_against_the_port(dev, rows, L, nseg, p_lo):
    """zabs, the factored pair and the resident `rows` form of both on identical z: each within the bar, and all the same bits"""
    B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=seed)
    prm = (p_lo, L, nseg, min_used, BINS)
    zf, forms = redshift_forms(dev, g, B, nb)
    ref, var = reference(zf, tr.cpu().numpy(), iv.cpu().numpy(), tbar, prm, 3, 1)
    assert_not_vacuous(ref, rows, L, ref["nv"], "forms")
    first = None
    for kw in forms:
        mom, stack = call_var(dev, tr, iv, tbar, prm, var, **kw)
        check(mom, stack, ref, str(sorted(kw)))
        first = first or (mom, stack)
        assert np.array_equal(mom, first[0]) and np.array_equal(stack, first[1]), sorted(kw)


def test_accumulation_independence_and_the_cut(dev):
    """ADD against QFA_F_ZERO_ACCUM, draws 0..1 of an S = 3 call against an S = 2 call (bit for bit), B cut in two calls that add into
    one stack (within the bar), moments-only and stack-only calls, a finite d_max.  More segments per draw than one chunk holds"""
    import torch
    B, S, nb, L, nseg = 50, 3, 64, 21, 3
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=41)
    prm = (0, L, nseg, 15, BINS)
    z = T(g["zabs"], dev)
    trn, ivn = tr.cpu().numpy(), iv.cpu().numpy()
    ref, var = reference(g["zabs"], trn, ivn, tbar, prm, 3, 1)
    assert ref["stack"][:, :, 0].sum() > 64 * S and B * nseg > 2 * 64
    mom, stack = call_var(dev, tr, iv, tbar, prm, var, zabs=z)
    check(mom, stack, ref, "whole")
    two = call_var(dev, tr[:, :2].contiguous(), iv[:, :2].contiguous(), tbar[:2], prm, var, zabs=z)
    assert np.array_equal(two[0], mom[:, :2]) and np.array_equal(two[1], stack[:2])
    m_only = call_var(dev, tr, iv, tbar, prm, var, zabs=z, outs="m")
    s_only = call_var(dev, tr, iv, tbar, prm, var, zabs=z, outs="s", flags=F_ZERO | F_SYNC)
    assert m_only[1] is None and s_only[0] is None and np.array_equal(m_only[0], mom) and np.array_equal(s_only[1], stack)
    # ADD onto a pre-filled stack: what it held is one more term of every sum; QFA_F_ZERO_ACCUM overwrites the same filling
    fill = np.linspace(0.5, 2.5, stack.size).reshape(stack.shape)
    fill[:, :, :2 + ref["nv"]] = np.round(fill[:, :, :2 + ref["nv"]] * 8)             # (integers where the stack holds counts)
    added = call_var(dev, tr, iv, tbar, prm, var, zabs=z, flags=0, stack=torch.tensor(fill, device=dev))[1]
    assert np.array_equal(added[:, :, :2 + ref["nv"]], (fill + stack)[:, :, :2 + ref["nv"]])
    assert (np.abs(added - (fill + ref["stack"])) <= (R.stack_terms(ref) + 1.0) * R.U52 * (np.abs(fill) + ref["stack_abs"])).all()
    over = call_var(dev, tr, iv, tbar, prm, var, zabs=z, flags=F_ZERO, stack=torch.tensor(fill, device=dev))[1]
    assert np.array_equal(over, stack)
    # B cut in two calls (not on a chunk boundary) that add into one stack: another order of the same terms
    acc = torch.zeros(stack.shape, dtype=torch.float64, device=dev)
    for lo, hi in ((0, 17), (17, B)):
        call_var(dev, tr[lo:hi].contiguous(), iv[lo:hi].contiguous(), tbar, prm, var, zabs=z[lo:hi].contiguous(), flags=0, stack=acc, outs="s")
    check(None, acc.cpu().numpy(), ref, "split")
    # a finite d_max removes exactly the pixels the port removes
    dcut = float(np.float32(0.35))
    refc = R.variance(trn, ivn, g["zabs"], tbar, TB_BINS, 0, L, nseg, 15, BINS, var[0], 3, 1, dcut)
    n_all, n_cut = ref["stack"][:, :, 2:2 + ref["nv"]].sum(), refc["stack"][:, :, 2:2 + ref["nv"]].sum()
    assert 0 < n_cut < n_all and np.array_equal(refc["stack"][:, :, :2], ref["stack"][:, :, :2])
    momc, stackc = call_var(dev, tr, iv, tbar, prm, (var[0], 3, 1, dcut), zabs=z)
    check(momc, stackc, refc, f"d_max {dcut}: {int(n_cut)} of {int(n_all)} pixels")


def test_the_host_cuts_a_call_into_launches_without_changing_the_result(dev):
    """4096 z-bins and 64 variance bins: a chunk's partial rows take 10 MB of the 64 MB a launch aims at, so that the 1200 segments of
    this call -- 19 chunks -- need several launches.  The stack is within the bar of the port's all the same"""
    from qfa_amd import _lib
    B, S, nb, L, nseg, nz = 400, 1, 64, 21, 3, 4096
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=43)
    bins = (1.6, np.float32(1.8 / nz), nz)
    prm = (0, L, nseg, 15, bins)
    ref, var = reference(g["zabs"], tr.cpu().numpy(), iv.cpu().numpy(), tbar, prm, 4, 4)
    need = _lib.lib().qfa_variance_workspace_bytes(B * S, S, nb, L, nseg, nz, 64)
    row = S * nz * (2 + 5 * 64) * 8                                                   # a chunk's partials
    assert 0 < need < (B * nseg + 63) // 64 * row                                     # fewer chunks than the call has: several launches
    assert ref["stack"][:, :, 0].sum() > 300 and (ref["stack"][:, :, 0] > 0).sum() > 100
    mom, stack = call_var(dev, tr, iv, tbar, prm, var, zabs=T(g["zabs"], dev), ws_bytes=need)
    check(mom, stack, ref, "launches")


def test_every_refusal_returns_its_code_and_touches_nothing(dev):
    B, S, nb, L, nseg = 4, 1, 60, 20, 2
    g, m, tr, iv, tbar = forest_case(dev, B, S, nb, seed=61)
    z = T(g["zabs"], dev)
    prm = (0, L, nseg, 10, BINS)
    var = (-8, 8, 1, R.FLT_MAX)

    refused = refusals(lambda **kw: call_var(dev, tr, iv, tbar, **kw), prm=prm, var=var, flags=F_ZERO, outs="ms", zabs=z)
    refused(-1, outs="")                                                              # both outputs missing
    refused(-1, zabs=None)                                                            # no redshift at all
    nan = float("nan")
    for bad in ((-8, 65, 0, 1.0), (-8, 5, 4, 1.0), (-8, 0, 1, 1.0), (-8, 8, 5, 1.0), (-8, 8, -1, 1.0), (-127, 8, 1, 1.0),
                (120, 8, 1, 1.0), (-8, 8, 1, nan), (-8, 8, 1, 0.0), (-8, 8, 1, -1.0)):
        refused(-2, var=bad)                                                          # nv = 65, e_lo + n_oct = 128, d_max = NaN, ...
    refused(-2, prm=(0, L, nseg, 0, BINS))                                            # min_used < 1
    refused(-2, prm=(21, L, nseg, 10, BINS))                                          # the segments pass Nb
    for flags in (0x1, 0x100, 0x400, 0x800, 0x2000):
        refused(-5, flags=flags)
    from qfa_amd import _lib
    need = _lib.lib().qfa_variance_workspace_bytes(B * S, S, nb, L, nseg, BINS[2], 16)
    refused(-3, ws_bytes=need - 1)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_variance_function_of_a_loader(dev):
    """QFA.variance_function on a resident loader at two batch sizes against the port run over the whole set; variance_segments in its
    tensor, factored and resident forms"""
    import torch
    from qfa_amd._lib import QFAHipError
    m, mk, wav = loader_case(dev)
    kw = dict(n_segments=2, seg_len=24, min_used_frac=0.75, tbar_nbins=8, seed=6)
    dl = mk(96)
    dv = 299792.458 * float(np.log(wav[1] / wav[0]))
    half = float(np.exp(0.5 * 25 * dv / 299792.458))
    tb1 = m.mean_transmission(dl, 2.8 / half - 1.0, 4.4 * half - 1.0, 8, batch_size=96)
    # the port over the whole set, on the transmission forest writes for it
    rb = dl.rows_batch(0, 96)[0]
    _, hm, _, _, unc = m.predict(batch=rb)
    tr, iv, _ = m.forest(batch=rb, hmean=hm, unc=unc)
    _, zfac = rb.materialize(raw_flux=True)
    zf = RP.z_factored(zfac[0].cpu().numpy(), zfac[1].cpu().numpy())
    tbn = tb1.mean.to(torch.float32).cpu().numpy()
    bins = (np.float32(1.8), np.float32(1.6 / 3), 3)
    probe = R.variance(tr.cpu().numpy(), iv.cpu().numpy(), zf, tbn, tb1.bins, 0, 24, 2, 18, bins, -126, 1, 0)
    e_lo = R.choose_bins(probe["v_all"], 6)
    ref = R.variance(tr.cpu().numpy(), iv.cpu().numpy(), zf, tbn, tb1.bins, 0, 24, 2, 18, bins, e_lo, 6, 1)
    assert ref["stack"][:, :, 0].sum() > 20 and (ref["moments"][..., 0, :].sum((0, 1, 2)) > 0).sum() >= 3
    a = m.variance_function(mk(96), 1.8, 3.4, 3, e_lo=e_lo, n_oct=6, tbar=tb1, batch_size=96, **kw)
    c = m.variance_function(mk(48), 1.8, 3.4, 3, e_lo=e_lo, n_oct=6, tbar=tb1, batch_size=40, **kw)
    for st, what in ((a, "batch 96"), (c, "batch 40")):
        assert st.S == 1 and st.L == 24 and st.nv == 12 and st.var_bins == (e_lo, 6, 1, R.FLT_MAX)
        check(None, st.buf.cpu().numpy(), ref, what)
    ft = a.fit(min_count=20)
    print(f"loader: n_bins {ft.n_bins.cpu().numpy().ravel()}, eta {ft.eta.cpu().numpy().ravel()}, sigma2 {ft.sigma2_lss.cpu().numpy().ravel()}")
    assert torch.isfinite(ft.eta).any() and torch.isfinite(ft.sigma2_lss).any() and torch.isfinite(ft.cov).any()
    # draws: S = 3 runs, and std_over_draws has the z-bins' shape
    d = m.variance_function(mk(96), 1.8, 3.4, 3, e_lo=e_lo, n_oct=6, n_samples=3, batch_size=96, **kw)
    assert d.S == 3 and d.n_segments.sum() > 20 * 3 and all(t.shape == (3,) for t in d.std_over_draws(min_count=20))
    # variance_segments: the resident form against the factored form of the same rows, and both against the loader's stack
    skw = dict(tbar=tb1, seg_len=24, n_segments=2, min_used=18, e_lo=e_lo, n_oct=6, bins=a.bins)
    m1, s1 = m.variance_segments(tr, iv, batch=rb, return_segments=True, **skw)
    m2, s2 = m.variance_segments(tr, iv, zfac=zfac, **skw)
    m3, s3 = m.variance_segments(tr, iv, zabs=T(zf, dev), return_segments=True, **skw)
    assert m2 is None and m1.shape == (96, 1, 2, 5, 12) and m1.dtype == torch.float64 and torch.equal(m1, m3)
    assert torch.equal(s1.buf, s2.buf) and torch.equal(s1.buf, s3.buf) and torch.equal(s1.buf, a.buf)
    check(m1.cpu().numpy(), s1.buf.cpu().numpy(), ref, "variance_segments")
    # adding onto a given stack; stack= must match in variance bins and d_max
    m.variance_segments(tr, iv, batch=rb, **{**skw, "bins": None}, stack=s1)
    assert torch.equal(s1.counts, 2 * s2.counts)
    for other in (dict(e_lo=e_lo + 1), dict(n_oct=3, sub=2), dict(d_max=1.0), dict(seg_len=23)):
        with pytest.raises(QFAHipError):
            m.variance_segments(tr, iv, batch=rb, **{**skw, "bins": None, **other}, stack=s1)
