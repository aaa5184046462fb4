"""Stage 3 of the pixel-resident pass 2 (k_grads_t, qfa_grads_t.h) contracts PAIRS of spectrum groups at N_h = 9..16: the K = 32 of
an MFMA holds the 16 spectra of groups 2 i and 2 i + 1, the Z image belongs to the pair (qfa_gt_layout.h), ranges start at even
groups, and a batch with an odd number of groups ends in a lone group whose area holds its own lower and upper column tiles, contracted
in two passes with zeros in the other half of beta.  N_h <= 8 (two
pixel tiles per wave) keeps the per-group contraction behind GTT::PAIR; it runs the same cases.

The smallest shapes at which the pairing can go wrong: one group (a pair with an empty half), a second group of one spectrum, one
full pair, three groups, and 16 (2 R + 1) spectra in two ranges or more by the library's own plan (``odd_even_batch``, ``plan_ranges``:
even ranges and an odd last one); N_pix = 40 with N_b = 20 (a ragged last tile, the blue / red boundary inside a tile) and N_pix = 128,
N_b = 48.  ``F_PASS2_PIXRES`` forces the kernel onto these sizes.  Every element of F, Psi, omega, the counts, the three scalar
gradients and the per-spectrum NLL are judged against the float64 oracle under the bars of tests/test_gt_walk_edges.py, and the
scalars against k_grads_x (``F_PASS2_XDL``) on the same input.  Before every call the workspace (the state images live there) is
filled with 0xFF bytes -- NaN patterns in float32 and float16: a stale beta or Z in a half no group owns would surface as a
NaN.  In the exact-gradient mode F, Psi, omega, the counts and the NLL are judged in the same way and the three scalars against the
float64 closed form of tests/_exact_ref.py.
"""
import numpy as np
import pytest

import _elementwise_ref as E
from qfa_amd import _lib
from test_gt_walk_edges import SKEYS, TOL_FORMS, TOL_NLL, TOL_SCALAR, oracle_sums

pytestmark = pytest.mark.gpu

PIXELS = ((40, 20), (128, 48))
NHS = (16, 12, 8, 5)


def plan_ranges(nh, B, npix, det=False):
    """groups of 16 spectra per range of the launch, read from the library's own plan (qfa_pixres_plan, include/qfa_hip.h)"""
    import ctypes as C
    R, gpr = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().qfa_pixres_plan(int(B), int(npix), int(nh), int(det), C.byref(R), C.byref(gpr)), "qfa_pixres_plan")
    G = -(-B // 16)
    groups = [min(gpr.value, G - r * gpr.value) for r in range(R.value)]
    assert sum(groups) == G and all(n > 0 for n in groups), (B, R.value, gpr.value)
    return groups


def odd_even_batch(nh, npix):
    """B = 16 (2 R + 1) for the smallest R >= 2 at which the library's plan has two ranges or more"""
    for R in range(2, 64):
        B = 16 * (2 * R + 1)
        if len(plan_ranges(nh, B, npix)) >= 2:
            return B
    raise AssertionError("no batch of 16 (2 R + 1) spectra in two ranges or more")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Case:
    """one batch on the device, its float64 sums (once), and a runner of the kernels over its input forms"""

    def __init__(self, dev, npix, nb, nh, B):
        import torch
        from qfa_amd import QFA, synthetic
        from qfa_amd.resident import ResidentBatch
        from tools import parity_sections as PS
        self.torch = torch
        self.what = f"N_pix {npix}, N_b {nb}, N_h {nh}, B {B}"
        p, mu, wav, nb, b, rows = E.gradient_case(npix, nb, nh, B)
        self.B, self.nb, self.p = B, nb, p
        self.ref, self.sc = oracle_sums(p, b, rows)
        self.sel = sel = E.select(b, rows)
        self.scale = np.maximum(np.maximum(np.abs(self.ref["nll"]), sel["mask"].sum(axis=1)), 1.0)
        self.m = m = QFA(nb, npix - nb, nh, dev, model_params=p)
        N = len(b["delta"])
        d, er, mk = (torch.as_tensor(b[k], device=dev) for k in ("delta", "error", "mask"))
        idx = torch.as_tensor(rows.astype(np.int64), device=dev)
        zq1 = torch.as_tensor((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), device=dev)
        ratio = torch.as_tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev)
        stride = (npix + 31) // 32 * 32

        def pad(t, fill):
            out = torch.full((N, stride), fill, dtype=t.dtype, device=dev)
            out[:, :npix] = t
            return out
        self.rb = ResidentBatch(None, pad(d, -7.0e9), pad(er, float("nan")), pad(mk, True), zq1, ratio,
                                torch.as_tensor(rows.astype(np.int32), device=dev), npix, nb)
        self.sd, self.ser, self.smk = d[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
        self.z = torch.as_tensor(sel["zabs"], device=dev).to(torch.float32).reshape(B, nb).contiguous()
        self.zfac = (zq1[idx].contiguous(), ratio)
        self.cnt_sl = PS.sections(m)["cnt"]

    def run(self, flags, form="zabs", det=False, exact=False):
        torch, m = self.torch, self.m
        m.flags, m.deterministic, m.exact_gradients = flags, det, exact
        try:
            m._workspace(self.B).fill_(0xFF)                   # NaN patterns where the state images will be written
            nll = torch.empty(self.B, dtype=torch.float32, device=self.sd.device)
            if form == "zabs":
                acc = m.accumulate(self.sd, self.ser, self.z, self.smk, nll=nll)
            elif form == "zfac":
                acc = m.accumulate(self.sd, self.ser, None, self.smk, nll=nll, zfac=self.zfac)
            else:
                acc = m.accumulate(batch=self.rb, nll=nll)
            acc = acc.clone()
            cnt = acc[self.cnt_sl].cpu().numpy()
            loss, gr = m._finalize(acc.clone(), True)
            return nll.cpu().numpy(), cnt, {k: v.cpu().numpy() for k, v in gr.items()}, acc.cpu().numpy()
        finally:
            m.flags, m.deterministic, m.exact_gradients = 0, False, False

    def judge(self, form="zabs", det=False):
        what = f"({self.what}; {form}, {'deterministic' if det else 'atomics'})"
        nll_t, cnt, gt, _ = self.run(_lib.F_PASS2_PIXRES, form, det)
        _, _, gx, _ = self.run(_lib.F_PASS2_XDL, form, det)
        ref, sc = self.ref, self.sc
        assert np.all(np.isfinite(nll_t)), what
        assert np.max(np.abs(nll_t - ref["nll"]) / self.scale) < TOL_NLL, what
        for k in E.GKEYS:
            assert not np.any(np.isnan(gt[k]) & ~np.isnan(ref[k]["grad"])), (k, what, "NaN where the oracle has a value")
            E.check_gradient(k, gt[k], ref, E.GRADIENT_BARS[k], counts=cnt[:gt[k].shape[0]], what=what)
        for k in SKEYS:
            total, absum, n = sc[k]
            assert np.isfinite(gt[k]) == np.isfinite(gx[k]) == (n > 0), (k, what, gt[k], gx[k], n)
            if n > 0 and absum > 0:
                for kernel, ours in (("k_grads_t", gt[k]), ("k_grads_x", gx[k])):
                    units = abs(float(ours) - total / n) * n / absum
                    assert units <= TOL_SCALAR, f"{k} {what}: {kernel} {float(ours)!r}, oracle {total / n!r}: {units:.3e} (bar {TOL_SCALAR:.0e})"
                units = abs(float(gt[k]) - float(gx[k])) * n / absum
                assert units <= TOL_FORMS, f"{k} {what}: k_grads_t {float(gt[k])!r}, k_grads_x {float(gx[k])!r}: {units:.3e} apart (bar {TOL_FORMS:.0e})"


def batches(nh, npix):
    return (16, 17, 32, 48, odd_even_batch(nh, npix))


@pytest.mark.parametrize("nh", NHS)
@pytest.mark.parametrize("npix,nb", PIXELS)
@pytest.mark.parametrize("which", range(5))
def test_pairs_against_the_oracle_and_k_grads_x(dev, npix, nb, nh, which):
    B = batches(nh, npix)[which]
    if which == 4 and nh > 8:                                  # an even range and an odd one
        groups = plan_ranges(nh, B, npix)
        assert len(groups) >= 2 and any(n % 2 for n in groups) and any(n % 2 == 0 for n in groups), (B, groups)
    Case(dev, npix, nb, nh, B).judge()


@pytest.fixture(scope="module")
def case48(dev):
    return Case(dev, 128, 48, 16, 48)


@pytest.mark.parametrize("form", ("zfac", "zabs", "rows"))
def test_forms_at_three_groups(case48, form):
    case48.judge(form)


def test_exact_gradients_at_three_groups(case48):
    """exact_gradients=True: Psi, omega, the counts and the per-spectrum NLL are the sums of the reference mode (tests/
    test_exact_gradients.py asserts their bits) and are judged element by element like them -- the packed buffer read as a
    reference-mode buffer: its count of exact-mode launches, slot -2, set to 0.  F is another quantity there (the gradient of the mean
    NLL: 0 where no spectrum observes a pixel) and has no per-element bars: it and the three scalars of both kernels are judged
    against the float64 closed form of tests/_exact_ref.py by the measures and under the bars of tests/test_exact_gradients.py (F
    1e-4, Psi / omega 2e-5 relative L2; tau0 / c0 / beta 1.5e-7 of the sum of |terms|), the scalars of the two kernels within twice
    that of each other"""
    import torch
    import _exact_ref as X
    from test_exact_gradients import TOL, TOL_SCAL, rel_l2
    c, m = case48, case48.m
    sel = c.sel
    ol, og, ab = X.exact_forward(c.p, sel["delta"], sel["error"], sel["zabs"], sel["mask"])
    got = {}
    for kernel, flags in (("k_grads_t", _lib.F_PASS2_PIXRES), ("k_grads_x", _lib.F_PASS2_XDL)):
        what = f"({c.what}; exact, {kernel})"
        nll, cnt, gex, acc = c.run(flags, exact=True)
        assert np.all(np.isfinite(nll)) and np.max(np.abs(nll - c.ref["nll"]) / c.scale) < TOL_NLL, what
        asref = torch.as_tensor(acc, device=m.device).clone()
        assert asref[-2].item() == c.B, what
        asref[-2] = 0.0
        _, gref = m._finalize(asref, True)
        for k in ("Psi", "omega"):
            E.check_gradient(k, gref[k].cpu().numpy(), c.ref, E.GRADIENT_BARS[k], counts=cnt[:gref[k].shape[0]], what=what)
        for k in E.GKEYS:
            assert np.isfinite(gex[k]).all(), (k, what)
            assert rel_l2(gex[k], og[k]) < TOL[k], (k, what, rel_l2(gex[k], og[k]))
        for k in SKEYS:
            err = abs(float(gex[k]) - float(og[k]))
            assert err <= TOL_SCAL * ab[k], f"{k} {what}: {float(gex[k])!r}, closed form {float(og[k])!r}: {err / ab[k]:.3e} of the sum of |terms| (bar {TOL_SCAL:.1e})"
        got[kernel] = gex
    for k in SKEYS:
        err = abs(float(got["k_grads_t"][k]) - float(got["k_grads_x"][k]))
        assert err <= 2 * TOL_SCAL * ab[k], (k, got["k_grads_t"][k], got["k_grads_x"][k], err / ab[k])


@pytest.mark.parametrize("B", (16, 48))
def test_deterministic_mode_repeats_bit_for_bit(dev, B):
    c = Case(dev, 40, 20, 16, B)
    c.judge(det=True)
    a = c.run(_lib.F_PASS2_PIXRES, det=True)[3]
    b = c.run(_lib.F_PASS2_PIXRES, det=True)[3]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
