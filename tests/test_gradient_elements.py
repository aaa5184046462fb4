"""Every element of the per-pixel gradients F, Psi, omega of every pass-2 form against the float64 oracle.

The other gradient tests compare whole tensors (rel-L2 at TOL_G): the measure of overall float32 quality, which one wrong
element of 10 000 does not move past its bar and which is blind to elements that are small next to the tensor's rms
(tests/test_elementwise_ref_cpu.py shows both).  Here every element is read in units of its own sum of |terms|
(tests/_elementwise_ref.py, ``grad_error_units``), its count -- the kernel's own, the ``cnt`` section of the packed buffer that
``k_finalize`` divides by -- must be the oracle's exactly, and the NaN pattern (0 / 0 of a pixel that no spectrum sees) too.
Shapes from the ragged, boundary and XDL tables of tests/test_hip_parity.py; forms: default dispatch, F_PASS2_PIXRES, F_PASS2_XDL,
F_PASS2_F32 (N_h <= 16; N_h = 17..32 has one form); input forms: zabs tensor, factored z, resident rows; ``exact_gradients``
off.  On top of the masks with runs: a block of pixels that only the last spectrum sees, a pixel that none sees, and the last
pixel of the last ragged tile seen by the first spectrum only.  A failure names the (pixel, column), its count and its units.

Bars, their float32-oracle reference values and the maxima the kernels achieve: profiles/elementwise_accuracy.txt.
"""
import numpy as np
import pytest

import _elementwise_ref as E
from conftest import rel_l2
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

TOL_NLL = 5e-6
TOL_G = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5}             # (whole tensors: tests/test_hip_parity.py)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("npix,nb,nh,B", E.GRADIENT_CASES)
def test_every_gradient_element_against_the_oracle(dev, npix, nb, nh, B):
    import torch
    from qfa_amd import QFA, synthetic
    from qfa_amd.resident import ResidentBatch
    from tools import parity_sections as PS
    p, mu, wav, nb, b, rows = E.gradient_case(npix, nb, nh, B)
    ref = E.gradient_units(p, b, rows)                                         # (once per case: forms and input forms share it)
    sel = E.select(b, rows)
    scale = np.maximum(np.maximum(np.abs(ref["nll"]), sel["mask"].sum(axis=1)), 1.0)
    f32 = torch.float32
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    assert m.exact_gradients is False
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
    rb = ResidentBatch(None, pad(d, -7.0e9), pad(er, float("nan")), pad(mk, True), zq1, ratio,
                       torch.as_tensor(rows.astype(np.int32), device=dev), npix, nb)
    sd, ser, smk = d[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
    z = torch.as_tensor(sel["zabs"], device=dev).to(f32).reshape(B, nb).contiguous()
    forms = [(0, "default")]
    if nh <= 16:
        forms += [(_lib.F_PASS2_PIXRES, "pixres"), (_lib.F_PASS2_XDL, "xdl"), (_lib.F_PASS2_F32, "f32")]
    cnt_sl = PS.sections(m)["cnt"]
    for flags, name in forms:
        m.flags = flags
        for form in ("zabs", "zfac", "rows"):
            nll = torch.empty(B, dtype=f32, device=dev)
            if form == "zabs":
                acc = m.accumulate(sd, ser, z, smk, nll=nll)
            elif form == "zfac":
                acc = m.accumulate(sd, ser, None, smk, nll=nll, zfac=(zq1[idx].contiguous(), ratio))
            else:
                acc = m.accumulate(batch=rb, nll=nll)
            acc = acc.clone()
            cnt = acc[cnt_sl].cpu().numpy()                                     # the count that k_finalize divides by, per pixel
            loss, gr = m._finalize(acc, True)
            what = f"(N_pix {npix}, N_b {nb}, N_h {nh}, B {B}; pass 2 {name}, {form})"
            ours_nll = nll.cpu().numpy()
            assert np.all(np.isfinite(ours_nll)), what
            assert np.max(np.abs(ours_nll - ref["nll"]) / scale) < TOL_NLL, what
            line = []
            for k in E.GKEYS:
                ours, r = gr[k].cpu().numpy(), ref[k]["grad"]
                worst = E.check_gradient(k, ours, ref, E.GRADIENT_BARS[k], counts=cnt[:ours.shape[0]], what=what)
                ok = ~np.isnan(r)
                whole = rel_l2(ours[ok], r[ok])
                assert whole < TOL_G[k], (k, what, whole)                       # the whole-tensor bar stays: overall quality
                line.append(f"{worst[0]:9.2e} {worst[1]:9.2e} {whole:9.2e}")
            E.record(f"gradient {npix:4d} {nb:3d} {nh:2d} {B:3d} {name:7s} {form:4s} | " + " | ".join(line))
    m.flags = 0
