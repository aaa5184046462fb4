"""Every row of the posterior, all five outputs, against the float64 oracle (reference QFA/model.py:160-180).

The other posterior tests judge a handful of rows (tests/test_hip_parity.py: B <= 20, or rows 0, B // 2, B - 1) and never
``hmean`` / ``hcov`` past the 20th row.  Here B sits on the edges of the groups the kernels cut a batch into (pass 1: blocks of
64 and waves of 16 spectra; the solve: 32 / 16 / 8 per block; the writers: 64 per block, 128 at N_h = 9..16 with two groups of
16 per wave -- tests/_elementwise_ref.py, PREDICT_GROUP), on every N_h arm (<= 8, 9..16, 17..32), through the three input forms
(zabs tensor, factored z, resident rows picked by a permutation from padded, poisoned storage) and both writers (flags = 0,
F_PREDICT_F32); the batch holds masks with runs, a fully masked spectrum in the middle of a group, a red-only one, a pixel
masked everywhere and a spectrum with errors of 1e-4 of its flux.  ALL B rows are judged by tests/_elementwise_ref.py
(``predict_row_errors``: ll, hmean, hcov, cont per row, unc per PIXEL), and a failure names the row.

Bars, their float32-oracle reference values and the maxima the kernels achieve: profiles/elementwise_accuracy.txt.
"""
import numpy as np
import pytest

import _elementwise_ref as E
from qfa_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("npix,nh,B", E.PREDICT_CASES)
def test_every_row_of_the_posterior_against_the_oracle(dev, npix, nh, B):
    import torch
    from qfa_amd import QFA, synthetic
    from qfa_amd.resident import ResidentBatch
    p, mu, wav, nb, b, rows = E.predict_case(npix, nh, B)
    ref = E.predict_rows(p, mu, b, rows)                                       # (once per case: the forms share it)
    f32 = torch.float32
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    m.mu = torch.as_tensor(mu, device=dev).to(f32)
    N = len(b["flux"])
    fx, er, mk = (torch.as_tensor(b[k], device=dev) for k in ("flux", "error", "mask"))
    idx = torch.as_tensor(rows.astype(np.int64), device=dev)
    zq1 = torch.as_tensor((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), device=dev)
    ratio = torch.as_tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev)
    stride = (npix + 31) // 32 * 32

    def pad(t, fill):
        out = torch.full((N, stride), fill, dtype=t.dtype, device=dev)
        out[:, :npix] = t
        return out
    rb = ResidentBatch(pad(fx, 3.0e9), None, pad(er, float("nan")), pad(mk, True), zq1, ratio,
                       torch.as_tensor(rows.astype(np.int32), device=dev), npix, nb)
    sfx, ser, smk = fx[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
    z = torch.as_tensor(b["zabs"][rows], device=dev).to(f32).reshape(B, nb).contiguous()
    dead = B // 2 if B >= 5 else None
    for flags, writer in ((0, "xdl"), (_lib.F_PREDICT_F32, "f32")):
        m.flags = flags
        for form in ("zabs", "zfac", "rows"):
            if form == "zabs":
                pred = m.predict(sfx, ser, z, smk)
            elif form == "zfac":
                pred = m.predict(sfx, ser, None, smk, zfac=(zq1[idx].contiguous(), ratio))
            else:
                pred = m.predict(batch=rb)
            pred = dict(zip(E.PKEYS, (x.cpu().numpy() for x in pred)))
            what = f"(N_pix {npix}, N_h {nh}, B {B}; {form}, writer {writer})"
            worst = E.check_predict(pred, ref, E.PREDICT_BARS, what=what)
            if dead is not None:                        # no data: the prior, as the oracle gives it (ll 0, h = 0, C = I, cont = mu)
                assert pred["ll"][dead] == 0.0 and not pred["hmean"][dead].any(), what
                assert np.max(np.abs(pred["hcov"][dead] - np.eye(nh))) <= E.PREDICT_BARS["hcov"], what
                assert np.max(np.abs(pred["cont"][dead] - mu)) <= E.PREDICT_BARS["cont"] * np.max(np.abs(mu)), what
            E.record(f"predict {npix:5d} {nh:2d} {B:3d} {form:4s} {writer:3s} | " + " ".join(f"{worst[k]:9.2e}" for k in E.PKEYS))
    m.flags = 0
