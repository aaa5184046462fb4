"""Every mean-optical-depth model and a spread of Lyman series through the kernels that read ``qfa_tau_t``.

The rest of the GPU suite runs becker, series 1 (one kamble forward aside).  Here the cases of tests/_tau_cases.py -- fg, kamble,
mock at series 1, becker at series 2 (offset x coefficient), kamble at series 5, becker at series 30 (A within ulps of 1), and
fg / kamble / mock once more at z_qso ~ U(4.5, 5.5), where tau reaches 2 to 3 -- go through the public surface
``QFA(..., tau=partial(utils.tau, which=w, series=s))`` into

* the training step: three input forms (zabs tensor, factored z, resident rows out of padded, poisoned storage) x every pass-2
  form (default, F_PASS2_PIXRES, F_PASS2_XDL, F_PASS2_F32 at N_h <= 16; one form at N_h = 17..32) x atomic / deterministic
  accumulation x ``exact_gradients`` off / on -- the full cross.  Reference mode: the per-spectrum NLL at TOL_NLL; F, Psi, omega
  element by element (``E.check_gradient``: the kernel's own ``cnt`` section, the NaN pattern, E.GRADIENT_BARS); tau0, c0, beta
  within TOL_SCAL = 1.5e-7 of their sum of |terms| against the float64 oracle on the DOUBLE constants -- but for kamble at
  z_qso ~ U(4.5, 5.5), which is judged against the oracle on the struct's FLOAT32 constants promoted to float64: against the
  double constants its factored and resident forms read 1.50e-7 .. 1.56e-7, against the struct's 1.0e-7; the excess is the
  rounding of expo and amp to float32, which the ABI fixes (TC.SCALARS_ON_STRUCT_CONSTANTS) --; whole tensors at TOL_G.  The
  references are computed once per case and set of redshifts (the zabs tensor | zq1 x pix_ratio) and shared by every run.
  Exact mode: the NLL, whole tensors at TOL_G and the three scalars at TOL_SCAL against tests/_exact_ref.py (its element sums
  are divided by B, not by a count, and a pixel nobody sees is 0: the element judge and its bars are the reference mode's).
  Deterministic mode: a second identical call returns the same bits of the packed buffer.
* the posterior: all rows, all five outputs (``E.check_predict``, E.PREDICT_BARS), both writers, the three input forms;
* the EM statistics (tests/_em_ref.py: ``em_terms`` / ``check_stat_elements``, STAT_BARS), zabs and factored form;
* mock spectra (tests/_mock_ref.py with the model's constants, the 1e-5 T bar of tests/test_mock_spectra.py);
* the template scan (tests/_dla_ref.py with the model, BAR and TIGHT of tests/test_dla_scan.py);
* the loader: ``set_tau`` on a loader built with becker, its resident delta / mu against the float64 port, then one step from
  ``next_batch_rows`` judged like the others.

Every run of a case is judged before anything fails: the assertion at the end lists each failed (form, quantity, element).
Achieved maxima: QFA_TAU_MODEL_LOG=<file> (profiles/tau_model_accuracy.txt).  The judges on the float32 oracle and the
attribution of the scalar bar to the float32 constants: tests/test_tau_models_cpu.py.
"""
from functools import partial

import numpy as np
import pytest

import _dla_ref as DR
import _elementwise_ref as E
import _em_ref as EM
import _exact_ref as X
import _mock_ref as MR
import _tau_cases as TC
from conftest import rel_l2
from oracle import qfa_oracle as O
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

TOL_NLL = 5e-6
TOL_G = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5}             # (whole tensors: tests/test_hip_parity.py)
TOL_SCAL = TC.TOL_SCAL
FORMS = ("zabs", "zfac", "rows")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def model_of(dev, which, series, nb, nr, nh, p, mu=None):
    import torch
    from qfa_amd import QFA, utils
    m = QFA(nb, nr, nh, dev, tau=partial(utils.tau, which=which, series=series), model_params=p)
    assert m._tau_callable is None                                         # a kernel model, not a host-evaluated A_blue
    want = TC.struct_f32(which, series)
    assert TC.struct_constants(m._tau_model) == tuple(float(c) for c in want), (which, series)
    if mu is not None:
        m.mu = torch.as_tensor(mu, device=dev).to(torch.float32)
    return m


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Inputs:
    """the three input forms of a batch of resident rows on the device (tests/test_gradient_elements.py)"""

    def __init__(self, dev, b, rows, wav, npix, nb, data="delta"):
        import torch
        from qfa_amd import synthetic
        from qfa_amd.resident import ResidentBatch
        N, B = len(b[data]), len(rows)
        d, er, mk = (torch.as_tensor(b[k], device=dev) for k in (data, "error", "mask"))
        self.idx = idx = torch.as_tensor(rows.astype(np.int64), device=dev)
        self.zq1 = zq1 = torch.as_tensor((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), device=dev)
        self.ratio = ratio = torch.as_tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev)
        stride = (npix + 31) // 32 * 32

        def pad(t, fill):
            out = torch.full((N, stride), fill, dtype=t.dtype, device=dev)
            out[:, :npix] = t
            return out
        rows32 = torch.as_tensor(rows.astype(np.int32), device=dev)
        if data == "delta":
            self.rb = ResidentBatch(None, pad(d, -7.0e9), pad(er, float("nan")), pad(mk, True), zq1, ratio, rows32, npix, nb)
        else:
            self.rb = ResidentBatch(pad(d, 3.0e9), None, pad(er, float("nan")), pad(mk, True), zq1, ratio, rows32, npix, nb)
        self.d, self.er, self.mk = d[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
        self.z = torch.as_tensor(b["zabs"][rows], device=dev).to(torch.float32).reshape(B, nb).contiguous()

    def args(self, form):
        """(positional arguments, keyword arguments) of accumulate / predict / em_statistics in an input form"""
        if form == "zabs":
            return (self.d, self.er, self.z, self.mk), {}
        if form == "zfac":
            return (self.d, self.er, None, self.mk), {"zfac": (self.zq1[self.idx].contiguous(), self.ratio)}
        return (), {"batch": self.rb}


def judge_reference_step(nll, packed, gr, ref, sc, scale, cnt_sl, what, fails):
    """one run of the reference mode: appends a line per missed bar to ``fails``; returns the record line's columns"""
    if not np.all(np.isfinite(nll)):
        fails.append(f"NLL {what}: not finite")
    err = float(np.max(np.abs(nll - ref["nll"]) / scale))
    if not err < TOL_NLL:
        fails.append(f"NLL {what}: spectrum {int(np.argmax(np.abs(nll - ref['nll']) / scale))} is {err:.3e} from the oracle (bar {TOL_NLL:.0e})")
    cols = [f"{err:8.2e}"]
    cnt = packed[cnt_sl]
    for k in E.GKEYS:
        try:
            worst = E.check_gradient(k, gr[k], ref, E.GRADIENT_BARS[k], counts=cnt[:gr[k].shape[0]], what=what)
        except AssertionError as e:
            fails.append(str(e))
            worst = (np.inf, np.inf)
        ok = ~np.isnan(ref[k]["grad"])
        whole = rel_l2(gr[k][ok], ref[k]["grad"][ok])
        if not whole < TOL_G[k]:
            fails.append(f"{k} {what}: whole tensor {whole:.3e} from the oracle (bar {TOL_G[k]:.0e})")
        cols.append(f"{worst[0]:8.2e} {worst[1]:8.2e} {whole:8.2e}")
    sca = []
    for k in TC.SKEYS:
        u = TC.scalar_units(gr[k], sc[k])
        if not u <= TOL_SCAL:
            fails.append(f"{k} {what}: ours {float(gr[k])!r}, oracle {sc[k][0] / max(sc[k][2], 1)!r}: {u:.3e} of the sum of |terms| "
                         f"(bar {TOL_SCAL:.1e})")
        sca.append(f"{u:8.2e}")
    cols.append(" ".join(sca))
    return cols


def judge_exact_step(nll, gr, ref_nll, og, ab, scale, dead, what, fails):
    err = float(np.max(np.abs(nll - ref_nll) / scale))
    if not (np.all(np.isfinite(nll)) and err < TOL_NLL):
        fails.append(f"NLL {what}: {err:.3e} from the oracle (bar {TOL_NLL:.0e})")
    cols = [f"{err:8.2e}"]
    for k in E.GKEYS:
        whole = rel_l2(gr[k], og[k]) if np.isfinite(gr[k]).all() else np.inf
        if not whole < TOL_G[k]:
            fails.append(f"{k} {what}: whole tensor {whole:.3e} from the closed form (bar {TOL_G[k]:.0e})")
        if dead < gr[k].shape[0] and np.any(gr[k][dead] != 0):
            fails.append(f"{k} {what}: pixel {dead}, which no spectrum sees, is not 0")
        cols.append(f"{whole:8.2e}")
    sca = []
    for k in TC.SKEYS:
        u = abs(float(gr[k]) - float(og[k])) / ab[k] if np.isfinite(gr[k]) else np.inf
        if not u <= TOL_SCAL:
            fails.append(f"{k} {what}: ours {float(gr[k])!r}, closed form {float(og[k])!r}: {u:.3e} of the sum of |terms| "
                         f"(bar {TOL_SCAL:.1e})")
        sca.append(f"{u:8.2e}")
    cols.append(" ".join(sca))
    return cols


def run_step(m, inp, form, flags, det, exact, B, dev):
    """(per-spectrum NLL, the packed buffer, the normalised gradients) as numpy"""
    import torch
    m.flags, m.deterministic, m.exact_gradients = flags, det, exact
    try:
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        a, kw = inp.args(form)
        acc = m.accumulate(*a, nll=nll, **kw).clone()
        packed = acc.cpu().numpy().copy()
        loss, gr = m._finalize(acc, True)
        return nll.cpu().numpy(), packed, {k: v.cpu().numpy().astype(np.float64) for k, v in gr.items()}
    finally:
        m.flags, m.deterministic, m.exact_gradients = 0, False, False


def pass2_forms(nh):
    forms = [(0, "default")]
    if nh <= 16:
        forms += [(_lib.F_PASS2_PIXRES, "pixres"), (_lib.F_PASS2_XDL, "xdl"), (_lib.F_PASS2_F32, "f32")]
    return forms


def step_cross(dev, m, inp, p, b, rows, which, series, tag, npix, nb, nh, input_forms=FORMS, on_struct=False):
    """the full cross of one (model, batch); returns the list of failures.  ``on_struct``: the three scalar gradients are judged
    against the oracle on the struct's float32 constants (TC.SCALARS_ON_STRUCT_CONSTANTS)"""
    from tools import parity_sections as PS
    B = len(rows)
    # The references, once per case.  Two sets of redshifts: the float32 zabs tensor, and 1 + z = zq1 x pix_ratio exactly
    # (float64 product of the float32 factors) for the factored and the resident form, which are GIVEN those factors --
    # float32(1 + z_qso) differs from the zabs tensor's by up to 6e-8 relative per SPECTRUM, which the scalar bar sees at tau = 2
    # (tests/test_exact_gradients.py judges its factored form the same way).  Every pass-2 form, accumulation and run shares them.
    zf = dict(b)
    zf["zabs"] = np.outer(inp.zq1.double().cpu().numpy(), inp.ratio.double().cpu().numpy()) - 1.0
    struct = TC.struct_constants(m._tau_model)
    refs = {}
    for key, bb in (("zabs", b), ("zfac", zf)):
        if key == "zabs" and "zabs" not in input_forms:
            continue
        ref, sc = TC.step_sums(p, bb, rows, which, series)
        sel = E.select(bb, rows)
        ol, og, ab = X.exact_forward(p, sel["delta"], sel["error"], sel["zabs"], sel["mask"], which, tau_series=series)
        # the same on the float32 constants the kernels were given (the attribution of tests/test_tau_models_cpu.py, measured)
        _, sc32 = TC.step_sums(p, bb, rows, struct)
        _, og32, ab32 = X.exact_forward(p, sel["delta"], sel["error"], sel["zabs"], sel["mask"], struct)
        refs[key] = (ref, sc, og, ab, sc32, og32, ab32)
    refs["rows"] = refs["zfac"]
    sel = E.select(b, rows)
    scale = np.maximum(np.maximum(np.abs(refs["zfac"][0]["nll"]), sel["mask"].sum(axis=1)), 1.0)
    dead = int(np.flatnonzero(sel["mask"].sum(axis=0) == 0)[0]) if (sel["mask"].sum(axis=0) == 0).any() else npix
    cnt_sl = PS.sections(m)["cnt"]
    fails = []
    for flags, name in pass2_forms(nh):
        for form in input_forms:
            for det in (False, True):
                for exact in (False, True):
                    what = f"({tag}; N_pix {npix}, N_b {nb}, N_h {nh}, B {B}; pass 2 {name}, {form}, " \
                           f"{'deterministic' if det else 'atomics'}, {'exact' if exact else 'reference'} gradients)"
                    nll, packed, gr = run_step(m, inp, form, flags, det, exact, B, dev)
                    ref, sc, og, ab, sc32, og32, ab32 = refs[form]
                    ud = [abs(float(gr[k]) - float(og[k])) / ab[k] if exact else TC.scalar_units(gr[k], sc[k]) for k in TC.SKEYS]
                    u32 = [abs(float(gr[k]) - float(og32[k])) / ab32[k] if exact else TC.scalar_units(gr[k], sc32[k]) for k in TC.SKEYS]
                    if on_struct:                       # (the scalars only: TC.SCALARS_ON_STRUCT_CONSTANTS says why)
                        sc, og, ab = sc32, dict(og, **{k: og32[k] for k in TC.SKEYS}), ab32
                    if exact:
                        cols = judge_exact_step(nll, gr, ref["nll"], og, ab, scale, dead, what, fails)
                    else:
                        cols = judge_reference_step(nll, packed, gr, ref, sc, scale, cnt_sl, what, fails)
                    cols[-1] = "double constants " + " ".join(f"{u:8.2e}" for u in ud) + " | struct's constants " + \
                               " ".join(f"{u:8.2e}" for u in u32) + (" (judged)" if on_struct else "")
                    TC.record(f"step {tag:22s} {name:7s} {form:4s} {'det ' if det else 'atom'} {'exact' if exact else 'ref  '} | "
                              + " | ".join(cols))
                    if det:
                        nll2, packed2, _ = run_step(m, inp, form, flags, det, exact, B, dev)
                        if not (same_bits(packed, packed2) and same_bits(nll, nll2)):
                            fails.append(f"{what}: a second identical call differs")
    return fails


@pytest.mark.parametrize("case", TC.STEP_CASES, ids=TC.case_id)
def test_training_step(dev, case):
    which, series, zr, shape = case
    npix, _, nh, B = shape
    p, mu, wav, nb, b, rows = TC.gradient_case(*case)
    m = model_of(dev, which, series, nb, npix - nb, nh, p)
    inp = Inputs(dev, b, rows, wav, npix, nb)
    fails = step_cross(dev, m, inp, p, b, rows, which, series, TC.case_id(case), npix, nb, nh,
                       on_struct=(which, series, zr) in TC.SCALARS_ON_STRUCT_CONSTANTS)
    assert not fails, f"{len(fails)} missed:\n" + "\n".join(fails)


@pytest.mark.parametrize("case", TC.PREDICT_CASES, ids=TC.case_id)
def test_posterior(dev, case):
    which, series, zr, shape = case
    npix, nh, B = shape
    p, mu, wav, nb, b, rows = TC.predict_case(*case)
    ref = E.predict_rows(p, mu, b, rows, tau_which=which, tau_series=series)  # (once per case: the forms share it)
    m = model_of(dev, which, series, nb, npix - nb, nh, p, mu)
    inp = Inputs(dev, b, rows, wav, npix, nb, data="flux")
    dead = B // 2
    fails = []
    for flags, writer in ((0, "xdl"), (_lib.F_PREDICT_F32, "f32")):
        m.flags = flags
        for form in FORMS:
            a, kw = inp.args(form)
            pred = dict(zip(E.PKEYS, (x.cpu().numpy() for x in m.predict(*a, **kw))))
            what = f"({TC.case_id(case)}; {form}, writer {writer})"
            errs = E.predict_row_errors(pred, ref)
            TC.record(f"predict {TC.case_id(case):22s} {form:4s} {writer:3s} | " + " ".join(f"{np.max(errs[k]):9.2e}" for k in E.PKEYS))
            try:
                E.check_predict(pred, ref, E.PREDICT_BARS, what=what)
                # no data: the prior (ll 0, h = 0, C = I, cont = mu)
                assert pred["ll"][dead] == 0.0 and not pred["hmean"][dead].any(), f"{what}: the fully masked row"
                assert np.max(np.abs(pred["hcov"][dead] - np.eye(nh))) <= E.PREDICT_BARS["hcov"], what
            except AssertionError as e:
                fails.append(str(e))
    m.flags = 0
    assert not fails, f"{len(fails)} missed:\n" + "\n".join(fails)


@pytest.mark.parametrize("case", TC.PREDICT_CASES, ids=TC.case_id)
def test_em_statistics(dev, case):
    which, series, zr, shape = case
    npix, nh, B = shape
    p, mu, wav, nb, b, rows = TC.predict_case(*case)
    sel = E.select(b, rows)
    m = model_of(dev, which, series, nb, npix - nb, nh, p)
    inp = Inputs(dev, b, rows, wav, npix, nb)
    zfac = ((1.0 + sel["zqso"].astype(np.float64)).astype(np.float32), inp.ratio.cpu().numpy())
    fails = []
    for form, zref in (("zabs", sel["zabs"]), ("zfac", EM.zabs_of(zfac)), ("rows", EM.zabs_of(zfac))):
        ref = EM.em_terms(p, sel["delta"], sel["error"], zref, sel["mask"], which, tau_series=series)
        a, kw = inp.args(form)
        st = m.em_statistics(*a, **kw)
        S2, S1 = st.S2.double().cpu().numpy(), st.S1.double().cpu().numpy()
        what = f"({TC.case_id(case)}; {form})"
        line = []
        for k, ours in (("S2", S2), ("S1", S1)):
            (w, _), (w1, _) = EM.class_worst(EM.stat_units(ours, ref[k], ref["abs" + k]), ref["cnt"])
            line.append(f"{w:8.2e} {w1:8.2e}")
        scale = np.maximum(np.maximum(np.abs(ref["nll"]), sel["mask"].sum(axis=1)), 1.0)
        TC.record(f"em {TC.case_id(case):22s} {form:4s} | " + " | ".join(line))
        try:
            EM.check_stat_elements(S2, S1, st.cnt.cpu().numpy(), ref, what=what)
            assert abs(float(st.tail[0]) - ref["nll_sum"]) <= TOL_NLL * float(scale.sum()), f"{what}: the sum of the NLL"
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, f"{len(fails)} missed:\n" + "\n".join(fails)


@pytest.mark.parametrize("variant", TC.VARIANTS, ids=lambda v: f"{v[0]}{v[1]}-{v[2]}")
def test_mock_spectra(dev, variant):
    """every unmasked element of flux and delta within 1e-5 T of the float64 port at the model's constants (series coefficient in
    amp and offset), T = A (|mu| + sum |F h|) + sqrt(D) |e| -- the bar of tests/test_mock_spectra.py"""
    import torch
    which, series, zr = variant
    npix, nh, B = 333, 13, 16
    S, seed, row0 = 2, 4321, 2 ** 33 + 5
    p, mu, wav, nb, b, rows = TC.predict_case(which, series, zr, (npix, nh, B))
    sel = E.select(b, rows)
    m = model_of(dev, which, series, nb, npix - nb, nh, p, mu)
    inp = Inputs(dev, b, rows, wav, npix, nb)
    zq1, ratio = (1.0 + sel["zqso"].astype(np.float64)).astype(np.float32), inp.ratio.cpu().numpy()
    consts = TC.tau_constants(which, series)
    use = np.broadcast_to(sel["mask"][:, None, :], (B, S, npix))
    fails = []
    for form, zp1 in (("zabs", 1.0 + sel["zabs"].astype(np.float64)), ("zfac", np.outer(zq1.astype(np.float64), ratio.astype(np.float64)))):
        if form == "zabs":
            flux, delta, h = m.sample_spectra(inp.er, inp.z, inp.mk, n_samples=S, seed=seed, offset=row0, return_delta=True,
                                              return_latent=True)
        else:
            flux, delta, h = m.sample_spectra(inp.er, None, inp.mk, n_samples=S, seed=seed, offset=row0, return_delta=True,
                                              return_latent=True, zfac=(inp.zq1[inp.idx].contiguous(), inp.ratio))
        want = MR.spectra(p, mu, sel["error"], zp1, sel["mask"], h.cpu().numpy(), seed, row0, tau=consts)
        for key, out in (("flux", flux), ("delta", delta)):
            got = out.cpu().numpy().astype(np.float64)
            rel = np.abs(got - want[key])[use] / want["T"][use]
            TC.record(f"mock {which}{series}-{zr} {form:4s} {key:5s} | {rel.max():.3e}")
            if not (rel <= 1e-5).all():
                bad = np.argwhere((np.abs(got - want[key]) > 1e-5 * want["T"]) & use)[0]
                fails.append(f"{key} ({which}{series}-{zr}; {form}): element {tuple(int(i) for i in bad)} is {rel.max():.3e} T from float64")
            if not (got[~use] == -999.0).all():
                fails.append(f"{key} ({which}{series}-{zr}; {form}): a masked element is not the sentinel")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", TC.VARIANTS, ids=lambda v: f"{v[0]}{v[1]}-{v[2]}")
def test_template_scan(dev, variant):
    """the (133, 64, 16) shape and the 5 x 3 grid of tests/test_dla_scan.py, spectra drawn from the model with an injected DLA,
    against tests/_dla_ref.py at the model: |llr - float64| <= TIGHT x BAR max(|NLL0|, |NLL'|)"""
    import torch
    from qfa_amd import synthetic
    from test_dla_scan import TIGHT, grid_kw
    which, series, zr = variant
    npix, nb, nh, B = 133, 64, 16, 3
    wav = np.concatenate([np.geomspace(1030.0, 1214.0, nb), np.geomspace(1217.0, 1600.0, npix - nb)])
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=npix + nh)
    m = model_of(dev, which, series, nb, npix - nb, nh, p, mu)
    d = DR.draw(p, mu, wav, nb, B, seed=7 * npix + nh, snr=(5.0, 100.0), tau_which=which, tau_series=series)
    if zr == "hiz":                                    # (DR.draw draws z_qso in [2.2, 3.4]: the same spectra seen from further away)
        d["zqso"] = d["zqso"] + 2.3
        d["zabs"] = ((1.0 + d["zqso"])[:, None] * wav[None, :nb] / DR.LYA - 1.0).astype(np.float32)
    g = grid_kw(5, 3)
    lam, logn = DR.centres(1190.0, g["dv_kms"], 5), np.array([20.0, 20.6, 21.2])
    flux, error, _, _ = DR.inject(d, wav, lam, logn, seed=nh)
    V = m.dla_profiles(wav, **g)
    T = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    llr, nll0, best_c, best_llr = m.template_scan(T(flux), T(error), T(d["zabs"]), T(d["mask"]), V)
    rl, r0, rn = DR.scan(p, mu, flux, error, d["zabs"], d["mask"], V.cpu().numpy(), which, series)
    bar = DR.BAR * np.maximum(np.abs(r0)[:, None], np.abs(rn))
    err = np.abs(llr.cpu().numpy().astype(np.float64) - rl)
    TC.record(f"scan {which}{series}-{zr} | llr max err / bar {float(np.max(err / bar)):.3f} | nll0 "
              f"{float(np.max(np.abs(nll0.cpu().numpy() - r0) / np.abs(r0))):.2e}")
    bad = np.argwhere(err > TIGHT * bar)
    assert bad.size == 0, f"llr ({which}{series}-{zr}): (spectrum, candidate) {tuple(int(i) for i in bad[0])} is " \
                          f"{float(np.max(err / bar)):.3f} of the bar from float64 (allowed {TIGHT})"
    assert np.all(np.abs(nll0.cpu().numpy() - r0) <= TOL_NLL * np.abs(r0))
    assert np.array_equal(best_c.cpu().numpy(), np.argmax(llr.cpu().numpy(), axis=1))


@pytest.mark.parametrize("which", ["fg", "kamble", "mock"])
def test_loader_set_tau_then_a_step(dev, which):
    """A loader built with becker and then given another model: mu and the resident delta against the float64 port of the
    reference's host preprocessing (tests/test_device_dataloader.py), then one step from next_batch_rows on the loader's own
    arrays, judged as in test_training_step (a factor table kept from the earlier model would show in either)."""
    import torch
    from qfa_amd import utils
    from qfa_amd.dataloader import DeviceDataloader
    p, mu0, wav, nb, b = TC.loader_case(which)
    npix, nh, N = len(wav), p["F"].shape[1], len(b["flux"])
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, batch_size=N, device=dev, shuffle=False)
    mu_becker = dl.mu.copy()
    dl.set_tau(partial(utils.tau, which=which))
    raw, mu = O.mu_estimate(wav, b["flux"].astype(np.float64), b["mask"], b["zqso"], nb, which=which)
    assert rel_l2(dl.mu, mu) < 1e-6 and rel_l2(mu_becker, mu) > 1e-3, (rel_l2(dl.mu, mu), rel_l2(mu_becker, mu))
    want = O.delta_from_flux(wav, b["flux"].astype(np.float64), b["zqso"], dl.mu, nb, which=which)
    dl.rewind()
    rb = dl.next_batch_rows()
    delta = rb.delta[:, :npix].cpu().numpy()
    ok = b["mask"]
    assert np.array_equal(rb.mask[:, :npix].cpu().numpy(), ok)
    err = np.max(np.abs(delta[ok] - want[ok])) / np.max(np.abs(want[ok]))
    TC.record(f"loader {which}: mu {rel_l2(dl.mu, mu):.2e}, delta {err:.2e} of its maximum")
    assert err < 5e-7, err
    # one step on the loader's own delta: the model's tau at series 1 on zabs of the loader's factors
    rows = rb.rows.cpu().numpy().astype(np.int64)
    bb = {"delta": delta, "error": b["error"], "mask": ok, "zqso": b["zqso"],
          "zabs": O.zabs_from_zqso(wav, b["zqso"], nb).astype(np.float32)}
    m = model_of(dev, which, 1, nb, npix - nb, nh, p)

    class Rows:
        zq1, ratio = rb.zq1, rb.pix_ratio

        def args(self, form):
            return (), {"batch": rb}
    fails = step_cross(dev, m, Rows(), p, bb, rows, which, 1, f"loader-{which}", npix, nb, nh, input_forms=("rows",))
    assert not fails, f"{len(fails)} missed:\n" + "\n".join(fails)
