"""The judges of tests/test_tau_models.py judged without a GPU, on exactly the cases of tests/_tau_cases.py.

* The numpy float32 oracle stands in for the kernels and the float64 oracle is the reference: it must pass every bar the GPU
  tests apply (E.GRADIENT_BARS, E.PREDICT_BARS -- which are 8 x its own worst values on the becker cases, so that at a new
  model it has to stay inside them with the project's usual factor of 8 to spare for the kernels: asserted at 1 / 8 x 8 = the
  bar itself here, and the fraction used is printed).
* ``emulate_A`` / ``emulate_A_factored`` (float32 restatements of ``blue_terms`` and of the factored form with correctly
  rounded log2 / exp2) are handed to the float64 oracle as ``A_blue``: how far the float32 constants of ``qfa_tau_t`` and the
  float32 chain alone move the three scalar gradients, in units of their sum of |terms|, per model -- the attribution table
  behind TOL_SCAL = 1.5e-7.  Each must stay inside the bar (a kernel could not pass otherwise).
* The struct: every field of the four models x series {1, 2, 5, 30} is float32(double constant x series coefficient).
* ``draw`` is synthetic.make_batch_numpy at becker, series 1, z_qso ~ U(2, 3.5), bit for bit.
"""
import numpy as np
import pytest

import _elementwise_ref as E
import _tau_cases as TC
from oracle import qfa_oracle as O
from qfa_amd import synthetic


def test_draw_is_the_synthetic_generator_at_becker_series_1():
    wav, nb, nr = synthetic.wavelength_grid(97)
    p, mu = synthetic.mock_parameters(97, nb, 3, seed=4)
    for masks in (False, True):
        a = synthetic.make_batch_numpy(p, mu, wav, nb, 9, seed=44, masks=masks)
        b = TC.draw(p, mu, wav, nb, 9, 44, masks=masks)
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    p0, mu0, wav0, nb0, b0, rows0 = E.gradient_case(333, None, 5, 17)
    p1, mu1, wav1, nb1, b1, rows1 = TC.gradient_case("becker", 1, "std", (333, None, 5, 17))
    assert nb0 == nb1 and np.array_equal(rows0, rows1) and all(np.array_equal(b0[k], b1[k]) for k in b0)
    p0, mu0, wav0, nb0, b0, rows0 = E.predict_case(97, 8, 17)
    p1, mu1, wav1, nb1, b1, rows1 = TC.predict_case("becker", 1, "std", (97, 8, 17))
    assert nb0 == nb1 and np.array_equal(rows0, rows1) and all(np.array_equal(b0[k], b1[k]) for k in b0)


def test_the_table_holds_what_the_docstring_says():
    assert len(TC.VARIANTS) == 9 and len(TC.STEP_CASES) == 27 and len(TC.PREDICT_CASES) == 27
    assert {nh for _, _, nh, _ in TC.STEP_SHAPES} == {5, 16, 24} and {nh for _, nh, _ in TC.PREDICT_SHAPES} == {8, 13, 17}
    for which, series, zr in TC.VARIANTS:
        wav, nb, nr = synthetic.wavelength_grid(333)
        lo, hi = TC.Z_RANGE[zr]
        tau_max = O.tau_eff((1.0 + hi) * wav[nb - 1] / synthetic.LYA - 1.0, which, series)
        if zr == "hiz":
            assert tau_max > 2.0, (which, tau_max)
        elif (which, series) == ("becker", 30):
            assert tau_max < 3e-4, tau_max                  # 1 - A is a few thousand float32 ulps of 1 at most
        else:
            assert tau_max < 0.75, (which, series, tau_max)
    # becker at series 2: both amp and offset carry a coefficient that is not 1
    amp, scale, expo, off = TC.tau_constants("becker", 2)
    assert off != 0 and abs(off / O.TAU_MODELS["becker"][3] - O.LYMAN_COEFF[1]) < 1e-15 and 0.1 < O.LYMAN_COEFF[1] < 0.2


@pytest.mark.parametrize("case", TC.STEP_CASES, ids=TC.case_id)
def test_float32_oracle_passes_the_gradient_judge_and_the_constants_stay_inside_the_scalar_bar(case):
    which, series, zr, shape = case
    p, mu, wav, nb, b, rows = TC.gradient_case(*case)
    ref, sc = TC.step_sums(p, b, rows, which, series)
    f32, _ = TC.step_sums(p, b, rows, which, series, dtype=np.float32)
    sel = E.select(b, rows)
    (a, e), none, last = E.thin_pixels(shape[0])
    seen = sel["mask"].sum(axis=0)
    assert np.all(seen[a:e] == 1) and seen[none] == 0 and seen[last] == 1
    used = {}
    for k in E.GKEYS:
        worst = E.check_gradient(k, f32[k]["grad"], ref, E.GRADIENT_BARS[k], counts=f32[k]["count"], what=TC.case_id(case))
        used[k] = (worst[0] / E.GRADIENT_BARS[k][0], worst[1] / E.GRADIENT_BARS[k][1])
    print(f"{TC.case_id(case)}: float32 oracle, fraction of the bar (dense, one term): " +
          "  ".join(f"{k} {u[0]:.3f} {u[1]:.3f}" for k, u in used.items()))
    # the attribution: A as the kernels form it from the float32 struct, correctly rounded transcendentals, into the float64 oracle
    t32 = TC.struct_f32(which, series)
    zq1 = (1.0 + b["zqso"].astype(np.float64)).astype(np.float32)
    ratio = (wav[:nb] / synthetic.LYA).astype(np.float32)
    forms = {
        "constants": np.exp(-O.tau_eff(sel["zabs"].astype(np.float64), tuple(float(c) for c in t32))),     # float64 arithmetic
        "zabs": TC.emulate_A(sel["zabs"], t32).astype(np.float64),
        "factored": TC.emulate_A_factored(zq1[rows], ratio, t32).astype(np.float64),
    }
    A64 = np.exp(-O.tau_eff(sel["zabs"].astype(np.float64), which, series))
    for name, A in forms.items():
        _, sca = TC.step_sums(p, b, rows, which, series, A_blue=A)
        shift = {k: abs(sca[k][0] - sc[k][0]) / sc[k][1] for k in TC.SKEYS}
        bias = float(np.mean(A / A64 - 1.0))
        print(f"{TC.case_id(case)}: {name:9s} mean relative error of A {bias:+.2e}; scalar gradients moved by " +
              " ".join(f"{k} {v:.2e}" for k, v in shift.items()) + f" of sum|terms| (bar {TC.TOL_SCAL:.1e})")
        assert max(shift.values()) <= TC.TOL_SCAL, (name, shift)


@pytest.mark.parametrize("case", TC.PREDICT_CASES, ids=TC.case_id)
def test_float32_oracle_passes_the_row_judge(case):
    which, series, zr, shape = case
    p, mu, wav, nb, b, rows = TC.predict_case(*case)
    ref = E.predict_rows(p, mu, b, rows, tau_which=which, tau_series=series)
    assert all(np.isfinite(ref[k]).all() for k in E.PKEYS) and np.all(ref["unc"] > 0)
    worst = E.check_predict(E.predict_rows(p, mu, b, rows, dtype=np.float32, tau_which=which, tau_series=series), ref,
                            E.PREDICT_BARS, what=TC.case_id(case))
    print(f"{TC.case_id(case)}: float32 oracle, fraction of the bar: " +
          "  ".join(f"{k} {worst[k] / E.PREDICT_BARS[k]:.3f}" for k in E.PKEYS))


@pytest.mark.parametrize("case", TC.PREDICT_CASES, ids=TC.case_id)
def test_float32_restatement_passes_the_em_judge(case):
    import _em_ref as EM
    which, series, zr, shape = case
    p, mu, wav, nb, b, rows = TC.predict_case(*case)
    sel = E.select(b, rows)
    ref = EM.em_terms(p, sel["delta"], sel["error"], sel["zabs"], sel["mask"], which, tau_series=series)
    f32 = EM.em_terms(p, sel["delta"], sel["error"], sel["zabs"], sel["mask"], which, tau_series=series, dtype=np.float32)
    w = EM.check_stat_elements(f32["S2"], f32["S1"], f32["cnt"], ref, what=TC.case_id(case))
    print(f"{TC.case_id(case)}: float32 restatement, fraction of the bar (dense, one term): " +
          "  ".join(f"{k} {w[k][0][0] / EM.STAT_BARS[k][0]:.3f} {w[k][1][0] / EM.STAT_BARS[k][1]:.3f}" for k in ("S2", "S1")))


@pytest.mark.parametrize("which", ["fg", "kamble", "mock"])
def test_float32_oracle_passes_the_gradient_judge_on_the_loader_batch(which):
    p, wav, nb, b = TC.loader_batch(which)
    rows = np.arange(len(b["delta"]))
    ref, _ = TC.step_sums(p, b, rows, which, 1)
    f32, _ = TC.step_sums(p, b, rows, which, 1, dtype=np.float32)
    for k in E.GKEYS:
        E.check_gradient(k, f32[k]["grad"], ref, E.GRADIENT_BARS[k], counts=f32[k]["count"], what=f"loader {which}")


def test_a_wrong_offset_coefficient_or_scale_fails_the_judges():
    """the two faults the GPU tests exist for, planted in the oracle's constants: the offset of becker, series 2, left without its
    coefficient; log2(scale) of mock replaced by becker's.  Both must fail the per-spectrum NLL bar by a wide margin."""
    for (which, series), wrong in ((("becker", 2), lambda c: (c[0], c[1], c[2], O.TAU_MODELS["becker"][3])),
                                   (("mock", 1), lambda c: (c[0], O.TAU_MODELS["becker"][1], c[2], c[3]))):
        case = (which, series, "std", TC.STEP_SHAPES[0])
        p, mu, wav, nb, b, rows = TC.gradient_case(*case)
        ref, _ = TC.step_sums(p, b, rows, which, series)
        bad, _ = TC.step_sums(p, b, rows, wrong(TC.tau_constants(which, series)))
        good, _ = TC.step_sums(p, b, rows, TC.tau_constants(which, series))
        scale = np.maximum(np.maximum(np.abs(ref["nll"]), E.select(b, rows)["mask"].sum(axis=1)), 1.0)
        assert np.max(np.abs(good["nll"] - ref["nll"]) / scale) < 1e-12
        assert np.max(np.abs(bad["nll"] - ref["nll"]) / scale) > 100 * 5e-6, (which, series)


def test_struct_fields_are_float32_of_the_double_products():
    """qfa_tau_model (host code of the library: no GPU is touched): amp and offset carry the series coefficient, every field is
    the float32 nearest to the float64 product, so within half a float32 ulp of it"""
    from qfa_amd import _lib
    for which in _lib.TAU_IDS:
        for series in (1, 2, 5, 30):
            t = _lib.tau_model(which, series)
            want = TC.tau_constants(which, series)
            for name, w in zip(("amp", "scale", "expo", "offset"), want):
                got = getattr(t, name)
                assert np.float32(got) == np.float32(w), (which, series, name, got, w)
                assert abs(float(got) - w) <= 0.5 * float(np.spacing(np.float32(abs(w)))) + 0.0, (which, series, name)
    with pytest.raises(_lib.QFAHipError):
        _lib.tau_model("becker", 31)
    with pytest.raises(_lib.QFAHipError):
        _lib.tau_model("becker", 0)
