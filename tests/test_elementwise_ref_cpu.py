"""The judges of tests/_elementwise_ref.py judged, without a GPU.

The numpy float32 oracle stands in for the implementation and the float64 oracle is the reference, over the very cases of
tests/test_predict_rows.py and tests/test_gradient_elements.py: it must pass at the bars (which are 8 x its own worst values,
profiles/elementwise_accuracy.txt), and each planted fault below -- the kind a wrong index or a dropped row in a kernel
produces -- must fail by at least 3 x its bar and be NAMED by element or row.  Two of the faults are also shown to the
whole-tensor rel-L2 at TOL_G, which does not see them: that is why the elementwise judge exists.
"""
import numpy as np
import pytest

import _elementwise_ref as E
from conftest import rel_l2

TOL_G = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5}             # (tests/test_hip_parity.py, tests/test_fuzz_shapes.py)
SHAPES = [(200, None, 16, 70), (640, None, 16, 48), (97, None, 9, 33)]


@pytest.fixture(scope="module")
def grads():
    """{shape: (float64 reference, float32 oracle)} of SHAPES, computed once; the tests copy what they change"""
    out = {}
    for c in SHAPES:
        p, mu, wav, nb, b, rows = E.gradient_case(*c)
        out[c] = (E.gradient_units(p, b, rows), E.gradient_units(p, b, rows, dtype=np.float32))
    return out


@pytest.fixture(scope="module")
def post():
    """(float64 reference, float32 oracle, index of the fully masked row) of one posterior case"""
    npix, nh, B = 97, 13, 63
    p, mu, wav, nb, b, rows = E.predict_case(npix, nh, B)
    return E.predict_rows(p, mu, b, rows), E.predict_rows(p, mu, b, rows, dtype=np.float32), B // 2


def units_of(ref, key, ours):
    return E.grad_error_units(ours, ref[key]["grad"], ref[key]["abssum"], ref[key]["count"])


def fails_naming(fn, *names):
    with pytest.raises(AssertionError) as ei:
        fn()
    for n in names:
        assert n in str(ei.value), (n, str(ei.value))


# ---------------------------------------------------------------------------------------------------------------------
# the float32 oracle passes, and nothing but count-0 elements / zero-uncertainty pixels is left out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.GRADIENT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_float32_oracle_passes_the_gradient_judge_on_every_case(case):
    p, mu, wav, nb, b, rows = E.gradient_case(*case)
    ref = E.gradient_units(p, b, rows)
    f32 = E.gradient_units(p, b, rows, dtype=np.float32)
    sel = E.select(b, rows)
    (a, e), none, last = E.thin_pixels(case[0])
    seen = sel["mask"].sum(axis=0)
    assert np.all(seen[a:e] == 1) and np.all(sel["mask"][-1, a:e]), "the block that only the last spectrum sees"
    assert seen[none] == 0 and seen[last] == 1 and sel["mask"][0, last]
    for k in E.GKEYS:
        n = ref[k]["grad"].shape[0]
        # every term of a seen pixel counts (no term is zero by accident), so the kernels' per-pixel count is the oracle's
        assert np.array_equal(ref[k]["count"], np.broadcast_to(seen[:n].reshape((n,) + (1,) * (ref[k]["count"].ndim - 1)),
                                                               ref[k]["count"].shape)), k
        u = units_of(ref, k, f32[k]["grad"])
        assert np.array_equal(np.isnan(u), ref[k]["count"] == 0), k           # only count-0 elements are left out
        E.check_gradient(k, f32[k]["grad"], ref, E.GRADIENT_BARS[k], counts=f32[k]["count"], what=str(case))


@pytest.mark.parametrize("case", E.PREDICT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_float32_oracle_passes_the_row_judge_on_every_case(case):
    npix, nh, B = case
    p, mu, wav, nb, b, rows = E.predict_case(*case)
    ref = E.predict_rows(p, mu, b, rows)
    assert np.all(ref["unc"] > 0), "no pixel of unc is left out on these inputs"
    assert all(np.isfinite(ref[k]).all() for k in E.PKEYS)
    if B >= 5:
        assert ref["nvalid"][B // 2] == 0 and not E.select(b, rows)["mask"][1, :nb].any()
        assert ref["ll"][B // 2] == 0 and not ref["hmean"][B // 2].any() and np.array_equal(ref["cont"][B // 2], mu.astype(np.float64))
    E.check_predict(E.predict_rows(p, mu, b, rows, dtype=np.float32), ref, E.PREDICT_BARS, what=str(case))


def test_the_tables_meet_every_group_edge_on_every_arm():
    for arm, lo, hi in ((8, 1, 8), (16, 9, 16), (32, 17, 32)):
        Bs = {B for npix, nh, B in E.PREDICT_CASES if lo <= nh <= hi}
        G = E.PREDICT_GROUP[arm]
        assert {1, 63, 64, 65, 129, 300, G - 1, G, G + 1, 2 * G + 1} <= Bs, (arm, sorted(Bs))
        assert {15, 16, 17} <= Bs, (arm, sorted(Bs))
    for nhs in ((1, 3, 8), (9, 13, 16), (17, 32)):
        assert set(nhs) <= {nh for npix, nh, B in E.PREDICT_CASES}
        assert {1913, 1920} <= {npix for npix, nh, B in E.PREDICT_CASES if nh in nhs}
    assert {33, 97, 333, 640} <= {npix for npix, nh, B in E.PREDICT_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: gradients
# ---------------------------------------------------------------------------------------------------------------------
def largest_dense(ref, key):
    g = np.where(ref[key]["count"] >= 2, np.abs(np.nan_to_num(ref[key]["grad"])), 0.0)
    return np.unravel_index(int(np.argmax(g)), g.shape)


def test_one_F_element_off_by_two_in_a_thousand_fails_where_the_whole_tensor_norm_passes(grads):
    blind = 0
    for c, (ref, f32) in grads.items():
        g = f32["F"]["grad"].astype(np.float64).copy()
        idx = largest_dense(ref, "F")
        g[idx] *= 1.002
        assert units_of(ref, "F", g)[idx] >= 3 * E.GRADIENT_BARS["F"][0], c
        fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"], what=str(c)), str(tuple(int(i) for i in idx)))
        ok = ~np.isnan(ref["F"]["grad"])
        blind += rel_l2(g[ok], ref["F"]["grad"][ok]) < TOL_G["F"]
    assert blind >= 1, "the whole-tensor rel-L2 at TOL_G was expected to miss this fault on at least one shape"


def test_a_dropped_term_of_Psi_fails(grads):
    for c, (ref, f32) in grads.items():
        p, mu, wav, nb, b, rows = E.gradient_case(*c)
        i = int(largest_dense(ref, "Psi")[0])
        s = int(np.flatnonzero(E.select(b, rows)["mask"][:, i])[0])                      # a spectrum that sees pixel i
        one = E.gradient_units(p, b, rows[s:s + 1])["Psi"]["sum"][i]
        g = f32["Psi"]["grad"].astype(np.float64).copy()
        g[i] -= one / ref["Psi"]["count"][i]
        assert units_of(ref, "Psi", g)[i] >= 3 * E.GRADIENT_BARS["Psi"][0], c
        fails_naming(lambda: E.check_gradient("Psi", g, ref, E.GRADIENT_BARS["Psi"]), f"({i},)")


def test_a_count_off_by_one_fails_by_its_count_and_by_its_value(grads):
    for c, (ref, f32) in grads.items():
        i = int(largest_dense(ref, "Psi")[0])
        cnt = f32["Psi"]["count"].copy()
        cnt[i] += 1
        fails_naming(lambda: E.check_gradient("Psi", f32["Psi"]["grad"], ref, E.GRADIENT_BARS["Psi"], counts=cnt),
                     f"count of element ({i},)")
        g = f32["Psi"]["grad"].astype(np.float64).copy()
        g[i] = f32["Psi"]["sum"][i] / cnt[i]
        assert units_of(ref, "Psi", g)[i] >= 3 * E.GRADIENT_BARS["Psi"][0], c
        fails_naming(lambda: E.check_gradient("Psi", g, ref, E.GRADIENT_BARS["Psi"]), f"({i},)")
        # and the pixel-level count that the kernels keep, against the (pixel, column) counts of F
        cpx = f32["Psi"]["count"].copy()
        cpx[i] -= 1
        fails_naming(lambda: E.check_gradient("F", f32["F"]["grad"], ref, E.GRADIENT_BARS["F"], counts=cpx), f"({i}, 0)")


def test_a_thin_pixel_given_another_pixels_value_fails_where_the_whole_tensor_norm_passes(grads):
    blind = 0
    for c, (ref, f32) in grads.items():
        (a, e), none, last = E.thin_pixels(c[0])
        assert np.all(ref["F"]["count"][a:e] == 1)
        r = ref["F"]["grad"]
        # the smallest element of the block that one spectrum sees takes the value of the next pixel in its column
        blk = np.abs(r[a:e - 1])
        i, col = np.unravel_index(int(np.argmin(blk)), blk.shape)
        i = int(i) + a
        g = f32["F"]["grad"].astype(np.float64).copy()
        g[i, col] = g[i + 1, col]
        assert units_of(ref, "F", g)[i, col] >= 3 * E.GRADIENT_BARS["F"][1], c
        fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"]), f"({i}, {int(col)})", "count 1")
        # the two neighbours of the block whose values are closest: the swap that a whole-tensor norm sees least
        d = np.abs(r[a:e - 1] - r[a + 1:e])
        i, col = np.unravel_index(int(np.argmin(d)), d.shape)
        i = int(i) + a
        g = f32["F"]["grad"].astype(np.float64).copy()
        g[i, col] = g[i + 1, col]
        ok = ~np.isnan(r)
        if rel_l2(g[ok], r[ok]) < TOL_G["F"] and units_of(ref, "F", g)[i, col] >= 3 * E.GRADIENT_BARS["F"][1]:
            blind += 1
            fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"]), f"({i}, {int(col)})")
    assert blind >= 1, "the whole-tensor rel-L2 at TOL_G was expected to miss this fault on at least one shape"


def test_count_zero_elements_are_nan_on_both_sides(grads):
    ref, f32 = grads[SHAPES[0]]
    (a, e), none, last = E.thin_pixels(SHAPES[0][0])
    u = units_of(ref, "F", f32["F"]["grad"])
    assert np.isnan(u[none]).all() and np.isnan(f32["F"]["grad"][none]).all()
    g = f32["F"]["grad"].astype(np.float64).copy()
    g[none, 2] = 0.0                                                                        # a number where the oracle has NaN
    assert np.isinf(units_of(ref, "F", g)[none, 2])
    fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"]), "NaN pattern", f"({none}, 2)")
    g = f32["F"]["grad"].astype(np.float64).copy()
    g[a, 1] = np.nan                                                                        # NaN where the oracle has a number
    fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"]), "NaN pattern", f"({a}, 1)")


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: the posterior
# ---------------------------------------------------------------------------------------------------------------------
def planted(f32, **changes):
    out = {k: np.array(f32[k], dtype=np.float64) for k in E.PKEYS}
    out.update(changes)
    return out


def test_two_rows_of_hmean_swapped_fail(post):
    ref, f32, dead = post
    h = np.array(f32["hmean"], dtype=np.float64)
    h[[5, 6]] = h[[6, 5]]
    errs = E.predict_row_errors(planted(f32, hmean=h), ref)
    assert errs["hmean"][5] >= 3 * E.PREDICT_BARS["hmean"] and errs["hmean"][6] >= 3 * E.PREDICT_BARS["hmean"]
    assert np.all(np.delete(errs["hmean"], [5, 6]) <= E.PREDICT_BARS["hmean"])
    fails_naming(lambda: E.check_predict(planted(f32, hmean=h), ref, E.PREDICT_BARS), "hmean", "row ")


def test_last_row_of_hcov_replaced_by_the_first_fails(post):
    ref, f32, dead = post
    B = len(ref["ll"])
    c = np.array(f32["hcov"], dtype=np.float64)
    c[B - 1] = c[0]
    errs = E.predict_row_errors(planted(f32, hcov=c), ref)
    assert int(np.argmax(errs["hcov"])) == B - 1 and errs["hcov"][B - 1] >= 3 * E.PREDICT_BARS["hcov"]
    fails_naming(lambda: E.check_predict(planted(f32, hcov=c), ref, E.PREDICT_BARS), "hcov", f"row {B - 1} of {B}")


def test_one_pixel_of_unc_off_by_one_in_a_thousand_fails_per_pixel_but_not_per_row_norm(post):
    ref, f32, dead = post
    u = np.array(f32["unc"], dtype=np.float64)
    u[7, 40] *= 1.001
    errs = E.predict_row_errors(planted(f32, unc=u), ref)
    assert int(np.argmax(errs["unc"])) == 7 and errs["unc"][7] >= 3 * E.PREDICT_BARS["unc"]
    fails_naming(lambda: E.check_predict(planted(f32, unc=u), ref, E.PREDICT_BARS), "unc", "row 7 of")
    assert rel_l2(u[7], ref["unc"][7]) < 1e-4                     # (the per-row rel-L2 the suite had: blind to it)


def test_cont_shifted_by_one_row_after_the_fully_masked_spectrum_fails(post):
    ref, f32, dead = post
    assert ref["nvalid"][dead] == 0 and ref["nvalid"][dead + 1] > 0
    c = np.array(f32["cont"], dtype=np.float64)
    c[dead + 1] = c[dead]                                         # the row after it is given the masked row's prior
    errs = E.predict_row_errors(planted(f32, cont=c), ref)
    assert int(np.argmax(errs["cont"])) == dead + 1 and errs["cont"][dead + 1] >= 3 * E.PREDICT_BARS["cont"]
    fails_naming(lambda: E.check_predict(planted(f32, cont=c), ref, E.PREDICT_BARS), "cont", f"row {dead + 1} of")


def test_a_nan_in_one_row_is_named(post):
    ref, f32, dead = post
    c = np.array(f32["cont"], dtype=np.float64)
    c[11, 3] = np.nan
    assert np.isinf(E.predict_row_errors(planted(f32, cont=c), ref)["cont"][11])
    fails_naming(lambda: E.check_predict(planted(f32, cont=c), ref, E.PREDICT_BARS), "cont", "(11, 3)")
