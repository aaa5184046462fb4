"""The judges of tests/test_em_elements.py judged on the CPU (tests/_em_ref.py): the matrix-product restatement of the statistics
against the per-spectrum one, the row-by-row solve against em_update, the plan arithmetic of the cases past the fold from the
exported byte counts alone, the conventions of stat_units, the planted rows of the solve test under the kernel's skip rule --
and that the element judge sees a fault the whole-tensor norm does not."""
import numpy as np
import pytest

import _em_ref as E
from conftest import rel_l2

TOL_STAT = 2e-5          # the rel-L2 bar of tests/test_em_step.py


def small_case(npix=203, nh=4, B=70, seed=223, **kw):
    p, b, dead, wav, nb, zfac = E.em_inputs(npix, nh, B, seed, **kw)
    return p, b, dead


@pytest.mark.parametrize("npix,nh,B", [(203, 4, 70), (130, 17, 40), (45, 5, 2)])
def test_em_terms_is_em_statistics(npix, nh, B):
    p, b, dead = small_case(npix, nh, B, seed=npix + 5 * nh)
    want = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])
    got = E.em_terms(p, b["delta"], b["error"], b["zabs"], b["mask"])
    for k in ("S2", "S1", "cnt", "nll"):
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=0), k
    assert got["nll_sum"] == want["nll_sum"] and got["n"] == want["n"]
    assert np.array_equal(got["S2"], np.swapaxes(got["S2"], 1, 2))
    assert (got["absS2"] >= np.abs(got["S2"]) * (1 - 1e-12)).all() and (got["absS1"] >= np.abs(got["S1"]) * (1 - 1e-12)).all()
    assert ((got["absS2"] == 0) == (got["cnt"] == 0)[:, None, None]).all()
    # the absolute sums, the slow way
    s = E.em_statistics(p, b["delta"][:1], b["error"][:1], b["zabs"][:1], b["mask"][:1])
    t = E.em_terms(p, b["delta"][:1], b["error"][:1], b["zabs"][:1], b["mask"][:1])
    assert np.allclose(t["absS2"], np.abs(s["S2"]), rtol=1e-12, atol=0) and np.allclose(t["absS1"], np.abs(s["S1"]), rtol=1e-12, atol=0)


def test_em_terms_takes_a_blue_and_float32():
    p, b, dead = small_case()
    ab = E.a_blue_of(b["zabs"])
    want = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"], A_blue=ab)
    got = E.em_terms(p, b["delta"], b["error"], b["zabs"], b["mask"], A_blue=ab)
    assert np.allclose(got["S2"], want["S2"], rtol=1e-12, atol=0) and np.allclose(got["S1"], want["S1"], rtol=1e-12, atol=0)
    f32 = E.em_terms(p, b["delta"], b["error"], b["zabs"], b["mask"], A_blue=ab, dtype=np.float32)
    assert f32["S2"].dtype == np.float32 and f32["S1"].dtype == np.float32 and np.array_equal(f32["cnt"], got["cnt"])
    u = E.stat_units(f32["S2"], got["S2"], got["absS2"])
    assert 0 < u.max() < E.STAT_BARS["S2"][0]                         # float32 arithmetic, and under the bar measured with it


def test_stat_units_conventions():
    ref = np.array([1.0, -2.0, 0.0, 0.0, 3.0, 4.0])
    ab = np.array([2.0, 4.0, 0.0, 0.0, 3.0, 4.0])
    ours = np.array([1.5, -2.0, 0.0, 1e-30, np.nan, np.inf])
    u = E.stat_units(ours, ref, ab)
    assert u[0] == 0.25 and u[1] == 0 and u[2] == 0 and np.isinf(u[3]) and np.isinf(u[4]) and np.isinf(u[5])
    assert E.worst_element(np.array([[0.0, 2.0], [1.0, np.nan]])) == ((1, 1), np.inf)
    (w, i), (w1, i1) = E.class_worst(np.array([[1.0, 2.0], [5.0, 0.0], [3.0, 4.0]]), np.array([2, 1, 0]))
    assert (w, i, w1, i1) == (4.0, (2, 1), 5.0, (1, 0))


def test_the_judge_sees_what_the_norm_cannot():
    """one element of S2 at the pixel of the lowest weight off by 20 x its bar: under the rel-L2 bar, far over its own"""
    p, b, dead = small_case(333, 8, 257, seed=333 + 40)
    ref = E.em_terms(p, b["delta"], b["error"], b["zabs"], b["mask"])
    dense = ref["cnt"] >= 2
    i = int(np.argmin(np.where(dense, ref["absS2"][:, 0, 0], np.inf)))
    bar = E.STAT_BARS["S2"][0]
    bad = ref["S2"].copy()
    bad[i, 0, 0] += 20 * bar * ref["absS2"][i, 0, 0]
    bad[i, 2, 1] -= 20 * bar * ref["absS2"][i, 2, 1]
    assert rel_l2(bad, ref["S2"]) <= TOL_STAT
    out = E.class_worst(E.stat_units(bad, ref["S2"], ref["absS2"]), ref["cnt"])
    assert out[0][1][0] == i and out[0][0] == pytest.approx(20 * bar, rel=1e-6)
    with pytest.raises(AssertionError, match=rf"element \({i}, "):
        E.check_stat_elements(bad, ref["S1"], ref["cnt"], ref)
    E.check_stat_elements(ref["S2"], ref["S1"], ref["cnt"], ref)
    with pytest.raises(AssertionError, match="cnt of pixel 5"):
        c = ref["cnt"].copy(); c[5] += 1
        E.check_stat_elements(ref["S2"], ref["S1"], c, ref)


def test_solve_rows_is_em_update_on_well_conditioned_input():
    p, b, dead = small_case(160, 4, 64, seed=3)
    st = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])
    s32 = (st["S2"].astype(np.float32), st["S1"].astype(np.float32), st["cnt"].astype(np.float32))
    s64 = {"S2": s32[0].astype(np.float64), "S1": s32[1].astype(np.float64), "cnt": s32[2].astype(np.float64)}
    for ridge, damping in E.SOLVE_RIDGE_DAMPING:
        want, nsk = E.em_update(p["F"], s64, ridge, damping)
        got, skipped, cond, x = E.solve_rows(s32, p["F"], ridge, damping)
        assert int(skipped.sum()) == nsk == int((st["cnt"] == 0).sum())
        assert np.array_equal(skipped, st["cnt"] == 0)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12)
        assert np.array_equal(got[skipped], np.asarray(p["F"], np.float64)[skipped])
        assert np.isnan(cond[skipped]).all() and (cond[~skipped] >= 1).all() and cond[~skipped].max() < 1e4
        # the derived bar holds between two float64 solves of the same system (numpy's general solver against Cholesky)
        direct = np.array([np.linalg.solve(s64["S2"][i] + ridge * np.eye(4), s64["S1"][i]) if not skipped[i] else np.zeros(4)
                           for i in range(160)])
        alt = np.where(skipped[:, None], got, np.asarray(p["F"], np.float64) + damping * (direct - p["F"]))
        bar = E.solve_bar(got, np.where(skipped[:, None], 0.0, x), np.where(skipped, 0.0, cond), 4, damping)
        assert (np.abs(alt - got) <= bar).all()


@pytest.mark.parametrize("nh", E.SOLVE_NH)
def test_planted_rows_of_the_solve_case(nh):
    for npix in E.SOLVE_NPIX:
        S2, S1, cnt, F, planted = E.solve_case(npix, nh)
        assert S2.dtype == S1.dtype == cnt.dtype == F.dtype == np.float32
        good = np.array([i not in planted.values() for i in range(npix)])
        assert np.array_equal(S2[good], np.swapaxes(S2[good], 1, 2))
        ev = np.linalg.eigvalsh(S2[good].astype(np.float64))
        assert (ev[:, 0] > 0).all() and (ev[:, -1] / ev[:, 0] < 1.2e6).all()
        if nh > 1 and npix >= 64:
            assert (ev[:, -1] / ev[:, 0]).max() > 1e3                 # the conditions are spread
        for ridge, damping in E.SOLVE_RIDGE_DAMPING:
            out, skipped, cond, x = E.solve_rows((S2, S1, cnt), F, ridge, damping)
            assert not skipped[good].any()
            if ridge == 0.0:
                assert skipped[~good].all(), (npix, nh, [k for k, i in planted.items() if not skipped[i]])
            assert np.array_equal(out[skipped], F.astype(np.float64)[skipped])
            if damping == 0.0:
                assert np.array_equal(out, F.astype(np.float64))
        if "rank" in planted:
            i = planted["rank"]
            A = S2[i].astype(np.float64)
            assert np.linalg.matrix_rank(A) == nh - 1
            if nh > 1:
                np.linalg.cholesky(A[:-1, :-1])                         # every leading pivot but the last is positive
        out, skipped, _, _ = E.solve_rows((S2, S1, cnt), F, 1e301, 1.0)
        assert skipped.all()


def test_the_solve_bar_rejects_a_float32_solve():
    """the same rows solved with float32-grade backward error: far over the bar wherever the row is badly conditioned; and one
    element of the best-conditioned row off by 3 float32 ulps is seen as well"""
    S2, S1, cnt, F, planted = E.solve_case(130, 16)
    want, skipped, cond, x = E.solve_rows((S2, S1, cnt), F, 0.0, 1.0)
    bar = E.solve_bar(want, np.where(skipped[:, None], 0.0, x), np.where(skipped, 0.0, cond), 16, 1.0)
    hard = np.flatnonzero(~skipped & (cond > 1e4))
    assert hard.size >= 20
    rng = np.random.default_rng(0)
    def backward32(A):                                   # a solve whose backward error is one float32 rounding per element
        P = np.tril(rng.uniform(-1.0, 1.0, size=A.shape)) * 2.0 ** -24
        return A.astype(np.float64) * (1.0 + P + np.tril(P, -1).T)
    f32 = np.array([np.linalg.solve(backward32(S2[i]), S1[i].astype(np.float64)) for i in hard])
    over = (np.abs(f32 - want[hard]) / bar[hard]).max(axis=1)
    print("a float32-grade solve of the rows with cond > 1e4: |error| / bar from", over.min(), "to", over.max())
    assert (over > 3).all(), over.min()
    i = int(np.nanargmin(cond))
    got = want.astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want) <= bar)[~skipped].all()
    got[i, 3] = np.nextafter(np.nextafter(np.nextafter(got[i, 3], np.float32(np.inf)), np.float32(np.inf)), np.float32(np.inf))
    assert np.abs(got[i, 3].astype(np.float64) - want[i, 3]) > bar[i, 3]


def test_plan_arithmetic_of_the_cases_past_the_fold():
    """R, per and the last range of em_plan recovered from qfa_em_workspace_bytes / qfa_workspace_bytes, which need no device"""
    from qfa_amd import _lib
    h = _lib.lib()
    B, npix = E.FOLD_B, E.FOLD_NPIX
    for nh, form in E.FOLD_CASES:
        R, per, last = E.plan_from_bytes(h.qfa_em_workspace_bytes(B, npix, nh), h.qfa_workspace_bytes(B, npix, nh), B, npix, nh)
        assert (R, per, last) == (E.FOLD_R, E.FOLD_PER, 201), (nh, R, per, last)
        assert per > 256 and last % 4 != 0 and (B % per) % 4 != 0
    # the shapes of tests/test_em_step.py stay on this side of the fold -- (97, 8, 4096) exactly on it
    pers = {}
    for n, k, Bs in E.SHAPES:
        if Bs > 256:                                     # (below, one range holds the batch: per <= 256 as it is)
            R, per, last = E.plan_from_bytes(h.qfa_em_workspace_bytes(Bs, n, k), h.qfa_workspace_bytes(Bs, n, k), Bs, n, k)
            pers[n, k, Bs] = per
    assert max(pers.values()) == 256 and pers[97, 8, 4096] == 256 and pers[333, 8, 257] == 132 and pers[75, 16, 1030] == 208
    # the planted columns of fold_plant
    mask = np.ones((B, npix), bool)
    E.fold_plant(mask)
    s = np.arange(B)
    assert mask[:, E.FOLD_COLUMNS["late"]].sum() == 4 * 15 and (s[mask[:, E.FOLD_COLUMNS["late"]]] % 260 >= 256).all()
    assert mask[:, E.FOLD_COLUMNS["early"]].sum() == 15 * 256 + 201
    assert s[mask[:, E.FOLD_COLUMNS["single"]]].tolist() == [B - 1]
    assert mask.sum() == B * (npix - 3) + 60 + 15 * 256 + 201 + 1
