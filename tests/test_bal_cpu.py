"""CPU-side checks of the BAL finder: the numpy restatement (tests/_bal_ref.py) on analytic profiles, the host's window and argument
checks, BALScan's hand-over to mask_absorbers, the csv round trip, and the condition on the GPU tests' seeded inputs."""
import numpy as np
import pytest

import _bal_cases as K
import _bal_ref as R

THR = 0.9


def rect(v1, v2, d, *, dv=1.0, v_end=26000.0, masked=(), max_gap=0, smooth=1, indices=(R.BI, R.AI)):
    """the reference on a rectangular trough of depth d over [v1, v2) km/s, pixels of dv km/s from 0 on, noise-free, c exact"""
    n = int(round(v_end / dv))
    vedge = np.arange(n + 1) * dv
    r = np.where((vedge[:-1] >= v1) & (vedge[1:] <= v2), 1.0 - d, 1.0)
    used = np.ones(n, bool)
    for a, b in masked:
        used[int(round(a / dv)):int(round(b / dv))] = False
    z = np.zeros(n)
    return R.scan_row(np.where(used, r, 0.0), z, np.where(used, 0.01, 0.0), z, used, vedge, indices, THR, smooth, max_gap, len(indices) - 1)


def test_rectangular_trough_gives_the_closed_forms():
    d, v1, v2 = 0.6, 5000.0, 11000.0
    o = rect(v1, v2, d)
    depth = 1.0 - (1.0 - d) / THR
    assert o["value"][0] == pytest.approx(depth * (v2 - max(v1, 3000.0) - 2000.0), rel=1e-12)
    assert o["value"][1] == pytest.approx(depth * (v2 - v1), rel=1e-12)
    assert o["counts"][0] == (4000, 1, 0) and o["counts"][1] == (6000, 1, 0)
    assert o["n_troughs"] == 1 and tuple(o["troughs"][0]) == (v1, v2) and np.isnan(o["troughs"][1:]).all()
    # var at smooth = 1: thr^-2 sum (sigma / c)^2 width^2
    assert o["var"][1] == pytest.approx(6000 * 0.01 ** 2 / THR ** 2, rel=1e-12)
    assert not o["contested"] and o["n_used"] == 26000


@pytest.mark.parametrize("width,bi,ai", [(1999.0, False, True), (2001.0, True, True), (449.0, False, False), (451.0, False, True)])
def test_minimum_widths_fall_on_either_side(width, bi, ai):
    o = rect(6000.0, 6000.0 + width, 0.5)
    depth = 1.0 - 0.5 / THR
    assert (o["value"][0] > 0) == bi and (o["value"][1] > 0) == ai
    assert o["counts"][0][1] == int(bi) and o["counts"][1][1] == int(ai)
    if bi:
        assert o["value"][0] == pytest.approx(depth * (width - 2000.0), rel=1e-12)
    if ai:
        assert o["value"][1] == pytest.approx(depth * width, rel=1e-12)


def test_troughs_that_straddle_the_ends_of_the_range():
    depth = 1.0 - 0.5 / THR
    o = rect(1000.0, 7000.0, 0.5)                               # over 3 000 km/s: BI counts from 3 000 + 2 000 on, AI the whole trough
    assert o["value"][0] == pytest.approx(depth * 2000.0, rel=1e-12) and o["value"][1] == pytest.approx(depth * 6000.0, rel=1e-12)
    o = rect(22000.0, 25900.0, 0.5)                             # over 25 000 km/s: both stop there
    assert o["value"][0] == pytest.approx(depth * 1000.0, rel=1e-12) and o["value"][1] == pytest.approx(depth * 3000.0, rel=1e-12)
    assert tuple(o["troughs"][0]) == (22000.0, 25000.0)
    # coarse pixels that the ends of the range cut: the clipped widths, not whole pixels
    o = rect(0.0, 26000.0, 0.5, dv=1300.0)
    assert o["value"][0] == pytest.approx(depth * (25000.0 - 5000.0), rel=1e-12)
    assert o["value"][1] == pytest.approx(depth * 25000.0, rel=1e-12)


def test_bridging():
    """a trough of 3 000 km/s with a masked stretch inside: it is one run iff the stretch has at most max_gap pixels"""
    dv, depth = 100.0, 1.0 - 0.5 / THR
    for gap_px in (1, 3, 4):
        for max_gap in (0, 1, 3):
            o = rect(6000.0, 9000.0, 0.5, dv=dv, masked=((7000.0, 7000.0 + gap_px * dv),), max_gap=max_gap)
            joined = gap_px <= max_gap
            below_w = 3000.0 - gap_px * dv
            assert o["counts"][1] == (int(below_w / dv), 1 if joined else 2, gap_px if joined else 0), (gap_px, max_gap)
            assert o["value"][1] == pytest.approx(depth * below_w, rel=1e-12)
            # BI: joined, the run is 3 000 km/s wide and the 1 000 beyond 8 000 count; split, neither part reaches 2 000
            assert o["value"][0] == pytest.approx(depth * 1000.0 if joined else 0.0, rel=1e-12, abs=0.0)
    # a masked stretch at the run's end is no bridge: nothing below follows it
    o = rect(6000.0, 9000.0, 0.5, dv=dv, masked=((9000.0, 9200.0),), max_gap=3)
    assert o["counts"][1] == (30, 1, 0) and tuple(o["troughs"][0]) == (6000.0, 9000.0)


def test_boxcar_and_its_variance():
    """smooth = 3 on a flat trough: interior values unchanged, and var is the window sum applied to width / n"""
    dv = 100.0
    o1, o3 = rect(6000.0, 9000.0, 0.5, dv=dv), rect(6000.0, 9000.0, 0.5, dv=dv, smooth=3)
    # r~ = (1 + 0.5 + 0.5) / 3 = 0.667 < thr on the pixel outside either edge: the run grows by one pixel on both sides
    assert o3["counts"][1] == (32, 1, 0) and o1["counts"][1] == (30, 1, 0)
    a = np.zeros(262)
    w = np.zeros(262); w[59:91] = dv
    for q in range(1, 261):
        a[q] = w[q - 1:q + 2].sum() / 3.0
    assert o3["var"][1] == pytest.approx((0.01 * a) @ (0.01 * a) / THR ** 2, rel=1e-9)


def test_window_of_the_host_equals_the_reference_and_refuses_the_blue_side():
    from qfa_amd._lib import QFAHipError
    from qfa_amd.bal import check_indices, check_scan_params, velocity_window
    wav = 10 ** np.arange(np.log10(1100.0), np.log10(1620.0), 2e-4)
    nb = int(np.sum(wav < 1215.67))
    for lam in (1549.06, 1396.76):
        p_lo, p_hi, vedge = velocity_window(wav, lam, 0.0, 25000.0, nb)
        assert nb <= p_lo < p_hi <= len(wav) and np.all(np.diff(vedge) > 0)
        assert np.array_equal(vedge, R.window(wav, lam, p_lo, p_hi))
        assert vedge[0] <= 0.0 < vedge[1] and vedge[-2] < 25000.0 <= vedge[-1]
    with pytest.raises(QFAHipError):
        velocity_window(wav, 1240.81, 0.0, 25000.0, nb)         # N V: the window crosses Ly-alpha
    assert velocity_window(wav, 1240.81, 0.0, 25000.0, 0)[0] < nb
    for bad in (dict(smooth=2), dict(smooth=17), dict(max_gap=17), dict(max_gap=-1), dict(lines=()), dict(lines=(1.0,) * 5), dict(thr=0.0)):
        with pytest.raises(QFAHipError):
            check_scan_params(**{**dict(lines=(1549.06,), thr=0.9, smooth=1, max_gap=0), **bad})
    with pytest.raises(QFAHipError):
        check_indices({"X": (5.0, 1.0, 0.0, "whole")})
    with pytest.raises(QFAHipError):
        check_indices({"X": (0.0, 1.0, 0.0, "sometimes")})
    assert list(check_indices(None)) == ["BI", "AI"]


def _scan_of(troughs, value):
    import torch
    from qfa_amd.bal import BALScan
    B, S, L = troughs.shape[:3]
    z = torch.zeros((B, S, L, 2), dtype=torch.float64)
    return BALScan(torch.as_tensor(value), z, torch.zeros((B, S, L, 2, 3), dtype=torch.int32), torch.zeros((B, S, L, 2), dtype=torch.int32),
                   torch.as_tensor(troughs), (1549.06, 1396.76), {"BI": (3000.0, 25000.0, 2000.0, "after"), "AI": (0.0, 25000.0, 450.0, "whole")},
                   "AI", 0.9)


def test_to_intervals_equals_bal_intervals_and_csv_round_trip(tmp_path):
    from qfa_amd import BALScan, io
    from qfa_amd.absorbers import BAL_LINES, bal_intervals
    tr = np.full((3, 2, 2, 8, 2), np.nan)
    tr[0, 0, 0, :2] = [(1000.0, 4000.5), (9000.25, 12345.678)]
    tr[0, 0, 1, :1] = [(500.0, 2500.0)]
    tr[2, 0, 0, :1] = [(3.0 / 7.0, 20000.0 / 3.0)]
    val = np.zeros((3, 2, 2, 2))
    val[0, 0, :, 1], val[2, 0, 0, 1] = (3000.0, 1500.0), 10.0
    val[0, 0, 0, 0] = 1234.5
    scan = _scan_of(tr, val)
    assert isinstance(scan, BALScan)
    rest = scan.to_intervals(line=0, pad_kms=150.0)
    assert np.array_equal(rest[0], bal_intervals(np.array([1000.0, 9000.25]) - 150.0, np.array([4000.5, 12345.678]) + 150.0, BAL_LINES))
    assert rest[1].shape == (0, 2) and np.array_equal(rest[2], bal_intervals(3.0 / 7.0 - 150.0, 20000.0 / 3.0 + 150.0))
    assert scan.to_intervals(line=0, min_value=100.0)[2].shape == (0, 2)
    assert len(scan.to_intervals(line=None)[0]) == 3 * len(BAL_LINES)
    names = ["a.npz", "b.npz", "c.npz"]
    t = scan.to_table(names)
    assert list(t["file"]) == ["a.npz", "a.npz", "c.npz", "a.npz"] and t["bi"][0] == 1234.5 and t["ai"][3] == 1500.0
    path = io.write_bal_csv(str(tmp_path / "bal.csv"), t)
    back = io.read_bal_csv(path)
    for k in io.BAL_COLUMNS:
        assert np.array_equal(np.asarray(back[k]), np.asarray(t[k])), k
    per = io.bal_rest_intervals(["a", "b", "c"], back, pad_kms=150.0)
    both = scan.to_intervals(line=None, pad_kms=150.0)
    for i in range(3):
        assert sorted(map(tuple, per[i])) == sorted(map(tuple, both[i]))
    assert set(scan.arrays()) >= {"value", "var", "n_pix", "n_runs", "n_used", "n_troughs", "troughs", "lines", "index_names"}
    assert scan.is_bal("AI").tolist() == [[True, True], [False, False], [True, False]]


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "win{}-nh{}-S{}-B{}-smooth{}-gap{}-p{}".format(*c))
def test_seeded_inputs_leave_few_rows_contested(case):
    """the condition on the GPU tests' inputs: the reference alone contests at most 5 % of the (b, s, line) rows, no continuum is
    within the float32 chain's reach of cont_min, and r is 0.3 .. 0.6 inside the troughs and >= 0.95 outside"""
    r = K.reference(case)
    assert r["contested"].mean() <= 0.05
    px = r["px"]
    nh = case[1]
    assert np.all(np.abs(px["c"] - K.CONT_MIN) > (nh + 2) * R.U * px["cabs"])
    g = K.inputs(*case[:4], case[6])
    T = px["T"][:, :, g["p_lo"]:g["p_hi"]][px["use"][:, :, g["p_lo"]:g["p_hi"]]]
    assert np.all(((T > 0.25) & (T < 0.65)) | (T >= 0.95))


def test_config_keys_and_command_line_refusals():
    from qfa_amd import cli
    from qfa_amd import config as Cf
    keys = ("BAL", "BAL_THR", "BAL_SMOOTH", "BAL_MAX_GAP", "BAL_NITER", "BAL_MIN_AI", "BAL_PAD_KMS")
    assert all("MODEL." + k in Cf.EXTRA_KEYS for k in keys)
    c = Cf.get_config()
    assert c.MODEL.BAL is False and c.MODEL.BAL_THR == 0.9 and c.MODEL.BAL_SMOOTH == 1 and c.MODEL.BAL_MAX_GAP == 0
    assert c.MODEL.BAL_NITER == 1 and c.MODEL.BAL_MIN_AI == 0.0 and c.MODEL.BAL_PAD_KMS == 0.0 and isinstance(c.MODEL.BAL_SMOOTH, int)
    for bad in (("MODEL.BAL_SMOOTH", "2"), ("MODEL.BAL_MAX_GAP", "17"), ("MODEL.BAL_THR", "0.0"), ("MODEL.BAL_NITER", "0"),
                ("MODEL.BAL_PAD_KMS", "-1.0")):
        with pytest.raises(ValueError):
            cli.main(["--type", "predict", "--opts", "MODEL.BAL", "True", *bad])


def test_draws_per_wave_of_the_cases():
    """one judged case makes a wave walk two draws; the others one"""
    per = [K.draws_per_wave(c[3], 2, c[2]) for c in K.CASES]
    assert per[-1] == 2 and set(per[:-1]) == {1}
