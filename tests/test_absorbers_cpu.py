"""Absorber masking without a GPU: the float64 restatement of the rule (tests/_absorber_ref.py) against the Voigt function itself
(scipy.special.wofz), the small-P series at its switch, the host logic of qfa_amd.absorbers and the C-ABI's argument checks.

The accuracy bars are 1.5 x the figures of profiles/absorber_accuracy.txt (tools/absorber_accuracy.py; float64 on the CPU is
deterministic).  The rule is the Tepper-Garcia approximation, first order in a: with Ly-alpha alone the kept pixels are good to
float32 grade for damped systems; with Ly-beta the edge of ITS mask sits at |x| of about 10, where the approximation is off by
4e-4 of H at b = 30, and weaker systems at larger b are worse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _absorber_ref as R

# (log_nhi, b_kms, lyb) -> max |T_rule - T_Faddeeva| over the kept pixels, as measured (profiles/absorber_accuracy.txt)
MEASURED = {(20.3, 10.0, True): 7.402226e-07, (20.3, 30.0, True): 5.952960e-05, (21.0, 10.0, True): 2.912916e-08,
            (21.0, 30.0, True): 2.355714e-06, (22.0, 10.0, True): 2.545102e-10, (22.0, 30.0, True): 2.061861e-08,
            (20.3, 10.0, False): 1.244136e-09, (20.3, 30.0, False): 1.009669e-07, (21.0, 10.0, False): 4.907974e-11,
            (21.0, 30.0, False): 4.020353e-09, (22.0, 10.0, False): 4.400924e-13, (22.0, 30.0, False): 4.015555e-11}


@pytest.mark.parametrize("log_nhi,b_kms,lyb", sorted(MEASURED))
def test_transmission_against_the_faddeeva_function(log_nhi, b_kms, lyb):
    d, edge, n = R.accuracy_against_faddeeva(log_nhi, b_kms, lyb)
    bar = 1.5 * MEASURED[(log_nhi, b_kms, lyb)]
    print(f"log_nhi {log_nhi} b {b_kms} lyb {lyb}: max |dT| {d:.6e} (bar {bar:.6e}), edge approached to {edge:.3e}, {n} points")
    assert n > 50000 and 0.0 <= edge < 1e-6                  # the T = t_min edge is approached
    assert d <= bar
    if not lyb and log_nhi >= 20.3:                          # Ly-alpha alone, damped systems: float32 grade
        assert d < 2.0 ** -23


@pytest.mark.parametrize("b_kms", [10.0, 30.0])
def test_series_joins_the_main_form_and_h_at_zero(b_kms):
    bar = 1.5 * min(v for (lg, b, _), v in MEASURED.items() if b == b_kms)
    for lam0, _, gamma in R.LINES:
        a = R.damping(lam0, gamma, b_kms)
        ka = a / np.sqrt(np.pi)
        P = R.P_SERIES * (1.0 + np.linspace(-1e-3, 1e-3, 201))
        assert np.max(np.abs(R.voigt_series(ka, P) - R.voigt_main(ka, P))) <= bar
        x = np.sqrt(R.P_SERIES) * np.array([1.0 - 1e-12, 1.0, 1.0 + 1e-12])            # voigt_h itself across the switch
        h = R.voigt_h(a, x)
        assert np.all(np.isfinite(h)) and np.ptp(h) <= bar + 1e-12
        h0 = R.voigt_h(a, np.zeros(1))[0]
        assert np.isfinite(h0) and h0 == 1.0 - 2.0 * ka
        assert abs(h0 - R.voigt_faddeeva(a, np.zeros(1))[0]) < 1e-6
        # the series also follows the Voigt function through the core: first order in a
        xs = np.linspace(0.0, 0.25, 26)[:-1]
        assert np.max(np.abs(R.voigt_h(a, xs) - R.voigt_faddeeva(a, xs))) < 1e-6
    # the far wing is the main form's own value where exp(-P) has underflowed
    P = np.array([750.0 * (1 + 1e-12), 1e4, 1e9])
    ka = 1e-4
    assert np.array_equal(R.voigt_main(ka, P), (ka / P) * (1.0 + 1.5 / P))


def test_no_absorber_is_unit_transmission_and_intervals_are_half_open():
    lam = np.array([4000.0, 4001.0, 4002.0])
    assert np.array_equal(R.transmission(lam, [], []), np.ones(3))
    assert R.in_intervals(lam, [[4000.0, 4001.0], [4002.0, 4002.5]]).tolist() == [True, False, True]
    grid = np.array([1000.0, 1001.0, 1002.0, 1003.0])
    f = np.ones((1, 4), np.float32)
    ref = R.mask_ref(f, 0.5 * f, [1.0], grid, obs=[[2002.0, 2004.0]], rest_offsets=[0, 1], rest=[[1003.0, 1004.0]],
                     snr_window=(1000.0, 1003.0))
    assert (ref["flux"][0] == R.SENTINEL).tolist() == [False, True, False, True]        # 2002 in, 2004 out; 1003 in
    assert ref["n_interval_masked"][0] == 2 and ref["n_absorber_masked"][0] == 0
    assert (ref["n_valid"][0], ref["n_lead"][0], ref["n_trail"][0], ref["num_mask"][0]) == (2, 0, 1, 1)
    assert ref["snr"][0] == 2.0 and ref["n_snr"][0] == 2


def test_catalog_from_table():
    from qfa_amd.absorbers import AbsorberCatalog
    table = {"file": ["b.npz", "zz", "a", "b", "yy.npz", "zz"], "z_abs": [2.1, 9.0, 2.5, 2.3, 9.1, 9.2],
             "log_nhi": [20.3, 20.0, 21.0, 20.5, 20.0, 20.1]}
    cat = AbsorberCatalog.from_table(["a.npz", "c", "b"], table)
    assert len(cat) == 3 and cat.offsets.tolist() == [0, 1, 1, 3] and cat.offsets.dtype == np.int64
    assert cat.z_abs.tolist() == [2.5, 2.1, 2.3] and cat.log_nhi.tolist() == [21.0, 20.3, 20.5]      # the table's order inside a row
    assert cat.unmatched == ["zz", "yy"]
    assert cat.row(1).shape == (0, 2) and cat.rows(1, 3).offsets.tolist() == [0, 0, 2]
    lists = AbsorberCatalog([[], [(2.0, 20.3), (2.2, 21.0)], []])
    assert lists.offsets.tolist() == [0, 0, 2, 2] and lists.z_abs.tolist() == [2.0, 2.2]
    empty = AbsorberCatalog.from_table(["a"], {"file": [], "z_abs": [], "log_nhi": []})
    assert empty.offsets.tolist() == [0, 0] and len(empty.z_abs) == 0 and empty.unmatched == []


def test_bal_intervals():
    from qfa_amd.absorbers import BAL_LINES, C_KMS, bal_intervals
    assert BAL_LINES == (1549.06, 1396.76, 1240.81, 1215.67)
    iv = bal_intervals(3000.0, 25000.0)
    assert iv.shape == (4, 2) and iv.dtype == np.float64
    for (lo, hi), lam in zip(iv, BAL_LINES):
        assert lo == lam * (1.0 - 25000.0 / C_KMS) and hi == lam * (1.0 - 3000.0 / C_KMS) and lo < hi < lam
    two = bal_intervals([3000.0, 0.0], [25000.0, 1000.0], lines=(1549.06,))
    assert two.shape == (2, 2) and two[1, 1] == 1549.06 and np.array_equal(two[0], iv[0])
    with pytest.raises(ValueError):
        bal_intervals(5000.0, 3000.0)
    with pytest.raises(ValueError):
        bal_intervals(float("nan"), 3000.0)


def test_io_readers(tmp_path):
    from qfa_amd import io
    from qfa_amd.absorbers import AbsorberCatalog
    (tmp_path / "dla.csv").write_text("file,z_abs,log_nhi,extra\ns1.npz,2.5,20.3,x\ns0,2.1,21.0,y\ns1.npz,2.7,20.6,z\n")
    t = io.read_absorber_csv(str(tmp_path / "dla.csv"))
    cat = AbsorberCatalog.from_table(["s0", "s1"], t)
    assert cat.offsets.tolist() == [0, 1, 3] and cat.z_abs.tolist() == [2.1, 2.5, 2.7] and cat.unmatched == []
    (tmp_path / "bad.csv").write_text("file,z\ns1,2.5\n")
    with pytest.raises(ValueError):
        io.read_absorber_csv(str(tmp_path / "bad.csv"))
    (tmp_path / "sky.txt").write_text("# sky lines\n5575.0 5585.0\n3932.0, 3936.0  # Ca K\n\n")
    iv = io.read_intervals(str(tmp_path / "sky.txt"))
    assert iv.dtype == np.float64 and iv.tolist() == [[5575.0, 5585.0], [3932.0, 3936.0]]
    (tmp_path / "three.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError):
        io.read_intervals(str(tmp_path / "three.txt"))


def test_host_side_refusals_and_the_surface():
    import inspect
    import qfa_amd
    from qfa_amd import absorbers
    from qfa_amd._lib import QFAHipError
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.preprocess import Preprocessed
    assert qfa_amd.mask_absorbers is absorbers.mask_absorbers and qfa_amd.AbsorberCatalog is absorbers.AbsorberCatalog
    assert qfa_amd.bal_intervals is absorbers.bal_intervals and hasattr(Preprocessed, "mask_absorbers")
    assert inspect.signature(DeviceDataloader.from_observed).parameters["absorbers"].default is None
    sig = inspect.signature(absorbers.mask_absorbers).parameters
    for name, default in (("dla", None), ("sky", None), ("rest", None), ("t_min", 0.8), ("b_kms", 30.0), ("lyb", True),
                          ("correct", True), ("snr_window", (1270.0, 1600.0)), ("out", None), ("return_trans", False)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    grid = np.linspace(1100.0, 1300.0, 20)
    f = np.ones((2, 20), np.float32)
    with pytest.raises(QFAHipError):                         # no CPU fallback
        absorbers.mask_absorbers(f, f, [2.0, 2.1], grid, device="cpu")
    for bad in ([[(np.nan, 20.3)], []], [[(2.0, np.inf)], []], [[(-1.0, 20.3)], []]):
        with pytest.raises(QFAHipError):
            absorbers.AbsorberCatalog(bad)
    with pytest.raises(QFAHipError):
        absorbers._intervals([[4000.0, 4000.0]], "sky")      # lo >= hi
    with pytest.raises(QFAHipError):
        absorbers._intervals([[4000.0, np.nan]], "sky")
    with pytest.raises(QFAHipError):
        absorbers._rest_csr([[[1200.0, 1100.0]], []], 2)
    with pytest.raises(QFAHipError):
        absorbers._rest_csr([[]], 2)                         # one list for two spectra
    off, iv = absorbers._rest_csr([[], [[1400.0, 1500.0], [1200.0, 1210.0]]], 2)
    assert off.tolist() == [0, 0, 2] and iv.tolist() == [[1400.0, 1500.0], [1200.0, 1210.0]]
    absorbers._check_params(0.0, 30.0, (1270.0, 1600.0))     # the parameter checks of mask_absorbers
    for bad in ((1.0, 30.0, (1270.0, 1600.0)), (-0.1, 30.0, (1270.0, 1600.0)), (np.nan, 30.0, (1270.0, 1600.0)),
                (0.8, 0.0, (1270.0, 1600.0)), (0.8, np.inf, (1270.0, 1600.0)), (0.8, 30.0, (1600.0, 1270.0))):
        with pytest.raises(QFAHipError):
            absorbers._check_params(*bad)


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    from qfa_amd import _lib
    h = _lib.lib()
    assert "qfa_absorber_mask_f32" in _lib.EXPORTS and "qfa_absorber_workspace_bytes" in _lib.EXPORTS
    wsb = h.qfa_absorber_workspace_bytes
    assert wsb(1, 16384) > 0 and wsb(0, 1) > 0
    assert wsb(1, 16385) == 0 and wsb(1, 0) == 0 and wsb(-1, 10) == 0
    fake = 0x1000                                            # stands for a device pointer: every call returns before a launch

    def call(N=1, npix=10, q="good", n_obs=0, ptr=None, over=None, ws=16, **par):
        p = dict(t_min=0.8, b_kms=30.0, snr_lo=1270.0, snr_hi=1600.0, flags=_lib.ABS_LYB | _lib.ABS_CORRECT)
        p.update(par)
        qq = None if q is None else C.byref(_lib.AbsorberParams(*[p[k] for k in ("t_min", "b_kms", "snr_lo", "snr_hi", "flags")]))
        a = dict(flux=ptr, error=ptr, zqso=ptr, grid=ptr, abs_off=None, abs_z=None, abs_lg=None, obs=None, rest_off=None,
                 rest=None, fo=ptr, eo=ptr, tr=None, rf=ptr, ri=ptr, ws=ptr)
        a.update(over or {})
        return h.qfa_absorber_mask_f32(a["flux"], a["error"], a["zqso"], a["grid"], N, npix, a["abs_off"], a["abs_z"], a["abs_lg"],
                                       a["obs"], n_obs, a["rest_off"], a["rest"], qq, a["fo"], a["eo"], a["tr"], a["rf"], a["ri"],
                                       a["ws"], ws, None)
    E_NULL, E_SIZE, E_WORKSPACE, E_FLAGS = -1, -2, -3, -5
    assert call() == E_NULL and call(q=None) == E_NULL
    assert call(N=-1) == E_SIZE and call(npix=0) == E_SIZE and call(npix=16385) == E_SIZE and call(n_obs=-1) == E_SIZE
    for t in (-0.1, 1.0, 1.5, float("nan")):
        assert call(t_min=t) == E_SIZE
    assert call(t_min=0.0) == E_NULL                         # 0 is inside [0, 1): the next check answers
    for b in (0.0, -30.0, float("inf"), float("nan")):
        assert call(b_kms=b) == E_SIZE
    assert call(snr_lo=1600.0) == E_SIZE and call(snr_hi=float("nan")) == E_SIZE
    assert call(flags=4) == E_FLAGS and call(flags=0) == E_NULL
    assert call(N=0) == 0                                    # a no-op, whatever the pointers
    assert call(npix=16384) == E_NULL                        # the limit itself passes the size checks
    # with every required pointer present: the optional lists are all or nothing, then the workspace
    assert call(ptr=fake, ws=15) == E_WORKSPACE
    assert call(ptr=fake, over=dict(abs_off=fake)) == E_NULL and call(ptr=fake, over=dict(abs_off=fake, abs_z=fake)) == E_NULL
    assert call(ptr=fake, n_obs=2) == E_NULL and call(ptr=fake, over=dict(rest_off=fake)) == E_NULL
    assert call(ptr=fake, over=dict(abs_off=fake, abs_z=fake, abs_lg=fake, rest_off=fake, rest=fake, obs=fake), n_obs=2,
                ws=15) == E_WORKSPACE
    assert call(ptr=fake, over=dict(ws=None)) == E_NULL


def test_kernel_uses_no_scratch():
    from conftest import REPO
    path = os.path.join(REPO, "qfa_amd", "csrc", "build", "qfa_absorber-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "build first"
    txt = open(path).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", txt)
    assert len(sizes) == 1 and int(sizes[0]) == 0
