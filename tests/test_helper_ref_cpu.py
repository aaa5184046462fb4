"""CPU side of the helper-kernel tests (tests/test_helper_kernels.py).

1. The references of tests/_helper_ref.py are pinned where a fixture or an independent statement exists, so that a wrong
   reference cannot hide a wrong kernel.
2. The argument-check contract of the helper entry points: it runs host-side, before any launch, and needs no GPU
   (as tests/test_boundary_cpu.py::test_host_only_entry_points)."""
import ctypes as C

import numpy as np
import pytest

import _helper_ref as R
from conftest import golden, rel_l2

KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")


# ------------------------------------------------------------------------------------------------ 1. the references
def test_adam_f32_reproduces_the_reference_adam_trace():
    """g7_adam.npz is the reference's own float32 Adam (three epochs of two updates, i advances per epoch): adam_f32 within the
    5e-6 of test_hip_parity.py::test_g7_adam_trace at every update."""
    from oracle import qfa_oracle as O
    g = golden("g7_adam.npz")
    p = {k: g[f"init_{k}"].astype(np.float32) for k in KEYS}
    m = {k: np.zeros_like(p[k]) for k in KEYS}
    v = {k: np.zeros_like(p[k]) for k in KEYS}
    it = 0
    for epoch in range(3):
        for _ in range(2):
            for k in KEYS:
                p[k], m[k], v[k] = R.adam_f32(p[k], g[f"grad{it}_{k}"], m[k], v[k], O.step_lr(epoch, 1e-2, 0.9, 2), 0.9, 0.999,
                                              1e-8, 1e-3, epoch, 1.0, 0.0)
                assert p[k].dtype == np.float32 and p[k].shape == g[f"p{it}_{k}"].shape
                assert rel_l2(p[k], g[f"p{it}_{k}"]) < 5e-6, (it, k)
            it += 1


@pytest.mark.parametrize("i", [0, 5, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_f32_against_float64_is_a_few_ulp(i, wd):
    """adam_f32 against the oracle's float64 update on the inputs of the GPU test: this difference is the unit of the kernel's
    elementwise bar.  On these inputs (no cancellation, _helper_ref.adam_case) it is at most 8 float32 ulp on m, v and p --
    except where the reference's float32 itself leaves the real line: for g = 1e20, v / (1 - b2^(i+1)) overflows at i = 0
    and 5 (1e37 / 1e-3), sqrt gives inf and p does not move, while float64 moves it by the order of lr."""
    lr = 1e-2
    p, g, m, v = R.adam_case(513, 40 + i, special=True)
    q32, m32, v32 = R.adam_f32(p, g, m, v, lr, 0.9, 0.999, 1e-8, wd, i, 1.0, 0.0)
    q64, m64, v64 = R.adam_f64(p, g, m, v, lr, 0.9, 0.999, 1e-8, wd, i, 1.0, 0.0)
    big, nan = int(np.flatnonzero(g == np.float32(1e20))[0]), int(np.flatnonzero(np.isnan(g))[0])
    for a, b in ((q32, q64), (m32, m64), (v32, v64)):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a).sum() == 1 and np.isnan(a[nan])
        assert np.array_equal(np.isinf(a), np.isinf(b)) and not np.isinf(a).any()
    ok = np.ones(513, bool)
    ok[[big, nan]] = False
    for a, b in ((q32, q64), (m32, m64), (v32, v64)):
        assert np.max(np.abs(a[ok] - b[ok]) / R.ulp32(b[ok])) <= 8.0
    assert abs(m32[big] - m64[big]) <= 8 * R.ulp32(m64[big]) and abs(v32[big] - v64[big]) <= 8 * R.ulp32(v64[big])
    assert 0.1 * lr < abs(q64[big] - float(p[big])) < 10 * lr
    if i == 1000:
        assert abs(q32[big] - q64[big]) <= 8 * R.ulp32(q64[big])
    else:
        assert q32[big] == p[big]


def _small_batch():
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(48)
    p, mu = synthetic.mock_parameters(48, nb, 3, seed=3)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 6, seed=33)
    b["mask"][:, 5] = False                                     # a pixel no spectrum observes: 0 / 0
    return p, nb, b


def test_finalize_ref_reproduces_the_oracle_forward():
    """reference mode: a buffer packed from the oracle's per-element sums and counts (accA = 0, accF = -sum gF) gives the
    oracle's normalised gradients and loss, NaN where no spectrum observes a pixel; normalize = 0 gives the sums back."""
    from oracle import qfa_oracle as O
    p, nb, b = _small_batch()
    npix, nh = p["F"].shape
    loss, grads, sums, counts = O.forward(p, b["delta"], b["error"], b["zabs"], b["mask"], return_sums=True)
    sl, tot = R.accum_layout(npix, nb, nh)
    acc = np.zeros(tot)
    acc[sl["F"]] = -sums["F"].ravel()
    acc[sl["Psi"]], acc[sl["omega"]], acc[sl["cnt"]] = sums["Psi"], sums["omega"], counts["Psi"]
    assert np.array_equal(counts["F"], np.repeat(counts["Psi"][:, None], nh, 1)) and counts["Psi"][5] == 0
    acc[sl["S"]] = [sums["tau0"], sums["c0"], sums["beta"], counts["tau0"], loss * 6, 6, 0, 0]
    out = R.finalize_ref(acc, p["F"], npix, nb, nh, 1)
    for k in KEYS:
        assert np.array_equal(np.isnan(out[k]), np.isnan(grads[k])), k
        assert np.allclose(out[k], grads[k], rtol=1e-14, atol=0, equal_nan=True), k
    assert np.isnan(out["Psi"][5]) and np.isnan(out["F"][5]).all()
    assert abs(out["loss"] - loss) <= 1e-14 * abs(loss)
    raw = R.finalize_ref(acc, p["F"], npix, nb, nh, 0)
    for k in KEYS:
        assert np.array_equal(raw[k], sums[k]), k
    assert raw["loss"] == loss * 6


def test_finalize_ref_exact_and_mixed_modes():
    """slot 6 = slot 5: the float64 closed form of the exact-gradient mode (tests/_exact_ref.py), normalised and raw;
    slot 6 different from slot 5: NaN everywhere, the loss included."""
    import _exact_ref as X
    p, nb, b = _small_batch()
    npix, nh = p["F"].shape
    loss, _, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"])
    _, raw, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"], normalize=False)
    sl, tot = R.accum_layout(npix, nb, nh)
    acc = np.zeros(tot)
    acc[sl["F"]] = -np.asarray(raw["F"]).ravel()
    acc[sl["A"]] = 7.0                                           # not read in this mode
    acc[sl["Psi"]], acc[sl["omega"]], acc[sl["cnt"]] = raw["Psi"], raw["omega"], b["mask"].sum(0)
    acc[sl["S"]] = [raw["tau0"], raw["c0"], raw["beta"], 6, loss * 6, 6, 6, 0]
    out = R.finalize_ref(acc, p["F"], npix, nb, nh, 1)
    un = R.finalize_ref(acc, p["F"], npix, nb, nh, 0)
    for k in KEYS:
        assert np.allclose(out[k], np.asarray(raw[k]) / 6, rtol=1e-14, atol=0), k
        assert np.array_equal(un[k], np.asarray(raw[k])), k
        assert not np.isnan(out[k]).any()                        # an element no spectrum observes gets 0, not NaN
    assert abs(out["loss"] - loss) <= 1e-14 * abs(loss) and un["loss"] == loss * 6
    acc[sl["S"]][6] = 2
    for normalize in (0, 1):
        mixed = R.finalize_ref(acc, p["F"], npix, nb, nh, normalize)
        for k in KEYS + ("loss",):
            assert np.isnan(mixed[k]).all() and mixed[k].shape == out[k].shape, k


def test_zfactor_ref_on_a_loader_zabs_and_on_planted_elements():
    """the reference's loader gives zabs = (1 + z_qso) wav / 1215.67 - 1: zfactor_ref recovers the two factors (three float32
    roundings: 4e-7) with no bad element, and counts planted elements and a NaN exactly"""
    rng = np.random.default_rng(8)
    wav = np.linspace(1040.0, 1215.0, 300)
    zq = rng.uniform(2.0, 3.5, 9)
    z = R.zabs_from_zqso(wav, zq, 300).astype(np.float32)
    zq1, ratio, nbad = R.zfactor_ref(z, 4e-7)
    assert nbad == 0 and zq1.dtype == ratio.dtype == np.float32
    assert np.max(np.abs(ratio / (wav / wav[0]) - 1.0)) < 2e-7
    assert np.max(np.abs(zq1 / ((1.0 + zq) * wav[0] / 1215.67) - 1.0)) < 2e-7
    assert R.zfactor_margin(z, 4e-7) > 0.25
    z[3, 7] = (1.0 + z[3, 7]) * (1.0 + 2e-6) - 1.0
    z[8, 299] = (1.0 + z[8, 299]) * (1.0 - 2e-6) - 1.0
    z[5, 100] = np.nan
    assert R.zfactor_ref(z, 4e-7)[2] == 3 and R.zfactor_margin(z, 4e-7) > 0.25


@pytest.mark.parametrize("n,k", R.WOODBURY_SHAPES)
def test_oracle_woodbury_agrees_with_the_dense_inverse(n, k):
    """the GPU test's reference is the dense float64 inverse / slogdet; the oracle's own float64 Woodbury form must reproduce
    it to 1e-9 on every case (cond(C) <= 1e8 at D in 1e-3 .. 1e2), which is what bounds the float64 part of the kernels'
    error under the 1e-7 bar"""
    M, D, inv, logdet = R.woodbury_case(n, k)
    C_ = np.eye(k) + (M.astype(np.float64) / D.astype(np.float64)[:, None]).T @ M.astype(np.float64)
    assert np.linalg.cond(C_) <= 1e8
    assert rel_l2(R.woodbury_inverse(M.astype(np.float64), D.astype(np.float64)), inv) < 1e-9
    assert abs(R.woodbury_logdet(M.astype(np.float64), D.astype(np.float64)) - logdet) <= 1e-9 * n


def _mu_finish_index_rule(s, w):
    """k_mu_finish's index rule (qfa_prep_kernels.h) in numpy"""
    n = len(s)
    out = np.empty(n)
    for i in range(n):
        p = i + w // 2 - 1 + np.arange(w) - (w - 1)
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
        out[i] = np.sum(s[p]) / w
    return out


def test_boxcar_reflect_agrees_with_the_kernels_index_rule():
    """every n <= 39 and 2 <= w <= n: the reference's reflect-pad / convolve / trim (n values for an even window, n + 1 for an
    odd one: the first n) equals the kernel's reflected index walk, so the oracle is safe to compare k_mu_finish with"""
    rng = np.random.default_rng(2)
    for n in range(2, 40):
        s = rng.uniform(0.5, 1.5, n)
        for w in range(2, n + 1):
            ref = R.boxcar_reflect(s, w)
            assert len(ref) == n + (w % 2)
            assert np.max(np.abs(ref[:n] - _mu_finish_index_rule(s, w))) < 1e-14, (n, w)


def test_edge_mean_is_the_window_mean():
    """O._edge_mean (prefix sums) against the windowed mean written out, mixed signs, half beyond n included"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 3))
    for half in (0, 1, 7, 39, 40, 100):
        ref = np.stack([x[max(i - half, 0):min(i + half + 1, 40)].mean(0) for i in range(40)])
        assert np.max(np.abs(R.edge_mean(x, half) - ref)) < 1e-13


# ------------------------------------------------------------------------------------------------ 2. argument checks
E_NULL, E_SIZE, E_WORKSPACE = -1, -2, -3


def _host_ptr(keep, nbytes=256):
    """a non-NULL pointer for calls that must return before any launch reads it"""
    buf = (C.c_char * nbytes)()
    keep.append(buf)
    return C.c_void_p(C.addressof(buf))


def test_empty_elementwise_calls_do_nothing_whatever_the_pointers_are():
    """an empty torch tensor has a NULL data_ptr(): n = 0 returns 0 from every elementwise entry point, and a NULL pointer with
    n > 0 is still QFA_E_NULL"""
    from qfa_amd import _lib
    h = _lib.lib()
    t = _lib.tau_model("becker", 1)
    assert h.qfa_tau_f32(None, None, 0, C.byref(t), None) == 0
    assert h.qfa_tau_f32(None, None, 0, None, None) == 0
    assert h.qfa_tauhi_f32(None, None, None, None, 0, None) == 0
    assert h.qfa_omega_func_f32(None, None, None, None, None, 0, None) == 0
    assert h.qfa_clip_f32(None, None, 0, 0.0, 1.0, None) == 0
    assert h.qfa_smooth_f32(None, None, 0, 3, 7, None) == 0
    assert h.qfa_adam_clip_f32(None, None, None, None, None, 0, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0, 0.0, 1.0, None) == 0
    assert h.qfa_tau_f32(None, None, 4, C.byref(t), None) == E_NULL
    assert h.qfa_tauhi_f32(None, None, None, None, 4, None) == E_NULL
    assert h.qfa_omega_func_f32(None, None, None, None, None, 4, None) == E_NULL
    assert h.qfa_clip_f32(None, None, 4, 0.0, 1.0, None) == E_NULL
    assert h.qfa_smooth_f32(None, None, 4, 3, 7, None) == E_NULL


def test_woodbury_argument_checks():
    from qfa_amd import _lib
    h, keep = _lib.lib(), []
    M, D, inv, ld, ws = (_host_ptr(keep) for _ in range(5))
    big = 33 * 33 * 8 + 8
    assert h.qfa_woodbury_f32(M, D, 4, 33, inv, ld, ws, big, None) == E_SIZE
    assert h.qfa_woodbury_f32(M, D, 4, 0, inv, ld, ws, big, None) == E_SIZE
    assert h.qfa_woodbury_f32(M, D, 0, 4, inv, ld, ws, big, None) == E_SIZE
    assert h.qfa_woodbury_f32(M, D, 4, 4, inv, ld, ws, (4 * 4 + 1) * 8 - 1, None) == E_WORKSPACE
    assert h.qfa_woodbury_f32(M, D, 4, 4, None, None, ws, big, None) == E_NULL
    assert h.qfa_woodbury_f32(None, D, 4, 4, inv, ld, ws, big, None) == E_NULL
    assert h.qfa_woodbury_f32(M, D, 4, 4, inv, ld, None, big, None) == E_NULL


def test_mu_window_must_lie_in_2_to_npix():
    from qfa_amd import _lib
    h, keep = _lib.lib(), []
    flux, err, zq, wav, scratch, raw, sm = (_host_ptr(keep) for _ in range(7))
    for window in (-1, 0, 1, 11):
        assert h.qfa_mu_estimate_f64(flux, err, zq, wav, 1040.0, 0, 3, 10, 4, 0, window, scratch, raw, sm, None) == E_SIZE
        assert h.qfa_mu_finish_f64(scratch, 10, window, raw, sm, None) == E_SIZE
    assert h.qfa_mu_estimate_f64(flux, err, zq, wav, 1040.0, 0, 3, 10, 4, 9, 5, scratch, raw, sm, None) == E_SIZE   # stride < Npix
    assert h.qfa_mu_estimate_f64(flux, err, zq, wav, 1040.0, 0, 0, 10, 4, 0, 5, scratch, raw, sm, None) == E_SIZE   # B = 0
    assert h.qfa_mu_estimate_f64(flux, err, zq, wav, 1300.0, 0, 3, 10, 4, 0, 5, scratch, raw, sm, None) == E_SIZE   # no Lyman line
    assert h.qfa_mu_estimate_f64(flux, err, zq, wav, 1040.0, 4, 3, 10, 4, 0, 5, scratch, raw, sm, None) == -4       # tau model
    assert h.qfa_mu_finish_f64(None, 10, 5, raw, sm, None) == E_NULL


def _adam_multi(keep, ns):
    from qfa_amd import _lib
    t = _lib.AdamMulti()
    for j, n in enumerate(ns):
        t.p[j], t.g[j], t.m[j], t.v[j], t.p_out[j] = (_host_ptr(keep).value for _ in range(5))
        t.n[j], t.lo[j], t.hi[j] = n, 1.0, 0.0
    t.count = len(ns)
    return t


def test_adam_multi_and_fused_finalize_argument_checks():
    from qfa_amd import _lib
    h, keep = _lib.lib(), []
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    t = _adam_multi(keep, [4] * 8)
    for count in (9, -1):
        t.count = count
        assert h.qfa_adam_clip_multi_f32(C.byref(t), *hyper, 0, None) == E_SIZE
    t.count = 8
    assert h.qfa_adam_clip_multi_f32(C.byref(t), *hyper, -1, None) == E_SIZE
    t.g[3] = None
    assert h.qfa_adam_clip_multi_f32(C.byref(t), *hyper, 0, None) == E_NULL
    assert h.qfa_adam_clip_multi_f32(None, *hyper, 0, None) == E_NULL
    empty = _lib.AdamMulti()                                    # every tensor empty and NULL: nothing to launch
    empty.count = 8
    assert h.qfa_adam_clip_multi_f32(C.byref(empty), *hyper, 0, None) == 0
    # the fused call takes exactly F, Psi, omega, tau0, c0, beta of its shape
    npix, nb, nh = 10, 4, 3
    accum, loss = _host_ptr(keep, 4 * (npix * nh + 3 * npix + nb + 8)), _host_ptr(keep)
    good = [npix * nh, npix, nb, 1, 1, 1]
    for k, wrong in ((0, npix * nh + 1), (1, npix - 1), (2, nb + 1), (2, 0), (3, 2), (5, 0)):
        ns = list(good)
        ns[k] = wrong
        assert h.qfa_finalize_adam_clip_f32(accum, npix, nb, nh, C.byref(_adam_multi(keep, ns)), *hyper, 0, loss, None) == E_SIZE
    t6 = _adam_multi(keep, good)
    t6.count = 5
    assert h.qfa_finalize_adam_clip_f32(accum, npix, nb, nh, C.byref(t6), *hyper, 0, loss, None) == E_SIZE
    t6.count = 6
    assert h.qfa_finalize_adam_clip_f32(accum, npix, nb, 33, C.byref(t6), *hyper, 0, loss, None) == E_SIZE
    assert h.qfa_finalize_adam_clip_f32(accum, npix, nb, nh, C.byref(t6), *hyper, -1, loss, None) == E_SIZE
    assert h.qfa_finalize_adam_clip_f32(None, npix, nb, nh, C.byref(t6), *hyper, 0, loss, None) == E_NULL
    t6.m[1] = None
    assert h.qfa_finalize_adam_clip_f32(accum, npix, nb, nh, C.byref(t6), *hyper, 0, loss, None) == E_NULL
