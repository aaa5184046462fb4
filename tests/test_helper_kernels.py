"""The helper and optimiser kernels at edge shapes against float64 (qfa_small_kernels.h, qfa_prep_kernels.h).

Every entry point around the likelihood paths -- Woodbury, smooth, clip, the three Adam launches, finalize, the tau helpers, the
batch builders, the mean-continuum estimate, the zabs structure test -- is called through the C-ABI directly, so that every
argument can be set, at the shapes where small kernels go wrong: the last partial block (255 / 256 / 257), the block-to-tensor
dispatch of the multi-tensor launches with an empty tensor in the middle, k k threads of a 1024-thread block with a partial last
wave (k = 3, 17) or none to spare (k = 32), windows wider than the array, more spectra than one chunk.  The references are
tests/_helper_ref.py (pinned by tests/test_helper_ref_cpu.py); the bars are derived from the arithmetic and stated at each
test; the achieved figures on an MI355X are in profiles/helper_accuracy.txt (this file under `pytest -s`)."""
import ctypes as C

import numpy as np
import pytest

import _helper_ref as R
from conftest import rel_l2
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

f32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of float32
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def D(x, dev):
    """numpy array -> device tensor of the same dtype"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def P(t, offset_bytes=0):
    """device pointer (NULL for None and for an empty tensor, as torch gives it)"""
    if t is None or t.numel() == 0:
        return None
    return C.c_void_p(t.data_ptr() + offset_bytes)


def H(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """NaN in the same places, the same bits everywhere else"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(iv)[~na], b.view(iv)[~nb]))


def same_pattern(ours, ref):
    return bool(np.array_equal(np.isnan(ours), np.isnan(ref)) and np.array_equal(np.isposinf(ours), np.isposinf(ref))
                and np.array_equal(np.isneginf(ours), np.isneginf(ref)))


# ================================================================================================ Woodbury
@pytest.mark.parametrize("n,k", R.WOODBURY_SHAPES)
def test_woodbury_against_the_dense_float64_inverse(dev, n, k):
    """k_wood_core / k_wood_inv: n > 1024 wraps the log D loop, k = 3 and 17 leave a partial wave in the `t < k*k` branches,
    k = 32 uses all 1024 threads.  The kernels compute in float64 and round once; cond(C) <= 1e8 keeps the float64 part below
    1e-8 (test_helper_ref_cpu.py::test_oracle_woodbury_agrees_with_the_dense_inverse), so: inverse rel-L2 < 1e-7, log-determinant
    within 2^-24 |ref| + 1e-9 n.  The inverse-only and logdet-only calls give the bits of the combined call.
    (profiles/helper_accuracy.txt: 1.9e-8 .. 5.1e-8 and at most 0.57 of the logdet bar)"""
    import torch
    M, Dg, inv_ref, ld_ref = R.woodbury_case(n, k)
    h, st = _lib.lib(), _lib.current_stream(dev)
    Mt, Dt = D(M, dev), D(Dg, dev)
    ws = torch.zeros((k * k + 1) * 8, dtype=torch.uint8, device=dev)

    def call(want_inv, want_ld):
        inv = torch.full((n * n + 8,), 7.5, device=dev) if want_inv else None
        ld = torch.full((3,), 7.5, device=dev) if want_ld else None
        assert h.qfa_woodbury_f32(P(Mt), P(Dt), n, k, P(inv), P(ld), P(ws), ws.numel(), st) == 0
        return (H(inv) if want_inv else None), (H(ld) if want_ld else None)

    inv, ld = call(True, True)
    assert (inv[n * n:] == 7.5).all() and (ld[1:] == 7.5).all()
    inv_only, _ = call(True, False)
    _, ld_only = call(False, True)
    assert same_bits(inv_only, inv) and same_bits(ld_only, ld)
    e_inv = rel_l2(inv[:n * n].reshape(n, n), inv_ref)
    e_ld, bar_ld = abs(float(ld[0]) - ld_ref), U * abs(ld_ref) + 1e-9 * n
    print(f"\nwoodbury n={n} k={k}: inverse rel-L2 {e_inv:.2e}, logdet err {e_ld:.2e} (bar {bar_ld:.2e})")
    assert np.isfinite(inv[:n * n]).all()
    assert e_inv < 1e-7
    assert e_ld <= bar_ld


# ================================================================================================ smooth
SMOOTH_SHAPES = [(1, 1, 7), (1, 5, 0), (5, 1, 7), (15, 3, 7), (16, 1, 7), (31, 16, 15), (257, 3, 15), (300, 32, 15), (40, 7, 40),
                 (1000, 1, 0)]


def _smooth(dev, x, half):
    import torch
    n, cols = x.shape
    y = torch.full((n * cols + 8,), 7.5, device=dev)
    xt = D(x, dev)                                               # (held until the result is back: a pointer keeps nothing alive)
    assert _lib.lib().qfa_smooth_f32(P(xt), P(y), n, cols, half, _lib.current_stream(dev)) == 0
    y = H(y)
    assert (y[n * cols:] == 7.5).all()
    return y[:n * cols].reshape(n, cols)


def _smooth_bar(x, half):
    """a float32 sum of w = hi - lo terms in order and one division: |err| <= (w + 1) 2^-24 sum|x| / w per element"""
    n = x.shape[0]
    i = np.arange(n)
    w = (np.minimum(i + half + 1, n) - np.maximum(i - half, 0)).astype(np.float64)[:, None]
    return (w + 1) * U * R.edge_mean(np.abs(x.astype(np.float64)), half)        # (edge_mean |x| = sum|x| / w)


@pytest.mark.parametrize("n,cols,half", SMOOTH_SHAPES)
def test_smooth_against_the_float64_window_mean(dev, n, cols, half):
    """k_smooth on mixed-sign input against O._edge_mean in float64; half = 0 returns the input's bits; windows wider than the
    array (half >= n); one NaN row makes exactly the rows within `half` of it NaN (the avg_pool of the reference; the oracle's
    prefix sums would carry a NaN to every later row, so the pattern is stated directly and the values of the other rows are
    compared with the oracle's on the input without that row).  (profiles/helper_accuracy.txt: at most 0.17 of the bar)"""
    rng = np.random.default_rng(100 * n + cols + half)
    x = rng.standard_normal((n, cols)).astype(f32)
    y = _smooth(dev, x, half)
    ref = R.edge_mean(x.astype(np.float64), half)
    if half == 0:
        assert same_bits(y, x)
    bar = _smooth_bar(x, half)
    ratio = float(np.max(np.abs(y - ref) / bar))
    print(f"\nsmooth n={n} cols={cols} half={half}: max err / bar {ratio:.3f}")
    assert ratio <= 1.0
    r = n // 2
    xn = x.copy()
    xn[r] = np.nan
    yn = _smooth(dev, xn, half)
    near = np.abs(np.arange(n) - r) <= half
    assert np.array_equal(np.isnan(yn), np.repeat(near[:, None], cols, 1))
    x0 = x.copy()
    x0[r] = 0.0
    assert (np.abs(yn - R.edge_mean(x0.astype(np.float64), half))[~near] <= _smooth_bar(x0, half)[~near]).all()


# ================================================================================================ clip
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("lo,hi", [(1e-3, 2.0), (-5.0, 5.0)])
def test_clip_is_np_clip_bit_for_bit(dev, n, lo, hi):
    """k_clip: +-inf, NaN, -0.0, denormals, exactly lo and hi, the last partial block; NaN kept in place"""
    import torch
    rng = np.random.default_rng(n)
    lo32, hi32 = f32(lo), f32(hi)
    x = (rng.standard_normal(n) * 4).astype(f32)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1e-39, lo32, hi32, np.nextafter(lo32, f32(-9)),
                        np.nextafter(hi32, f32(9)), -999.0], dtype=f32)
    if n > 1:
        x[rng.permutation(n)[:len(special)]] = special
        x[-1] = np.nan                                           # the last element of the last, partial block
    else:
        x[0] = np.nan if lo > 0 else -0.0
    y = torch.full((n + 8,), 7.5, device=dev)
    xt = D(x, dev)
    assert _lib.lib().qfa_clip_f32(P(xt), P(y), n, float(lo32), float(hi32), _lib.current_stream(dev)) == 0
    y = H(y)
    assert (y[n:] == 7.5).all()
    ref = np.clip(x, lo32, hi32)
    assert ref.dtype == f32 and np.array_equal(np.isnan(ref), np.isnan(x))
    assert same_bits(y[:n], ref)


# ================================================================================================ Adam
PAD = 16


class AdamState:
    """p, g, m, v, p_out of some tensors in device buffers with PAD guard elements behind each"""

    def __init__(self, dev, tensors, inplace=()):
        import torch
        self.host = tensors                                      # list of (p, g, m, v) float32 arrays
        self.n = [len(t[0]) for t in tensors]
        self.buf = []
        for j, t in enumerate(tensors):
            b = [D(np.r_[a, np.full(PAD, 7.5, f32)], dev) for a in t]
            b.append(b[0] if j in inplace else torch.full((self.n[j] + PAD,), 7.5, device=dev))
            self.buf.append(b)
        self.inplace = set(inplace)

    def ptrs(self, j, with_g=True):
        p, g, m, v, q = self.buf[j]
        if self.n[j] == 0:
            return (None,) * 5                                   # an empty tensor carries NULL pointers
        return (p.data_ptr(), g.data_ptr() if with_g else None, m.data_ptr(), v.data_ptr(), q.data_ptr())

    def multi(self, bounds, with_g=True):
        t = _lib.AdamMulti()
        for j in range(len(self.n)):
            t.p[j], t.g[j], t.m[j], t.v[j], t.p_out[j] = self.ptrs(j, with_g)
            t.n[j], (t.lo[j], t.hi[j]) = self.n[j], bounds[j]
        t.count = len(self.n)
        return t

    def results(self, j):
        """(p_out, m, v) of tensor j after the launches; guards and the inputs that must stay are checked here"""
        n = self.n[j]
        p, g, m, v, q = (H(b) for b in self.buf[j])
        for a in (p, g, m, v, q):
            assert (a[n:] == 7.5).all(), "a guard element behind the tensor was written"
        assert same_bits(g[:n], self.host[j][1])
        if j not in self.inplace:
            assert same_bits(p[:n], self.host[j][0]), "the update is functional: p stays"
        return q[:n], m[:n], v[:n]


def _check_adam(ours, host, i, wd, lo, hi, label):
    """m, v and p_out of one tensor against float64 (oracle adam_update + np.clip):
      - the NaN / inf pattern is the float64 reference's;
      - p: rel-L2 < 5e-6, the project's own bar (test_g7_adam_trace);
      - every element within max(4 x |adam_f32 - float64|, 2 float32 ulp): the kernel differs from the float32 restatement only
        by fused multiply-adds (the build leaves contraction on), each of which moves an intermediate by at most one rounding.
    Returns the largest error in units of max(|adam_f32 - float64|, ulp / 2) -- the bar is 4."""
    p, g, m, v = host
    r64 = R.adam_f64(p, g, m, v, wd=wd, i=i, lo=lo, hi=hi, **HYPER)
    r32 = R.adam_f32(p, g, m, v, wd=wd, i=i, lo=lo, hi=hi, **HYPER)
    worst = 0.0
    for name, a, b64, b32 in zip(("p_out", "m", "v"), ours, r64, r32):
        assert a.dtype == f32 and same_pattern(a, b64), (label, name)
        fin = np.isfinite(b64)
        if not fin.any():
            continue
        unit = np.maximum(np.abs(b32.astype(np.float64) - b64), 0.5 * R.ulp32(b64))[fin]
        ratio = float(np.max(np.abs(a.astype(np.float64) - b64)[fin] / unit))
        assert ratio <= 4.0, (label, name, ratio)
        worst = max(worst, ratio)
    fin = np.isfinite(r64[0])
    if fin.any():
        assert rel_l2(ours[0][fin], r64[0][fin]) < 5e-6, label
    return worst


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("i", [0, 5, 1000])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_adam_clip_single_tensor(dev, n, i, wd):
    """k_adam_clip from non-zero m and v, with one NaN and one 1e20 gradient element (n = 1: one of the two), clipped to
    -1 .. 1.2.  (profiles/helper_accuracy.txt: at most 2.76 units of the bar's 4)"""
    lo, hi = -1.0, 1.2
    s = AdamState(dev, [R.adam_case(n, 7 * n + i)])
    rc = _lib.lib().qfa_adam_clip_f32(*[C.c_void_p(x) for x in s.ptrs(0)], n, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"],
                                      wd, i, lo, hi, _lib.current_stream(dev))
    assert rc == 0
    worst = _check_adam(s.results(0), s.host[0], i, wd, lo, hi, (n, i, wd))
    print(f"\nadam single n={n} i={i} wd={wd}: max err {worst:.2f} units (bar 4)")


MULTI_N = [257, 0, 1, 256, 1, 1, 300, 255]
MULTI_BOUNDS = [(-1.0, 1.2), (0.0, 1.0), (-5.0, 5.0), (1e-3, 2.0), (0.1, 5.0), (-1.0, 1.0), (1.0, 0.0), (-0.5, 0.5)]


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("i", [0, 5, 1000])
def test_adam_clip_multi_equals_the_single_tensor_call_bit_for_bit(dev, i, wd):
    """k_adam_clip_multi with eight tensors: an empty one with NULL pointers in the middle (blk0[] repeats a value), three of
    one element, tensor 6 without clip (lo > hi), tensor 0 in place.  The header promises "same arithmetic" as
    qfa_adam_clip_f32: the same bits, tensor by tensor, in m, v and p_out; and the float64 bars of the single-tensor test.
    (profiles/helper_accuracy.txt: at most 2.78 units)"""
    h, st = _lib.lib(), _lib.current_stream(dev)
    cases = [R.adam_case(n, 31 * j + i + 1) for j, n in enumerate(MULTI_N)]
    a, b = AdamState(dev, cases, inplace=(0,)), AdamState(dev, cases)
    t = a.multi(MULTI_BOUNDS)
    assert h.qfa_adam_clip_multi_f32(C.byref(t), HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, i, st) == 0
    worst = 0.0
    for j, n in enumerate(MULTI_N):
        lo, hi = MULTI_BOUNDS[j]
        assert h.qfa_adam_clip_f32(*[C.c_void_p(x) if x else None for x in b.ptrs(j)], n, HYPER["lr"], HYPER["b1"], HYPER["b2"],
                                   HYPER["eps"], wd, i, lo, hi, st) == 0
        ra, rb = a.results(j), b.results(j)
        for x, y, name in zip(ra, rb, ("p_out", "m", "v")):
            assert same_bits(x, y), (j, name)
        if n:
            worst = max(worst, _check_adam(ra, cases[j], i, wd, lo, hi, (j, i, wd)))
    print(f"\nadam multi i={i} wd={wd}: max err {worst:.2f} units (bar 4)")


# ================================================================================================ finalize
FINALIZE_SHAPES = [(1, 0, 1), (1, 1, 1), (257, 256, 3), (300, 0, 32), (260, 100, 16)]
SLOT6 = {"reference": 0.0, "exact": 9.0, "mixed": 4.0}          # slot 5 (n_spectra) is 9
GKEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")


def _accum_case(npix, nb, nh, mode):
    """a synthetic packed buffer: integer counts with zeros (0 / 0 = NaN; one zero count under a non-zero sum: inf).  sumA > 0
    and accF has the sign of -F, so that F sumA - accF does not cancel and '2 ulp' means the same fused or not."""
    rng = np.random.default_rng(1000 * npix + 10 * nb + nh)
    sl, tot = R.accum_layout(npix, nb, nh)
    cnt = rng.integers(0, 9, npix).astype(np.float64)
    if npix > 1:
        cnt[[0, npix - 1]] = 0.0
    elif nb == 0:
        cnt[0] = 0.0
    else:
        cnt[0] = 3.0
    F = (np.where(rng.random((npix, nh)) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 1.0, (npix, nh))).astype(f32)
    acc = np.zeros(tot)
    acc[sl["A"]] = rng.uniform(0.5, 3.0, npix) * cnt
    acc[sl["F"]] = (-np.sign(F) * rng.uniform(0.1, 2.0, (npix, nh)) * cnt[:, None]).ravel()
    acc[sl["Psi"]] = rng.standard_normal(npix) * cnt
    acc[sl["omega"]] = rng.standard_normal(nb) * cnt[:nb]
    if npix > 1:
        acc[sl["Psi"]][npix - 1] = 1.5                           # x / 0 = inf
    acc[sl["cnt"]] = cnt
    acc[sl["S"]] = [0.37, -1.21, 2.5, 7.0 if nb else 0.0, 1234.5, 9.0, SLOT6[mode], 0.0]
    if nb == 0:
        acc[sl["S"]][:3] = 0.0                                   # no blue side: 0 / 0
    return acc.astype(f32), F


def _finalize(dev, acc, F, npix, nb, nh, normalize):
    import torch
    out = {"F": torch.full((npix * nh + 8,), 7.5, device=dev), "Psi": torch.full((npix + 8,), 7.5, device=dev),
           "omega": torch.full((nb + 8,), 7.5, device=dev)}
    for k in ("tau0", "c0", "beta", "loss"):
        out[k] = torch.full((3,), 7.5, device=dev)
    acc_t, F_t = D(acc, dev), D(F, dev)
    rc = _lib.lib().qfa_finalize_grads_f32(P(acc_t), P(F_t), npix, nb, nh, normalize, P(out["F"]), P(out["Psi"]),
                                           P(out["omega"]), P(out["tau0"]), P(out["c0"]), P(out["beta"]), P(out["loss"]),
                                           _lib.current_stream(dev))
    assert rc == 0
    size = {"F": npix * nh, "Psi": npix, "omega": nb, "tau0": 1, "c0": 1, "beta": 1, "loss": 1}
    res = {}
    for k, t in out.items():
        a = H(t)
        assert (a[size[k]:] == 7.5).all(), k
        res[k] = a[:size[k]]
    return res


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("mode", list(SLOT6))
@pytest.mark.parametrize("npix,nb,nh", FINALIZE_SHAPES)
def test_finalize_on_synthetic_buffers(dev, npix, nb, nh, mode, normalize):
    """k_finalize without any pass kernel in front: the three modes of scalar slot 6, normalised and raw, against finalize_ref
    in float64: identical NaN / inf pattern (all NaN in mixed mode, the loss included); values within 2 float32 ulp (one
    product-minus and one division, each rounded once, possibly fused).  (profiles/helper_accuracy.txt: at most 1.19 ulp)"""
    acc, F = _accum_case(npix, nb, nh, mode)
    ours = _finalize(dev, acc, F, npix, nb, nh, normalize)
    ref = R.finalize_ref(acc, F, npix, nb, nh, normalize)
    worst = 0.0
    for k in GKEYS + ("loss",):
        r = np.asarray(ref[k], dtype=np.float64).ravel()
        assert same_pattern(ours[k], r), k
        if mode == "mixed":
            assert np.isnan(ours[k]).all(), k
        fin = np.isfinite(r)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(ours[k][fin] - r[fin]) / R.ulp32(r[fin]))))
    if mode == "reference" and normalize and npix > 1:
        assert np.isnan(ours["F"][:nh]).all() and np.isposinf(ours["Psi"][npix - 1])
    print(f"\nfinalize ({npix},{nb},{nh}) {mode} normalize={normalize}: max err {worst:.2f} ulp (bar 2)")
    assert worst <= 2.0


MODEL_BOUNDS = [(1.0, 0.0), (1e-3, 2.0), (1e-3, 2.0), (0.0, 1.0), (-5.0, 5.0), (0.1, 5.0)]       # F, Psi, omega, tau0, c0, beta


@pytest.mark.parametrize("wd,i", [(0.0, 0), (0.1, 5)])
@pytest.mark.parametrize("mode", list(SLOT6))
@pytest.mark.parametrize("npix,nb,nh", FINALIZE_SHAPES)
def test_fused_finalize_adam_equals_finalize_then_multi_bit_for_bit(dev, npix, nb, nh, mode, wd, i):
    """k_finalize_adam against qfa_finalize_grads_f32 (normalised) + qfa_adam_clip_multi_f32 on the same synthetic buffers, NaN and
    inf gradients included: the same bits in the loss and in p_out, m and v of all six tensors; N_b = 0 gives an empty omega
    with NULL pointers."""
    import torch
    h, st = _lib.lib(), _lib.current_stream(dev)
    acc, F = _accum_case(npix, nb, nh, mode)
    grads = _finalize(dev, acc, F, npix, nb, nh, 1)
    sizes = [npix * nh, npix, nb, 1, 1, 1]
    cases = []
    for j, n in enumerate(sizes):
        p, _, m, v = R.adam_case(n, 50 + j, special=False)
        if j == 0:
            p = F.ravel().copy()
        cases.append((np.abs(p) if 1 <= j <= 2 else p, grads[GKEYS[j]].copy(), m, v))
    two, one = AdamState(dev, cases), AdamState(dev, cases, inplace=(1,))
    hyper = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, i)
    assert h.qfa_adam_clip_multi_f32(C.byref(two.multi(MODEL_BOUNDS)), *hyper, st) == 0
    loss = torch.full((3,), 7.5, device=dev)
    acc_t = D(acc, dev)
    assert h.qfa_finalize_adam_clip_f32(P(acc_t), npix, nb, nh, C.byref(one.multi(MODEL_BOUNDS, with_g=False)), *hyper,
                                        P(loss), st) == 0
    loss = H(loss)
    assert (loss[1:] == 7.5).all() and same_bits(loss[:1], grads["loss"])
    for j in range(6):
        for x, y, name in zip(one.results(j), two.results(j), ("p_out", "m", "v")):
            assert same_bits(x, y), (GKEYS[j], name)


# ================================================================================================ tau helpers
def _z_values(n):
    rng = np.random.default_rng(n)
    if n == 1:
        return np.array([2.5], dtype=f32)
    z = rng.uniform(0.0, 7.0, n).astype(f32)
    z[:6] = [-1.0, 0.0, 1e-7, 6.5, 20.0, -1.5]                   # 1 + z = 0; one value below -1: NaN
    z[-1] = 3.0
    return z


@pytest.mark.parametrize("n", [0, 1, 257])
def test_tau_helpers_against_float64(dev, n):
    """k_tau (four models x series 1, 2, 30), k_tauhi, k_omega_func through the C-ABI with test_g9_tau's bars (rel-L2 2e-6,
    5e-6 for omega_func) on the non-NaN values and the float64 reference's NaN pattern; n = 0 with the NULL pointers of an
    empty tensor returns 0 and writes nothing.  (profiles/helper_accuracy.txt: at most 2.9e-7, 3.2e-8 and 6.2e-7)"""
    import torch
    h, st = _lib.lib(), _lib.current_stream(dev)
    z = _z_values(n) if n else np.zeros(0, f32)
    zt = D(z, dev)
    z64 = z.astype(np.float64)
    tau0, beta, c0 = 0.0123, 3.1, 0.27
    sc = [D(np.array([x], dtype=f32), dev) for x in (tau0, beta, c0)]
    t0, be, cc = (float(f32(x)) for x in (tau0, beta, c0))

    def run(fn, *args):
        out = torch.full((n + 8,), 7.5, device=dev)
        assert fn(P(zt), *args, P(out) if n else None, n, st) == 0
        a = H(out)
        assert (a[n:] == 7.5).all()
        return a[:n]

    def judge(ours, ref, bar, what):
        assert same_pattern(ours, ref), what
        ok = np.isfinite(ref)
        if n == 0:
            return 0.0
        assert ok.sum() >= n - 1
        e = rel_l2(ours[ok], ref[ok])
        assert e < bar, (what, e)
        return e

    worst_tau = 0.0
    with np.errstate(all="ignore"):
        for which in ("becker", "fg", "kamble", "mock"):
            for series in (1, 2, 30):
                t = _lib.tau_model(which, series)
                out = torch.full((n + 8,), 7.5, device=dev)
                assert h.qfa_tau_f32(P(zt), P(out) if n else None, n, C.byref(t), st) == 0
                a = H(out)
                assert (a[n:] == 7.5).all()
                worst_tau = max(worst_tau, judge(a[:n], R.tau_eff(z64, which, series), 2e-6, (which, series)))
        e_hi = judge(run(h.qfa_tauhi_f32, P(sc[0]), P(sc[1])), R.tau_hi(z64, t0, be), 2e-6, "tauHI")
        e_om = judge(run(h.qfa_omega_func_f32, P(sc[0]), P(sc[1]), P(sc[2])), R.omega_zdep(z64, t0, be, cc), 5e-6, "omega_func")
    print(f"\ntau helpers n={n}: rel-L2 tau {worst_tau:.2e}, tauHI {e_hi:.2e}, omega_func {e_om:.2e}")


def test_tau_helpers_return_an_empty_tensor_for_an_empty_input(dev):
    """a model without a blue side hands utils.tau a (B, 0) tensor, whose data_ptr() is NULL: the reference returns an empty
    tensor, and so do utils.tau, utils.tauHI and utils.omega_func (before qfa_tau_f32 and its two siblings tested n == 0 ahead
    of their pointers, this raised QFAHipError(QFA_E_NULL))"""
    import torch
    from qfa_amd import utils
    z = torch.empty((3, 0), device=dev)
    assert z.data_ptr() == 0
    for out in (utils.tau(z), utils.tau(z, which="fg", series=2), utils.tauHI(z, 0.0123, 3.1), utils.omega_func(z, 0.0123, 3.1, 0.27)):
        assert out.shape == (3, 0) and out.dtype == torch.float32 and out.device == z.device


# ================================================================================================ data preparation
PREP_SHAPES = [(1, 2, 1), (3, 255, 100), (5, 257, 257), (70, 300, 120)]
PREP_STARTS = [1040.0, 1000.0, 905.0]                            # one Lyman series, two, all 30 lines
MODELS = ("becker", "fg", "kamble", "mock")


def _prep_case(nrow, npix, nb, start):
    """flux ~ 1 (positive: the sums do not cancel); ~5 % of the pixels are -999 in flux and error, ~5 % have a valid flux with
    error = -999 (in the denominator of mu, not in its numerator), one pixel is valid in no spectrum"""
    from oracle import qfa_oracle as O
    rng = np.random.default_rng(int(nrow * 1000 + npix + start))
    wav = np.r_[np.linspace(start, 1215.0, nb), np.linspace(1216.5, 1600.0, npix - nb)]
    assert int(np.sum(wav < O._LYMAN_LAM[0])) == nb and int(np.sum(wav[0] < O._LYMAN_LAM)) == {1040.0: 1, 1000.0: 2, 905.0: 30}[start]
    zq = rng.uniform(2.0, 3.5, nrow)
    flux = rng.uniform(0.7, 1.3, (nrow, npix)).astype(f32)
    err = rng.uniform(0.05, 0.15, (nrow, npix)).astype(f32)
    if npix > 2:
        u = rng.random((nrow, npix))
        flux[u < 0.05] = -999.0
        err[u < 0.10] = -999.0
        flux[0, 1], err[0, 1] = 1.1, -999.0
        flux[:, npix // 2] = -999.0
        err[:, npix // 2] = -999.0
    mu = rng.uniform(0.8, 1.2, npix)
    return wav, zq, flux, err, mu


def _padded(a, stride, fill):
    out = np.full((a.shape[0], stride), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("start", PREP_STARTS)
@pytest.mark.parametrize("nrow,npix,nb", PREP_SHAPES)
def test_batch_builders_against_the_oracle_preprocessing(dev, nrow, npix, nb, start):
    """k_build_batch / k_build_resident for all four tau models, contiguous rows and rows Npix + 5 apart with NaN in the pad, idx in
    reverse order with a repeat:
      zabs, zq1    bit-equal to float32(oracle);   mask, error_out  bit-equal;
      delta        within one float32 ulp of float32(oracle): both sides round a float64 value once;
      resident     bit-equal to the gathered batch on its Npix pixels, exactly 0 / masked on the pad.
    (profiles/helper_accuracy.txt: delta came out bit-equal as well)"""
    import torch
    h, st = _lib.lib(), _lib.current_stream(dev)
    wav, zq, flux, err, mu = _prep_case(nrow, npix, nb, start)
    idx = np.r_[np.arange(nrow)[::-1], nrow // 2].astype(np.int32)
    nout = len(idx)
    wav_d, zq_d, mu_d, idx_d = D(wav, dev), D(zq, dev), D(mu, dev), D(idx, dev)
    zabs_ref = R.zabs_from_zqso(wav, zq[idx], nb).astype(f32)
    worst = 0.0
    for which in MODELS:
        delta_ref = R.delta_from_flux(wav, flux[idx].astype(np.float64), zq[idx], mu, nb, which).astype(f32)
        for stride in (0, npix + 5):
            s = stride or npix
            fl, er = (D(_padded(a, s, np.nan), dev) for a in (flux, err))

            def build(index, rows):
                delta, eout = torch.full((rows * npix + 8,), 7.5, device=dev), torch.full((rows * npix + 8,), 7.5, device=dev)
                zabs = torch.full((rows * nb + 8,), 7.5, device=dev)
                mask = torch.full((rows * npix + 8,), 9, dtype=torch.uint8, device=dev)
                assert h.qfa_build_batch_f32(P(fl), P(er), P(zq_d), P(index), P(wav_d), float(wav[0]), P(mu_d), _lib.TAU_IDS[which],
                                             rows, npix, nb, stride, P(delta), P(eout), P(zabs), P(mask), st) == 0
                outs = []
                for t, width, guard in ((delta, npix, 7.5), (eout, npix, 7.5), (zabs, nb, 7.5), (mask, npix, 9)):
                    a = H(t)
                    assert (a[rows * width:] == guard).all()
                    outs.append(a[:rows * width].reshape(rows, width))
                return outs

            delta, eout, zabs, mask = build(idx_d, nout)
            assert same_bits(zabs, zabs_ref)
            assert np.array_equal(mask, ((flux != -999.0) & (err != -999.0))[idx].astype(np.uint8))
            assert same_bits(eout, err[idx])
            assert not np.isnan(delta).any()
            ulps = np.abs(delta.astype(np.float64) - delta_ref) / R.ulp32(delta_ref)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= 1.0, (which, stride)
            # the resident form of the whole data set against the materialised batch of the same rows in storage order
            d0, e0, z0, m0 = build(None, nrow)
            rd = torch.full((nrow * s + 8,), 7.5, device=dev)
            rm = torch.full((nrow * s + 8,), 9, dtype=torch.uint8, device=dev)
            rz = torch.full((nrow + 8,), 7.5, device=dev)
            assert h.qfa_build_resident_f32(P(fl), P(er), P(zq_d), P(wav_d), float(wav[0]), P(mu_d), _lib.TAU_IDS[which], nrow, npix,
                                            nb, s, P(rd), P(rm), P(rz), st) == 0
            rd, rm, rz = H(rd), H(rm), H(rz)
            assert (rd[nrow * s:] == 7.5).all() and (rm[nrow * s:] == 9).all() and (rz[nrow:] == 7.5).all()
            rd, rm = rd[:nrow * s].reshape(nrow, s), rm[:nrow * s].reshape(nrow, s)
            assert same_bits(rd[:, :npix], d0) and np.array_equal(rm[:, :npix], m0)
            assert (rd[:, npix:] == 0.0).all() and not np.signbit(rd[:, npix:]).any() and (rm[:, npix:] == 0).all()
            assert same_bits(rz[:nrow], (1.0 + zq).astype(f32))
            assert same_bits(z0, R.zabs_from_zqso(wav, zq, nb).astype(f32))
    print(f"\nbuild ({nrow},{npix},{nb}) start={start:.0f}: delta max {worst:.2f} ulp of float32(oracle) (bar 1)")


@pytest.mark.parametrize("start", PREP_STARTS)
@pytest.mark.parametrize("nrow,npix,nb", PREP_SHAPES)
def test_mu_estimate_against_the_oracle(dev, nrow, npix, nb, start):
    """k_mu_accumulate + k_mu_finish (nrow = 70 passes the 64-spectrum chunk: two blocks add into one pixel) for all four tau
    models, both row strides and window_len in {2, 3, 16, Npix}: float64 against float64, rel 1e-12 on the non-NaN values of
    mu_raw and mu_smooth; the NaN patterns are the oracle's (the pixel no spectrum observes: mu_raw NaN there, mu_smooth NaN
    exactly within the window); the odd window's n + 1 reference values: the first n.  A valid flux under error = -999 counts
    in the denominator only (reference QFA/dataloader.py:111).  qfa_mu_sums_f64 over two shards + qfa_mu_finish_f64 equals
    the one-call form to 1e-13.  (profiles/helper_accuracy.txt: at most 6.7e-16 and 7.5e-16)"""
    import torch
    h, st = _lib.lib(), _lib.current_stream(dev)
    wav, zq, flux, err, _ = _prep_case(nrow, npix, nb, start)
    mask = (flux != -999.0) & (err != -999.0)
    wav_d, zq_d = D(wav, dev), D(zq, dev)
    windows = sorted({w for w in (2, 3, 16, npix) if 2 <= w <= npix})
    worst, worst_shard = 0.0, 0.0

    def rel(a, b, ok):
        return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))) if ok.any() else 0.0

    for which in MODELS:
        with np.errstate(all="ignore"):
            raw_ref, _ = R.mu_estimate(wav, flux.astype(np.float64), mask, zq, nb, which, window_len=2)
        if npix > 2:
            assert np.isnan(raw_ref[npix // 2]) and np.isnan(raw_ref).sum() < npix // 4
            with_err_only = (flux != -999.0).sum(0) != mask.sum(0)
            assert with_err_only[1]                              # the two masks of mu differ somewhere
        for stride in (0, npix + 5):
            s = stride or npix
            fl, er = (D(_padded(a, s, np.nan), dev) for a in (flux, err))
            for w in windows:
                scratch = torch.full((2 * npix + 2,), 7.5, dtype=torch.float64, device=dev)
                raw = torch.full((npix + 2,), 7.5, dtype=torch.float64, device=dev)
                sm = torch.full((npix + 2,), 7.5, dtype=torch.float64, device=dev)
                assert h.qfa_mu_estimate_f64(P(fl), P(er), P(zq_d), P(wav_d), float(wav[0]), _lib.TAU_IDS[which], nrow, npix, nb,
                                             stride, w, P(scratch), P(raw), P(sm), st) == 0
                raw_h, sm_h = H(raw), H(sm)
                assert (raw_h[npix:] == 7.5).all() and (sm_h[npix:] == 7.5).all() and (H(scratch)[2 * npix:] == 7.5).all()
                raw_h, sm_h = raw_h[:npix], sm_h[:npix]
                sm_ref = R.boxcar_reflect(raw_ref, w)[:npix]
                assert np.array_equal(np.isnan(raw_h), np.isnan(raw_ref)) and np.array_equal(np.isnan(sm_h), np.isnan(sm_ref))
                worst = max(worst, rel(raw_h, raw_ref, ~np.isnan(raw_ref)), rel(sm_h, sm_ref, ~np.isnan(sm_ref)))
            # two shards, then finish (the last window of the loop)
            cut = nrow // 2
            sc2 = torch.zeros(2 * npix, dtype=torch.float64, device=dev)
            raw2, sm2 = torch.empty(npix, dtype=torch.float64, device=dev), torch.empty(npix, dtype=torch.float64, device=dev)
            for lo, hi in ((0, cut), (cut, nrow)):
                if hi > lo:
                    assert h.qfa_mu_sums_f64(P(fl, 4 * lo * s), P(er, 4 * lo * s), P(zq_d, 8 * lo), P(wav_d), float(wav[0]),
                                             _lib.TAU_IDS[which], hi - lo, npix, nb, stride, P(sc2), st) == 0
            assert h.qfa_mu_finish_f64(P(sc2), npix, w, P(raw2), P(sm2), st) == 0
            raw2, sm2 = H(raw2), H(sm2)
            assert np.array_equal(np.isnan(raw2), np.isnan(raw_h)) and np.array_equal(np.isnan(sm2), np.isnan(sm_h))
            worst_shard = max(worst_shard, rel(raw2, raw_h, ~np.isnan(raw_h)), rel(sm2, sm_h, ~np.isnan(sm_h)))
    print(f"\nmu ({nrow},{npix},{nb}) start={start:.0f}: max rel err {worst:.2e} (bar 1e-12), shards vs one call {worst_shard:.2e} (bar 1e-13)")
    assert worst < 1e-12
    assert worst_shard < 1e-13


# ================================================================================================ zabs factor
@pytest.mark.parametrize("planted", [0, 1, 5])
@pytest.mark.parametrize("B,nb", [(1, 1), (1, 300), (9, 257), (20, 2049)])
def test_zabs_factor_counts_and_factors(dev, B, nb, planted):
    """k_zfactor_derive / k_zfactor_check ((20, 2049) is past 8 x 256 pixels: the x stride of the check wraps): an exact loader
    zabs has no bad element; planted elements -- the last element of the last row among them, and a NaN -- are counted exactly
    as zfactor_ref counts them (no element lies within 25 % of the threshold, so a fused a - zq1 ratio counts the same); zq1
    and pix_ratio are the reference's bits."""
    import torch
    rng = np.random.default_rng(B * 10000 + nb)
    wav = np.linspace(1040.0, 1215.0, nb)
    z = R.zabs_from_zqso(wav, rng.uniform(2.0, 3.5, B), nb).astype(f32)
    tol = 4e-7
    if planted:
        spots = []
        for pos in ((B - 1, nb - 1), (B // 2, nb // 2), (0, nb - 1), (B - 1, 0), (B // 3, (2 * nb) // 3)):
            if pos not in spots:
                spots.append(pos)
        spots = spots[:planted]
        for j, (r, c) in enumerate(spots):
            z[r, c] = (1.0 + z[r, c]) * (1.0 + (2e-6 if j % 2 == 0 else -2e-6)) - 1.0
        if planted == 5:
            z[spots[1] if len(spots) > 1 else spots[0]] = np.nan
    zq1_ref, ratio_ref, nbad_ref = R.zfactor_ref(z, tol)
    assert R.zfactor_margin(z, tol) > 0.25
    if not planted:
        assert nbad_ref == 0
    elif B > 1 and nb > 1:
        assert nbad_ref >= planted
    zq1, ratio = torch.full((B + 8,), 7.5, device=dev), torch.full((nb + 8,), 7.5, device=dev)
    nbad = torch.full((3,), 12345, dtype=torch.int32, device=dev)
    zt = D(z, dev)
    assert _lib.lib().qfa_zabs_factor_f32(P(zt), B, nb, tol, P(zq1), P(ratio), P(nbad), _lib.current_stream(dev)) == 0
    zq1, ratio, nbad = H(zq1), H(ratio), H(nbad)
    assert (zq1[B:] == 7.5).all() and (ratio[nb:] == 7.5).all() and (nbad[1:] == 12345).all()
    assert int(nbad[0]) == nbad_ref
    assert same_bits(zq1[:B], zq1_ref) and same_bits(ratio[:nb], ratio_ref)
