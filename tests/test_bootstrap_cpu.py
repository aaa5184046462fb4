"""CPU-side checks of the sightline bootstrap (include/qfa_hip.h: qfa_segment_codes_f32, qfa_bootstrap_workspace_bytes,
qfa_bootstrap_f64): the boundary and its refusals, the statistics of the contract's weights on the numpy restatement, the arithmetic
of ``BootstrapStack`` and of the per-statistic estimates on CPU tensors, the config keys.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _bootstrap_ref as ref

E_NULL, E_SIZE, E_WS, E_FLAGS = -1, -2, -3, -5


def test_header_declares_and_library_exports_the_entry_points():
    from conftest import REPO
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    h = C.CDLL(_lib.LIB_PATH)
    for name in ("qfa_segment_codes_f32", "qfa_bootstrap_workspace_bytes", "qfa_bootstrap_f64"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.EXPORTS and hasattr(h, name), name
    assert _lib.lib().qfa_abi_version() == _lib.ABI_VERSION == 4


def test_workspace_sizes_of_supported_and_unsupported_shapes():
    from qfa_amd import _lib
    wsb = _lib.lib().qfa_bootstrap_workspace_bytes
    assert wsb(4096, 1, 3, 120, 8, 1000) > 0 and wsb(0, 1, 1, 1, 1, 1) > 0 and wsb(1, 1, 1, 4096, 4096, 65536) > 0
    for bad in ((-1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 4097, 1, 1), (1, 1, 1, 1, 0, 1),
                (1, 1, 1, 1, 4097, 1), (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 65537), (1 << 30, 1, 4, 1, 1, 1), (1, 1 << 20, 1, 4095, 4096, 1)):
        assert wsb(*bad) == 0, bad


def test_bootstrap_refuses_bad_arguments_before_any_device_work():
    """every pointer is a host address no kernel may touch: a refusal that came after device work would fault, not return"""
    from qfa_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(8)                                          # non-NULL and never dereferenced

    def call(rows=one, row_type=0, codes=one, B=2, S=1, nseg=3, W=5, nz=2, R=7, seed=1, off=0, flags=0, boot=one, ws=one, nbytes=16):
        return h.qfa_bootstrap_f64(rows, row_type, codes, B, S, nseg, W, nz, R, seed, off, flags, boot, ws, nbytes, None)
    assert call(boot=None) == E_NULL and call(ws=None) == E_NULL
    assert call(rows=None) == E_NULL and call(codes=None) == E_NULL
    for bad in (dict(B=-1), dict(S=0), dict(nseg=0), dict(W=0), dict(W=4097), dict(nz=0), dict(nz=4097), dict(R=0), dict(R=65537),
                dict(off=-1), dict(row_type=3), dict(row_type=-1), dict(B=1 << 30, nseg=4)):
        assert call(**bad) == E_SIZE, bad
    assert call(flags=0x1) == E_FLAGS and call(flags=0x200) == E_FLAGS
    assert call(nbytes=15) == E_WS
    assert call(B=0, rows=None, codes=None) == 0                 # nothing to add: a no-op, whatever the pointers
    # the order of the checks: sizes before flags before the workspace before the row pointers
    assert call(W=0, flags=0x1, nbytes=0, rows=None) == E_SIZE and call(flags=0x1, nbytes=0, rows=None) == E_FLAGS
    assert call(nbytes=0, rows=None) == E_WS


def test_segment_codes_refuses_what_p1d_refuses():
    from qfa_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(8)

    def call(trans=one, ivar=one, batch="zabs", tbar=one, B=2, S=1, Nb=30, p=None, codes=one, **over):
        prm = dict(zT0=1.5, dzT=0.125, nT=17, St=1, p_lo=0, seg_len=10, nseg=3, min_used=5, z0=2.0, dz=0.5, nz=3)
        prm.update(over)
        pp = _lib.P1DParams(*[prm[k] for k in ("zT0", "dzT", "nT", "St", "p_lo", "seg_len", "nseg", "min_used", "z0", "dz", "nz")])
        bs = _lib.Batch()
        bs.zabs = 8 if batch == "zabs" else None
        bs.zq1 = 8 if batch == "half" else None
        bs.row_stride = over.get("row_stride", 0)
        return h.qfa_segment_codes_f32(trans, ivar, None if batch is None else C.byref(bs), tbar, B, S, Nb,
                                       None if p == "null" else C.byref(pp), codes, None)
    assert call(trans=None) == E_NULL and call(ivar=None) == E_NULL and call(tbar=None) == E_NULL and call(codes=None) == E_NULL
    assert call(batch=None) == E_NULL and call(p="null") == E_NULL and call(batch="none") == E_NULL and call(batch="half") == E_NULL
    for bad in (dict(B=-1), dict(S=0), dict(Nb=0), dict(seg_len=0), dict(seg_len=4097), dict(nseg=0), dict(p_lo=-1), dict(p_lo=1),
                dict(min_used=0), dict(dz=0.0), dict(dz=float("nan")), dict(z0=float("inf")), dict(nz=0), dict(nz=4097), dict(dzT=-1.0),
                dict(nT=0), dict(St=2), dict(row_stride=29)):
        assert call(**bad) == E_SIZE, bad
    assert call(B=0) == 0


def test_threshold_table_is_the_poisson_cdf():
    acc, fact = 0.0, 1.0
    for k in range(13):
        fact = fact * k if k else 1.0
        acc += math.exp(-1.0) / fact
        assert abs(int(ref.THRESHOLDS[k]) - min(acc * 2.0 ** 32, 2.0 ** 32 - 1)) <= 1.0, k   # floor, within one unit of float64 rounding


N_ROWS, N_BOOT = 4000, 64                                        # 256 000 weights of one fixed counter range


@pytest.fixture(scope="module")
def sample():
    return ref.weights(20240607, np.arange(N_ROWS), N_BOOT)


def test_weights_reproduce_the_poisson_table_within_binomial_5_sigma(sample):
    n = sample.size
    for k in range(8):
        p = math.exp(-1.0) / math.factorial(k)
        got = int((sample == k).sum())
        assert abs(got - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p)), (k, got, n * p)
    assert sample.min() == 0 and sample.max() <= 13
    # mean and variance 1: the sums of n integers, within 5 sigma (var of w = 1, var of (w - 1)^2 = 1 + 1 = 2 for Poisson(1))
    assert abs(int(sample.sum()) - n) <= 5.0 * math.sqrt(n)
    assert abs(int(((sample - 1) ** 2).sum()) - n) <= 5.0 * math.sqrt(2.0 * n)


def test_weights_depend_on_seed_row_and_replicate_alone(sample):
    seed = 20240607
    assert np.array_equal(ref.weights(seed, np.arange(N_ROWS), 5), sample[:, :5])                    # not on R
    assert np.array_equal(ref.weights(seed, np.arange(N_ROWS), 17), sample[:, :17])
    cut = np.concatenate([ref.weights(seed, np.arange(0, 1234), N_BOOT), ref.weights(seed, np.arange(1234, N_ROWS), N_BOOT)])
    assert np.array_equal(cut, sample)                                                                # not on the batch cut
    rows = np.zeros((3, 2, 2, 1))                                                                     # not on the draw s: one w per (b, r)
    rows[:, 0], rows[:, 1] = 1.0, 1.0
    boot, _, _ = ref.bootstrap(rows, np.zeros((3, 2, 2), np.int32), 1, 4, seed, 10)
    assert np.array_equal(boot[0], boot[1])
    other = ref.weights(seed + 1, np.arange(N_ROWS), N_BOOT)
    assert (other != sample).mean() > 0.5                                                             # another seed
    hi = ref.weights(seed, np.arange(N_ROWS) + (1 << 32), N_BOOT)                                     # same low 32 bits of the row
    assert (hi != sample).mean() > 0.5
    hi_seed = ref.weights(seed + (1 << 32), np.arange(N_ROWS), N_BOOT)                                # same low 32 bits of the seed
    assert (hi_seed != sample).mean() > 0.5


def test_bootstrap_counter_is_disjoint_from_the_other_streams():
    import _philox_ref
    key = np.array([7, 0], np.uint32)
    boot = ref.words(7, [3], 4)[0]
    for first in (0, 0x80000000):                                # the latent stream's and the mock stream's first word at q = 0
        other = _philox_ref.philox4x32_10(np.array([first, 0, 3, 0], np.uint32), key)
        assert not np.array_equal(other, boot)
    same = _philox_ref.philox4x32_10(np.array([0x40000000, 0, 3, 0], np.uint32), key)
    assert np.array_equal(same, boot)


def test_bootstrap_stack_arithmetic_on_cpu_tensors():
    import torch
    import qfa_amd
    from qfa_amd.stacks import BootstrapStack
    assert qfa_amd.BootstrapStack is BootstrapStack
    rng = np.random.default_rng(5)
    S, R, nz, W = 2, 6, 3, 4
    buf = rng.uniform(1.0, 2.0, (S, R, nz, 1 + W))
    st = BootstrapStack(torch.tensor(buf), seed=11, bins=(2.0, 0.5, nz))
    assert (st.S, st.R, st.nz, st.W, st.seed) == (S, R, nz, W, 11)
    mean = buf[..., 1:] / buf[..., :1]
    assert np.array_equal(st.n.numpy(), buf[..., 0]) and np.allclose(st.mean_rows.numpy(), mean, rtol=1e-15)
    for s in range(S):
        for kz in range(nz):
            want = np.cov(mean[s, :, kz].T, ddof=1)
            assert np.allclose(st.cov()[s, kz].numpy(), want, rtol=1e-12, atol=1e-15)
        full = np.cov(mean[s].reshape(R, nz * W).T, ddof=1)
        assert np.allclose(st.cov(across_z=True)[s].numpy(), full, rtol=1e-12, atol=1e-15)
    assert np.allclose(st.err().numpy() ** 2, np.diagonal(st.cov().numpy(), axis1=2, axis2=3), rtol=1e-12)
    assert np.allclose(np.diagonal(st.corr().numpy(), axis1=2, axis2=3), 1.0, rtol=1e-12)
    sq = st.estimates(lambda sums: (sums[..., 1:3] / sums[..., :1]) ** 2)
    assert tuple(sq.shape) == (S, R, nz, 2) and tuple(st.cov(fn=lambda sums: sums[..., 1:3]).shape) == (S, nz, 2, 2)
    assert st.draws(1, 2).buf.data_ptr() == st.buf[1:].data_ptr() and st.draws(1, 2).S == 1
    arr = st.arrays()
    assert {"estimates", "cov", "n_boot", "seed"} <= set(arr) and arr["n_boot"] == R and arr["seed"] == 11
    assert arr["estimates"].shape == (S, R, nz, W) and arr["cov"].shape == (S, nz, W, W) and len(arr["z_edges"]) == nz + 1
    from qfa_amd._lib import QFAHipError
    with pytest.raises(QFAHipError):
        BootstrapStack(torch.zeros((S, R, nz, 1), dtype=torch.float64))
    with pytest.raises(QFAHipError):
        BootstrapStack(torch.zeros((S, R, nz, 3), dtype=torch.float32))
    with pytest.raises(QFAHipError):
        BootstrapStack(torch.zeros((S, R, nz, 3), dtype=torch.float64), bins=(0.0, 1.0, nz + 1))
    assert torch.isnan(BootstrapStack(torch.ones((1, 1, 1, 2), dtype=torch.float64)).cov()).all()


def test_estimates_agree_with_the_stack_classes_at_unit_weights():
    """with every weight 1 the bootstrap sums are the stacks' own sums: each ``bootstrap_estimate`` must give its class's formula"""
    import torch
    from qfa_amd.stacks import P1DBandStack, P1DStack, PDFStack, VarianceStack, XiStack
    rng = np.random.default_rng(8)
    S, nz, n = 2, 3, 40.0
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    L, M, dv = 12, 6, 69.0
    P, N = rng.uniform(1, 2, (S, nz, M)) * n, rng.uniform(0.1, 0.2, (S, nz, 1)) * n
    st = P1DStack(t64(np.concatenate([np.full((S, nz, 1), n), N, P, P * P], -1)), 2.0, 0.5, nz, L, dv)
    got = P1DStack.bootstrap_estimate(t64(np.concatenate([np.full((S, nz, 1), n), N, P], -1)), dv=dv)
    assert torch.allclose(got, st.power(), rtol=1e-13, atol=0)
    edges = P1DBandStack.linear_k_edges(L, dv, 3)
    Q = rng.uniform(1, 2, (S, nz, 3)) * n
    sb = P1DBandStack(t64(np.concatenate([np.full((S, nz, 1), n), Q, np.zeros((S, nz, 9))], -1)), 2.0, 0.5, nz, L, dv, edges)
    assert torch.equal(P1DBandStack.bootstrap_estimate(t64(np.concatenate([np.full((S, nz, 1), n), Q], -1))), sb.mean)
    nlag = 4
    N0, Wl, Al = rng.uniform(0.1, 0.2, (S, nz, 1)), rng.uniform(5, 9, (S, nz, nlag)), rng.uniform(-1, 1, (S, nz, nlag))
    Wl[0, 0, 2] = 0.0
    sx = XiStack(t64(np.concatenate([np.full((S, nz, 1), n), N0, Wl, Al, np.zeros((S, nz, 3 * nlag))], -1)), 2.0, 0.5, nz, L, nlag, dv)
    sums = t64(np.concatenate([np.full((S, nz, 1), n), N0, Wl, Al], -1))
    for sub in (True, False):
        assert torch.equal(torch.nan_to_num(XiStack.bootstrap_estimate(sums, nlag, subtract_noise=sub), nan=-7.0),
                           torch.nan_to_num(sx.xi(subtract_noise=sub), nan=-7.0))
    nt = 5
    H = rng.integers(0, 30, (S, nz, nt)).astype(np.float64)
    H[1, 1] = 0.0
    sp = PDFStack(t64(np.concatenate([np.full((S, nz, 1), n), H.sum(-1, keepdims=True) + 2, H, np.zeros((S, nz, nt * nt))], -1)),
                  2.0, 0.5, nz, L, 0.0, 0.2, nt)
    got = PDFStack.bootstrap_estimate(t64(np.concatenate([np.full((S, nz, 1), n), H], -1)), dt=sp.dt)
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(sp.pdf(), nan=-7.0))
    nv = 4
    mom = rng.uniform(1, 2, (S, nz, 5 * nv)) * n
    sv = VarianceStack(t64(np.concatenate([np.full((S, nz, 1), n), np.full((S, nz, 1), 12 * n), mom], -1)), 2.0, 0.5, nz, L, -8, 2, 1)
    got = VarianceStack.bootstrap_estimate(t64(np.concatenate([np.full((S, nz, 1), n), mom], -1)), nv)
    assert torch.equal(got, sv.var_delta)


def test_config_keys_and_cpu_refusals():
    from qfa_amd import config as Cf
    from qfa_amd._lib import QFAHipError
    from qfa_amd.statistics import _BOOT_STATS, ForestStatistics
    assert "MODEL.BOOT_N" in Cf.EXTRA_KEYS and "MODEL.BOOT_SEED" in Cf.EXTRA_KEYS
    c = Cf.get_config()
    assert c.MODEL.BOOT_N == 0 and c.MODEL.BOOT_SEED == 0 and isinstance(c.MODEL.BOOT_N, int)
    assert sorted(_BOOT_STATS) == ["bands", "p1d", "pdf", "variance", "xi"]
    with pytest.raises(QFAHipError):
        ForestStatistics().bootstrap(None, "forest", 2.0, 3.0, 2, 10)
    with pytest.raises(QFAHipError):
        ForestStatistics().bootstrap(None, "p1d", 2.0, 3.0, 2, 0)
    from qfa_amd import cli
    with pytest.raises(ValueError):
        cli.main(["--type", "predict", "--opts", "MODEL.BOOT_N", "-1"])


def test_kernels_use_no_scratch():
    from conftest import REPO
    path = os.path.join(REPO, "qfa_amd", "csrc", "build", "qfa_bootstrap-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "build first"
    txt = open(path).read()
    names = re.findall(r"\.name:\s*(\S*k_bootstrap\S*|\S*k_segment_codes\S*)\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)", txt)
    assert len(names) >= 3 and all(int(size) == 0 for _, size in names), names
