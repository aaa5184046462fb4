"""Posterior draws, the parts that need no GPU: the numpy port of the draw contract against Random123's known answers,
the C-ABI's exports and argument checks (which return before any device work), and the predict-mode config keys."""
import ctypes as C

import numpy as np
import pytest

import _philox_ref as P


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = P.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert tuple(int(v) for v in got) == want


def test_port_draws_are_prefixes_and_depend_on_the_row_only():
    z16 = P.normals(7, [0, 5, 2 ** 32 + 1], 9, 16)
    assert np.array_equal(P.normals(7, [0, 5, 2 ** 32 + 1], 9, 8), z16[..., :8])
    assert np.array_equal(P.normals(7, [5], 9, 16)[0], z16[1])
    assert np.array_equal(P.normals(7, [0, 5, 2 ** 32 + 1], 4, 16), z16[:, :4])
    assert not np.array_equal(P.normals(8, [0], 9, 16)[0], z16[0])
    assert not np.array_equal(P.normals(7, [2 ** 32], 9, 16)[0], P.normals(7, [0], 9, 16)[0])   # the high word counts
    assert np.isfinite(z16).all()


def test_port_cholesky_pivot_rule():
    a = np.array([[4.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 9.0]])      # singular leading block: second pivot is 0
    L = P.chol64(a)
    assert L[0, 0] == 2.0 and L[1, 0] == 1.0 and L[1, 1] == 0.0 and L[2, 1] == 0.0 and L[2, 2] == 3.0
    assert np.allclose(L @ L.T, a)
    s = np.random.default_rng(1).standard_normal((6, 6))
    s = s @ s.T
    assert np.allclose(P.chol64(s), np.linalg.cholesky(s), rtol=0, atol=1e-12)


def test_new_symbols_exported():
    from qfa_amd import _lib
    h = C.CDLL(_lib.LIB_PATH)
    for name in ("qfa_sample_latent_f32", "qfa_continua_workspace_bytes", "qfa_continua_f32"):
        assert hasattr(h, name) and name in _lib.EXPORTS
    assert _lib.lib().qfa_abi_version() == 4


def test_bad_arguments_return_before_device_work():
    """The pointers below are never dereferenced: every call returns at its argument check."""
    from qfa_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(256)                                          # a non-NULL pointer that the checks accept as such
    ws = h.qfa_continua_workspace_bytes(1913, 8)
    assert ws >= 9 * 1913 * 4
    assert h.qfa_continua_workspace_bytes(0, 8) == 0
    assert h.qfa_continua_workspace_bytes(100, 0) == 0 and h.qfa_continua_workspace_bytes(100, 33) == 0
    assert h.qfa_continua_workspace_bytes(100, 32) > 0
    # qfa_sample_latent_f32(hmean, hcov, B, Nh, S, seed, row0, h, stream)
    assert h.qfa_sample_latent_f32(None, p, 4, 8, 10, 0, 0, p, None) == -1
    assert h.qfa_sample_latent_f32(p, None, 4, 8, 10, 0, 0, p, None) == -1
    assert h.qfa_sample_latent_f32(p, p, 4, 8, 10, 0, 0, None, None) == -1
    assert h.qfa_sample_latent_f32(p, p, 4, 8, 0, 0, 0, p, None) == -2              # S < 1
    assert h.qfa_sample_latent_f32(p, p, 4, 0, 10, 0, 0, p, None) == -2             # Nh < 1
    assert h.qfa_sample_latent_f32(p, p, 4, 33, 10, 0, 0, p, None) == -2            # Nh > 32
    assert h.qfa_sample_latent_f32(p, p, -1, 8, 10, 0, 0, p, None) == -2            # B < 0
    assert h.qfa_sample_latent_f32(p, p, 4, 8, 10, 0, -1, p, None) == -2            # row0 < 0
    # qfa_continua_f32(F, mu, h, R, Npix, Nh, out, workspace, workspace_bytes, stream)
    assert h.qfa_continua_f32(None, p, p, 4, 1913, 8, p, p, ws, None) == -1
    assert h.qfa_continua_f32(p, None, p, 4, 1913, 8, p, p, ws, None) == -1
    assert h.qfa_continua_f32(p, p, None, 4, 1913, 8, p, p, ws, None) == -1
    assert h.qfa_continua_f32(p, p, p, 4, 1913, 8, None, p, ws, None) == -1
    assert h.qfa_continua_f32(p, p, p, 4, 1913, 8, p, None, ws, None) == -1
    assert h.qfa_continua_f32(p, p, p, 4, 0, 8, p, p, ws, None) == -2                # Npix < 1
    assert h.qfa_continua_f32(p, p, p, 4, 1913, 33, p, p, ws, None) == -2            # Nh > 32
    assert h.qfa_continua_f32(p, p, p, -1, 1913, 8, p, p, ws, None) == -2            # R < 0
    assert h.qfa_continua_f32(p, p, p, 4, 1913, 8, p, p, ws - 1, None) == -3         # workspace too small


def test_sampling_config_keys_merge_through_opts():
    from qfa_amd import config as Cf
    from qfa_amd.cli import build_parser
    c = Cf.get_config()
    assert c.MODEL.N_SAMPLES == 0 and c.MODEL.SAMPLE_SEED == 0
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.N_SAMPLES", "100", "MODEL.SAMPLE_SEED", "42"])
    c = Cf.get_config(args)
    assert c.MODEL.N_SAMPLES == 100 and isinstance(c.MODEL.N_SAMPLES, int)
    assert c.MODEL.SAMPLE_SEED == 42 and isinstance(c.MODEL.SAMPLE_SEED, int)
    assert {"MODEL.N_SAMPLES", "MODEL.SAMPLE_SEED"} <= set(Cf.EXTRA_KEYS)
