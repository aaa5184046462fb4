"""CPU-side checks of the closed-form EM update of F: the float64 closed form of tests/_em_ref.py against the exact-gradient
closed form of tests/_exact_ref.py (the identity S2 f - S1 = d sum NLL / df), its monotone descent, the rows it must leave
alone, and the host-only entry points of the C-ABI."""
import numpy as np
import pytest

import _em_ref as E
import _exact_ref as X

SHAPES = [(160, 4, 64), (320, 8, 200), (256, 16, 300)]      # (Npix, Nh, B)


def batch(npix, nh, B, seed=0):
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    dead = (npix // 3, npix // 3 + 10)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1, dead_range=dead)
    p = dict(p)
    p["F"] = np.random.default_rng(seed + 2).uniform(-0.5, 0.5, size=(npix, nh))
    return p, b, dead


@pytest.mark.parametrize("npix,nh,B", SHAPES)
def test_identity_with_exact_gradient(npix, nh, B):
    p, b, _ = batch(npix, nh, B, seed=npix)
    st = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])
    _, g, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"], normalize=False)
    F = np.asarray(p["F"], dtype=np.float64)
    lhs = np.einsum("iab,ib->ia", st["S2"], F) - st["S1"]
    err = np.linalg.norm(lhs - g["F"]) / np.linalg.norm(g["F"])
    print("identity", (npix, nh, B), err)
    assert err <= 1e-12
    assert np.array_equal(st["cnt"], b["mask"].sum(axis=0))
    assert np.allclose(st["S2"], np.swapaxes(st["S2"], 1, 2), rtol=1e-12, atol=1e-12)    # (numpy's inverse: symmetric to rounding)


@pytest.mark.parametrize("npix,nh,B", SHAPES)
def test_full_batch_updates_never_raise_the_nll(npix, nh, B):
    p, b, dead = batch(npix, nh, B, seed=npix + 1)
    F0 = np.array(p["F"], dtype=np.float64)
    losses = []
    for it in range(4):
        loss, p, st, skipped = E.em_step(p, b["delta"], b["error"], b["zabs"], b["mask"])
        losses.append(loss)
        # the range masked in every spectrum: unchanged and reported
        assert skipped == int((st["cnt"] == 0).sum()) >= dead[1] - dead[0]
        assert np.array_equal(p["F"][dead[0]:dead[1]], F0[dead[0]:dead[1]])
    losses.append(E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])["nll_sum"] / B)
    print("mean NLL", (npix, nh, B), losses)
    assert all(losses[k + 1] <= losses[k] for k in range(4)), losses
    assert losses[1] < losses[0]


def test_ridge_and_damping_closed_form():
    p, b, _ = batch(160, 4, 64, seed=3)
    st = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])
    F = np.asarray(p["F"], dtype=np.float64)
    full, _ = E.em_update(F, st)
    half, _ = E.em_update(F, st, damping=0.5)
    assert np.allclose(half, 0.5 * (F + full), rtol=1e-13, atol=1e-15)
    rid, _ = E.em_update(F, st, ridge=0.7)
    i = 5
    assert np.allclose(rid[i], np.linalg.solve(st["S2"][i] + 0.7 * np.eye(4), st["S1"][i]), rtol=1e-12)


def test_blend_with_rho_one_is_replacement():
    import torch
    from qfa_amd.model import EMStats
    n = 7 * (9 + 3 + 1) + 4
    g = torch.Generator().manual_seed(0)
    a = EMStats(torch.randn(n, generator=g), 7, 3)
    b = EMStats(torch.randn(n, generator=g), 7, 3)
    a0 = a.buf.clone()
    a.blend_(b, 1.0)
    assert torch.equal(a.buf, b.buf)
    c = EMStats(a0.clone(), 7, 3).blend_(b, 0.25)
    assert torch.allclose(c.buf, 0.75 * a0 + 0.25 * b.buf, rtol=1e-6, atol=1e-7)
    assert c.S2.shape == (7, 3, 3) and c.S1.shape == (7, 3) and c.cnt.shape == (7,)
    assert c.S2.data_ptr() == c.buf.data_ptr()                       # views, not copies
    with pytest.raises(Exception):
        EMStats(torch.zeros(n + 1), 7, 3)


def test_host_only_entry_points():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_em_floats(1913, 8) == 1913 * (64 + 8 + 1) + 4
    assert h.qfa_em_floats(1913, 33) == 0 and h.qfa_em_floats(0, 8) == 0
    assert h.qfa_em_workspace_bytes(128, 1913, 8) > h.qfa_workspace_bytes(128, 1913, 8)
    assert h.qfa_em_workspace_bytes(0, 1913, 8) == 0 and h.qfa_em_workspace_bytes(4, 100, 33) == 0
    # argument validation happens before any device work
    assert h.qfa_em_stats_f32(None, None, None, 1, 1, 1, 1, None, None, None, 0, 0, None) == -1
    assert h.qfa_em_update_f_f32(None, None, 1, 1, 0.0, 1.0, None, None, None) == -1
    for name in ("qfa_em_floats", "qfa_em_workspace_bytes", "qfa_em_stats_f32", "qfa_em_update_f_f32"):
        assert name in _lib.EXPORTS


def test_config_keys_default_to_todays_run():
    from qfa_amd import config
    assert config.DEFAULTS["TRAIN"]["F_UPDATE"] == "adam"
    assert config.DEFAULTS["TRAIN"]["EM_RHO"] == 1.0 and config.DEFAULTS["TRAIN"]["EM_RIDGE"] == 0.0
    for k in ("TRAIN.F_UPDATE", "TRAIN.EM_RHO", "TRAIN.EM_RIDGE"):
        assert k in config.EXTRA_KEYS
