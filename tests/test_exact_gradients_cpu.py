"""The exact gradient mode without a GPU: the float64 closed form of tests/_exact_ref.py against torch autograd on the
dense NLL, the config key and the library's flag (QFA.exact_gradients, include/qfa_hip.h QFA_F_EXACT_GRAD)."""
import numpy as np
import pytest

import _exact_ref as X
from oracle import qfa_oracle as O

KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")


def dense_autograd(params, delta, error, zabs, mask):
    """mean NLL of the dense Gaussian (Sigma = M M^T + D over the observed pixels only) and its torch float64 gradients"""
    import torch
    tp = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in params.items()}
    Nb = len(params["omega"])
    B = len(delta)
    total = torch.zeros((), dtype=torch.float64)
    for s in range(B):
        w = torch.tensor(np.asarray(mask[s], dtype=bool))
        z = torch.tensor(np.asarray(zabs[s], dtype=np.float64))
        A = torch.ones(len(params["Psi"]), dtype=torch.float64)
        A[:Nb] = torch.tensor(np.exp(-O.tau_eff(np.asarray(zabs[s], dtype=np.float64))))
        r = 1.0 - tp["c0"] - torch.exp(-tp["tau0"] * (1.0 + z) ** tp["beta"])
        om = torch.cat([tp["omega"] * r * r, torch.zeros(len(A) - Nb, dtype=torch.float64)])
        sig = torch.tensor(np.asarray(error[s], dtype=np.float64))
        D = A * A * tp["Psi"] + om + sig * sig
        M = A[:, None] * tp["F"]
        Mo, Do = M[w], D[w]
        d = torch.tensor(np.asarray(delta[s], dtype=np.float64))[w]
        S = Mo @ Mo.T + torch.diag(Do)
        n = int(w.sum())
        total = total + 0.5 * (d @ torch.linalg.solve(S, d) + n * O.LOG2PI + torch.logdet(S))
    loss = total / B
    loss.backward()
    return loss.item(), {k: tp[k].grad.numpy() for k in KEYS}


def mock_batch(npix, nh, B, seed, **kw):
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1, **kw)
    return {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}, b


@pytest.mark.parametrize("npix,nh,B,seed,kw", [
    (40, 1, 3, 11, {}),
    (60, 3, 4, 12, {}),
    (48, 8, 3, 13, {"red_only": (1,)}),
    (50, 32, 2, 14, {}),
    (64, 5, 4, 15, {"dead_range": (3, 6)}),
])
def test_closed_form_matches_autograd(npix, nh, B, seed, kw):
    p, b = mock_batch(npix, nh, B, seed, **kw)
    rng = np.random.default_rng(seed)
    mask = np.asarray(b["mask"], dtype=bool).copy()
    mask &= rng.random(mask.shape) > 0.2                 # extra masked pixels
    mask[:, npix // 3] = False                           # a pixel masked in every spectrum (blue for these grids)
    loss, g, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], mask)
    ref_loss, rg = dense_autograd(p, b["delta"], b["error"], b["zabs"], mask)
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss)
    for k in KEYS:
        a, r = np.asarray(g[k], dtype=np.float64), np.asarray(rg[k], dtype=np.float64)
        assert np.linalg.norm(a - r) <= 1e-10 * max(np.linalg.norm(r), 1e-300), (k, a, r)
    assert (g["F"][npix // 3] == 0).all() and g["Psi"][npix // 3] == 0


def test_closed_form_differs_from_the_reference_formulas():
    """the point of the mode: the reference's F / tau0 / beta / c0 are not the gradient of its loss"""
    p, b = mock_batch(80, 6, 4, 21)
    _, g, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"], normalize=False)
    ref = {k: 0.0 for k in KEYS}
    for s in range(4):
        _, gs = O.nll_and_grads_single(p, b["delta"][s], b["error"][s], b["zabs"][s], b["mask"][s])
        ref = {k: ref[k] + gs[k] for k in KEYS}
    for k in ("Psi", "omega"):
        assert np.allclose(g[k], ref[k], rtol=1e-12, atol=1e-14 * np.abs(ref[k]).max()), k
    for k in ("F", "tau0", "c0", "beta"):
        assert np.linalg.norm(np.asarray(g[k]) - ref[k]) > 1e-6 * np.linalg.norm(ref[k]), k


def test_config_key():
    from qfa_amd import config
    assert "MODEL.EXACT_GRADIENTS" in config.EXTRA_KEYS
    assert config.DEFAULTS["MODEL"]["EXACT_GRADIENTS"] is False


def test_library_exports_the_flag_and_abi_4():
    from qfa_amd import _lib
    assert _lib.F_EXACT_GRAD == 0x100
    assert _lib.ABI_VERSION == 4
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qfa_hip.h")).read()
    flag = re.search(r"#define\s+QFA_F_EXACT_GRAD\s+(0x[0-9a-fA-F]+)u?", hdr)
    abi = re.search(r"#define\s+QFA_ABI_VERSION\s+(\d+)", hdr)
    assert flag and int(flag.group(1), 16) == _lib.F_EXACT_GRAD
    assert abi and int(abi.group(1)) == 4
    if os.path.exists(_lib.LIB_PATH):
        try:
            h = _lib.lib()
        except Exception:                                # (a CPU box without the ROCm runtime)
            return
        assert h.qfa_abi_version() == 4
