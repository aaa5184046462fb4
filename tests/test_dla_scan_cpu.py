"""The DLA finder without a GPU: the C-ABI's declarations, the restatement's own invariants, and the condition under which the GPU
test may compare arg-maxes with no spectrum left out -- on every committed seed the restatement finds the injected node and its
top-two gap is more than twice the bar."""
import os
import re

import numpy as np
import pytest

import _dla_ref as R
from conftest import REPO

CALLS = ("qfa_dla_profiles_f32", "qfa_template_scan_workspace_bytes", "qfa_template_scan_f32")


def test_header_and_exports():
    from qfa_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "qfa_hip.h")).read(), flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS, name


def _small(npix=70, nb=30, nh=5, B=3, seed=3):
    from qfa_amd import synthetic
    wav = np.concatenate([np.geomspace(1030.0, 1214.0, nb), np.geomspace(1217.0, 1600.0, npix - nb)])
    params, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    return wav, params, mu, R.draw(params, mu, wav, nb, B, seed, masks=False)


def test_ones_template_and_all_masked_give_zero():
    wav, params, mu, d = _small()
    V = np.ones((2, len(wav)))
    llr, nll0, _ = R.scan(params, mu, d["flux"], d["error"], d["zabs"], d["mask"], V)
    assert np.all(llr == 0.0) and np.all(np.isfinite(nll0))
    V = R.profiles(wav, 1150.0, 8000.0, 3, 20.0, 0.6, 2)
    mask = d["mask"].copy()
    mask[1] = False
    flux = d["flux"].copy()
    flux[1] = np.nan
    llr, nll0, _ = R.scan(params, mu, flux, d["error"], d["zabs"], mask, V)
    assert np.all(llr[1] == 0.0) and nll0[1] == 0.0
    assert np.all(llr[0] != 0.0)


def test_null_is_predict_ll():
    from oracle import qfa_oracle as O
    wav, params, mu, d = _small()
    _, nll0, _ = R.scan(params, mu, d["flux"], d["error"], d["zabs"], d["mask"], np.ones((1, len(wav))))
    for s in range(len(nll0)):
        ll = O.predict_single(params, mu, d["flux"][s], d["error"][s], d["zabs"][s], d["mask"][s])[0]
        assert abs(nll0[s] - ll) <= 1e-12 * abs(ll)


@pytest.mark.parametrize("seed", R.SDSS_SEEDS)
def test_injected_node_is_the_argmax_with_a_gap(shipped, seed):
    c = R.sdss_case(shipped, seed)
    assert np.all(c["logn"][c["node"] % len(c["logn"])] >= 20.7 - 1e-9)
    top = np.sort(c["llr"], axis=1)
    gap = top[:, -1] - top[:, -2]
    bar = R.BAR * np.maximum(np.abs(c["nll0"])[:, None], np.abs(c["nll"])).max(axis=1)
    print("seed", seed, "min gap / bar", float(np.min(gap / bar)), "min best llr", float(top[:, -1].min()))
    assert np.array_equal(np.argmax(c["llr"], axis=1), c["node"])
    assert np.all(gap > 2.0 * bar)
