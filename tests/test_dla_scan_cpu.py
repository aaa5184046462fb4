"""The DLA finder without a GPU: the C-ABI's declarations, the restatement's own invariants, and the condition under which the GPU
test may compare arg-maxes with no spectrum left out -- on every committed seed the restatement finds the injected node and its
top-two gap is more than twice the bar.  Also the batched form of the restatement (the one the long-table GPU tests compare with)
against its loop form, and the chunk size of the scan's batch walk, read off the library's size function: the GPU test of the
chunked walk needs more than one chunk and a ragged tail, and a change of the budget fails here first."""
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


@pytest.mark.parametrize("shape", [(70, 30, 5), (133, 64, 32)], ids=lambda s: "px%d_nb%d_nh%d" % s)
def test_batched_restatement_against_the_loop(shape):
    """two orders of the same float64 sums: llr and nll within 1e-11 max(|NLL0|, |NLL'|)"""
    npix, nb, nh = shape
    from qfa_amd import synthetic
    wav = np.concatenate([np.geomspace(1030.0, 1214.0, nb), np.geomspace(1217.0, 1600.0, npix - nb)])
    params, mu = synthetic.mock_parameters(npix, nb, nh, seed=npix + nh)
    d = R.draw(params, mu, wav, nb, 3, seed=npix, snr=(5.0, 100.0))
    V = R.profiles(wav, 1190.0, R.C_KMS * np.log(1190.0 / 1060.0) / 6, 7, 20.0, 0.6, 3).astype(np.float32)
    assert V.shape == (21, npix)
    V[0] = 1.0                                                 # an all-ones template
    V[1][V[1] < 0.5] = 0.0                                     # a template with a run of exact zeros
    assert np.any(V[2:] == 0.0) and np.all(V <= 1.0)           # (and the saturated cores of the table itself)
    flux, mask = d["flux"].copy(), d["mask"].copy()
    mask[1] = False                                            # an all-masked spectrum
    flux[1] = np.nan
    a = R.scan(params, mu, flux, d["error"], d["zabs"], mask, V)
    b = R.scan_batched(params, mu, flux, d["error"], d["zabs"], mask, V, block=8)
    scale = np.maximum(np.abs(a[1])[:, None], np.abs(a[2]))
    keep = scale > 0.0
    assert np.array_equal(keep, np.repeat(np.array([True, False, True])[:, None], 21, axis=1))
    for x, y in zip(a, b):
        assert np.all(x[1] == 0.0) and np.all(y[1] == 0.0)     # the all-masked spectrum: exact zeros in both
    e_llr, e_nll = np.abs(a[0] - b[0])[keep] / scale[keep], np.abs(a[2] - b[2])[keep] / scale[keep]
    print("batched against loop %s: max |d llr| / max|NLL| = %.3g, max |d nll| / max|NLL| = %.3g, max |d nll0| / |NLL0| = %.3g"
          % (shape, float(e_llr.max()), float(e_nll.max()), float(np.max(np.abs(a[1] - b[1])[[0, 2]] / np.abs(a[1])[[0, 2]]))))
    assert np.all(e_llr <= 1e-11) and np.all(e_nll <= 1e-11)
    assert np.all(np.abs(a[1] - b[1]) <= 1e-11 * np.abs(a[1]))
    assert np.all(np.abs(b[0][:, 0]) <= 1e-11 * np.abs(b[1]))  # the all-ones template: llr = 0 to the same rounding


def test_chunked_case_has_chunks_and_a_ragged_tail():
    """the chunk size at the GPU test's shape, from the library: below the batch, and a tail that is neither empty nor whole groups
    of four spectra (its last workgroup has idle waves)"""
    from qfa_amd import _lib
    npix, _, nh = R.CHUNK_SHAPE
    nc = R.CHUNK_GRID[0] * R.CHUNK_GRID[1]
    assert nc == 16384
    bc = R.chunk_size(_lib.lib().qfa_template_scan_workspace_bytes, npix, nh, nc)
    print("Bc =", bc, "at", R.CHUNK_SHAPE, "nc", nc, "; B =", R.CHUNK_B, "; tail", R.CHUNK_B % bc)
    assert bc < R.CHUNK_B
    assert R.CHUNK_B % bc != 0 and (R.CHUNK_B % bc) % 4 != 0
    # the shapes of every other scan test stay one chunk: their B = 17 is below this figure
    assert R.chunk_size(_lib.lib().qfa_template_scan_workspace_bytes, 1913, 8, 231, limit=4096) > 17


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
