"""Mock spectra without a GPU: the numpy port of the draw contract (tests/_mock_ref.py), the boundary (header, exports,
config key) and the Python surface's names."""
import inspect
import os

import numpy as np
import pytest

import _mock_ref as R
import _philox_ref as P
from conftest import REPO


@pytest.mark.parametrize("seed,row,s", [(0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2), (12345, 2 ** 40, 7)])
def test_pixel_normals_are_standard(seed, row, s):
    n = 1 << 16
    e = R.pixel_normals(seed, [row], s + 1, n)[0, s].astype(np.float64)
    assert e.shape == (n,) and np.isfinite(e).all()
    assert abs(e.mean()) <= 5 / np.sqrt(n)
    assert abs(e.var() - 1) <= 5 * np.sqrt(2 / n)
    assert abs((e ** 4).mean() - 3) <= 5 * np.sqrt(96 / n)
    assert abs((e[1:] * e[:-1]).mean()) <= 5 / np.sqrt(n - 1)            # lag 1 across pixels


def test_pixel_stream_is_disjoint_from_the_latent_stream():
    rows = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40]
    pc = R.pixel_counters(rows, 5, 9243).reshape(-1, 4)
    lc = R.latent_counters(rows, 5, 32).reshape(-1, 4)
    assert (pc[:, 0] >= 2 ** 31).all() and (lc[:, 0] <= 7).all()
    as_set = lambda c: set(map(bytes, np.ascontiguousarray(c)))
    assert not (as_set(pc) & as_set(lc))
    assert len(as_set(pc)) == len(pc)                                     # and no pixel counter is used twice
    # under one seed the two streams draw different numbers for the same (r, s) and a like-numbered element
    z = P.normals(7, rows, 5, 8)
    e = R.pixel_normals(7, rows, 5, 8)
    assert not np.array_equal(z, e)


def test_port_does_not_depend_on_the_split():
    from qfa_amd import synthetic
    npix, nh, B, S = 90, 5, 7, 3
    wav, nb, _ = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=2)
    rng = np.random.default_rng(0)
    err = rng.uniform(0.01, 0.2, (B, npix)).astype(np.float32)
    zp1 = rng.uniform(3.0, 4.5, (B, 1)) * wav[None, :nb] / synthetic.LYA
    mask = rng.random((B, npix)) > 0.1
    h = P.latent(np.zeros((B, nh)), np.tile(np.eye(nh, dtype=np.float32), (B, 1, 1)), 11, 40, S).astype(np.float32)
    whole = R.spectra(p, mu, err, zp1, mask, h, 11, 40)
    for cut in (2, 5):
        a = R.spectra(p, mu, err[:cut], zp1[:cut], mask[:cut], h[:cut], 11, 40)
        b = R.spectra(p, mu, err[cut:], zp1[cut:], mask[cut:], h[cut:], 11, 40 + cut)
        for k in ("flux", "delta", "e"):
            assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), (cut, k)
    assert (whole["flux"][~np.broadcast_to(mask[:, None, :], whole["flux"].shape)] == -999.0).all()


def test_boundary_declares_the_mock_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in ("qfa_mock_workspace_bytes", "qfa_mock_spectra_f32"):
        assert name in _lib.EXPORTS and name + "(" in txt
    h = _lib.lib()
    assert h.qfa_mock_workspace_bytes(1913, 8) >= (8 + 3) * 1913 * 4
    assert h.qfa_mock_workspace_bytes(0, 8) == 0 and h.qfa_mock_workspace_bytes(100, 0) == 0
    assert h.qfa_mock_workspace_bytes(100, 33) == 0 and h.qfa_mock_workspace_bytes(1, 32) > 0
    # argument validation happens before any device work
    assert h.qfa_mock_spectra_f32(None, None, None, None, None, 1, 1, 1, 0, 1, 0, 0, None, None, None, 0, None) == -1


def test_python_surface_and_config_key():
    from qfa_amd import config as Cf
    from qfa_amd import model
    from qfa_amd.cli import build_parser
    sig = inspect.signature(model.QFA.sample_spectra)
    assert list(sig.parameters)[1:4] == ["error", "zabs", "mask"]
    for k in ("n_samples", "seed", "offset", "h", "hmean", "hcov", "zfac", "batch", "out", "return_delta", "return_latent"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(model.QFA.posterior_predictive).parameters)[1:8] == [
        "flux", "error", "zabs", "mask", "n_samples", "seed", "offset"]
    assert inspect.signature(model.QFA.predict_to_npz).parameters["n_replicates"].default == 0
    assert Cf.get_config().MODEL.N_REPLICATES == 0
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.N_REPLICATES", "4", "MODEL.SAMPLE_SEED", "42"])
    c = Cf.get_config(args)
    assert c.MODEL.N_REPLICATES == 4 and isinstance(c.MODEL.N_REPLICATES, int) and c.MODEL.SAMPLE_SEED == 42
    assert "MODEL.N_REPLICATES" in Cf.EXTRA_KEYS
