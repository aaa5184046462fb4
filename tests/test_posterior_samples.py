"""Posterior draws on the MI355X (QFA.sample_latent / continua_from_latent / sample_continua, qfa_sample_latent_f32 /
qfa_continua_f32) against the numpy port of the draw contract (tests/_philox_ref.py) and float64 arithmetic."""

import numpy as np
import pytest

import _philox_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    if x.dtype == bool:
        return torch.tensor(x, dtype=torch.bool, device=dev)
    return torch.tensor(x, dtype=torch.float32, device=dev)


def plain_model(dev, npix, nh, seed=0):
    """a model with random F, mu and no blue side: for the draws and the writer only F and mu matter"""
    from qfa_amd import QFA
    rng = np.random.default_rng(seed)
    p = {"F": rng.uniform(-0.5, 0.5, (npix, nh)).astype(np.float32), "Psi": np.ones(npix, np.float32),
         "omega": np.ones(0, np.float32), "tau0": np.float32(0.02), "c0": np.float32(0.3), "beta": np.float32(2.0)}
    m = QFA(0, npix, nh, dev, model_params=p)
    m.mu = T(rng.uniform(0.5, 2.0, npix).astype(np.float32), dev)
    return m


def synthetic_posterior(dev, npix, nh, B, seed, mask_rows=(), snr=None):
    from qfa_amd import QFA, synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=100 + seed)
    for r in mask_rows:
        b["mask"][r, :] = False
    if snr is not None:
        b["error"] = (np.abs(b["flux"]) * snr + 1e-12).astype(np.float32)
    m = QFA(nb, nr, nh, dev, model_params=p)
    m.mu = T(mu, dev)
    inputs = (T(b["flux"], dev), T(b["error"], dev), T(b["zabs"], dev), T(b["mask"], dev))
    return m, inputs


def identity_posterior(dev, B, nh):
    import torch
    return (torch.zeros((B, nh), dtype=torch.float32, device=dev),
            torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1).contiguous())


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ------------------------------------------------------------------------------------------------------------ draw bits
@pytest.mark.parametrize("nh", [3, 8, 13, 32])
def test_z_bits_match_the_port(dev, nh):
    m = plain_model(dev, 16, nh)
    hm, hc = identity_posterior(dev, 5, nh)
    for seed in (0, 1, 2 ** 40 + 5, 2 ** 64 - 1):
        for row0 in (0, 2 ** 32 - 3, 2 ** 33 - 1):
            h = m.sample_latent(hm, hc, 37, seed=seed, offset=row0).cpu().numpy()
            z = P.normals(seed, row0 + np.arange(5), 37, nh)
            assert h.shape == (5, 37, nh)
            assert ulps(h, z).max() <= 1.0, (seed, row0)


@pytest.mark.parametrize("nh", [4, 8, 16, 32])
def test_latent_matches_cholesky_of_predict_posterior(dev, nh):
    m, inputs = synthetic_posterior(dev, 600, nh, 6, seed=20 + nh)
    _, hm, hc, _, _ = m.predict(*inputs)
    S = 50
    h = m.sample_latent(hm, hc, S, seed=11, offset=1000).cpu().numpy().astype(np.float64)
    hm64, hc64 = hm.cpu().numpy().astype(np.float64), hc.cpu().numpy()
    z = P.normals(11, 1000 + np.arange(6), S, nh).astype(np.float64)
    for b in range(6):
        want = z[b] @ P.chol64(hc64[b]).T
        got = h[b] - hm64[b]
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 2e-6, b


# ------------------------------------------------------------------------------------------------------------ writer
@pytest.mark.parametrize("npix", [1, 1913, 4000, 9243])
@pytest.mark.parametrize("nh", [1, 7, 8, 16, 17, 32])
def test_writer_matches_float64(dev, npix, nh):
    import torch
    m = plain_model(dev, npix, nh, seed=npix + nh)
    R = 37
    g = torch.Generator(device=dev).manual_seed(npix * 33 + nh)
    h = torch.randn((R, nh), generator=g, device=dev)
    F, mu = m.F.cpu().numpy().astype(np.float64), m.mu.cpu().numpy().astype(np.float64)
    h64 = h.cpu().numpy().astype(np.float64)
    want = mu + h64 @ F.T
    # the predict writer's bar, relative to the row's largest value; a one-pixel row has no such scale (its single value may be
    # a cancellation of the N_h terms), so there the bar is relative to the terms |mu| + sum_j |F h|
    scale = np.max(np.abs(want), axis=1) if npix > 1 else np.max(np.abs(mu) + np.abs(h64) @ np.abs(F).T, axis=1)
    for off in (4, 8, 64):
        buf = torch.full((off // 4 + R * npix + 16,), -7.0, dtype=torch.float32, device=dev)
        out = buf[off // 4: off // 4 + R * npix].view(R, npix)
        m.continua_from_latent(h, out=out)
        got = out.cpu().numpy().astype(np.float64)
        err = np.max(np.abs(got - want), axis=1)
        assert (err <= 2e-6 * scale).all(), (off, err.max())
        rest = buf.cpu().numpy()
        assert (rest[:off // 4] == -7.0).all() and (rest[off // 4 + R * npix:] == -7.0).all(), off
    # leading batch dimensions are kept
    h3 = h[:36].reshape(4, 9, nh)
    assert tuple(m.continua_from_latent(h3).shape) == (4, 9, npix)


# ------------------------------------------------------------------------------------------------------------ statistics
def test_statistics_of_the_draws(dev):
    import torch
    nh, S, B = 8, 65536, 3
    m, inputs = synthetic_posterior(dev, 500, nh, B, seed=5)
    _, hm, hc, _, unc = m.predict(*inputs)
    cont, h = m.sample_continua(n_samples=S, seed=3, hmean=hm, hcov=hc, return_latent=True)
    h64 = h.double()
    hm64, hc64 = hm.double(), hc.double()
    mean = h64.mean(1)
    sd_mean = torch.sqrt(torch.diagonal(hc64, dim1=1, dim2=2) / S)
    assert (torch.abs(mean - hm64) <= 5 * sd_mean).all()
    d = h64 - mean[:, None, :]
    cov = torch.einsum("bsi,bsj->bij", d, d) / (S - 1)
    dg = torch.diagonal(hc64, dim1=1, dim2=2)
    sd_cov = torch.sqrt((dg[:, :, None] * dg[:, None, :] + hc64 ** 2) / S)
    assert (torch.abs(cov - hc64) <= 5 * sd_cov).all()
    sd = cont.double().std(1)
    assert (torch.abs(sd - unc.double()) <= 0.02 * unc.double()).all()
    # whiteness of z: draws of the prior over rows, samples and components
    zh, zc = identity_posterior(dev, 8, 16)
    mz = plain_model(dev, 8, 16)
    z = mz.sample_latent(zh, zc, 8192, seed=9, offset=2 ** 32 - 4).double()
    n = z.numel()
    assert abs(z.mean().item()) <= 5 / np.sqrt(n)
    assert abs(z.var().item() - 1) <= 5 * np.sqrt(2 / n)
    assert abs((z ** 4).mean().item() - 3) <= 5 * np.sqrt(96 / n)
    for a, b in ((z[..., 1:], z[..., :-1]), (z[:, 1:], z[:, :-1]), (z[1:], z[:-1])):    # lag 1 across j, s and r
        assert abs((a * b).mean().item()) <= 5 / np.sqrt(a.numel())


# ------------------------------------------------------------------------------------------------------------ contract
def test_contract_bit_for_bit(dev, tmp_path):
    import torch
    nh, B, S = 8, 7, 20
    m, inputs = synthetic_posterior(dev, 400, nh, B, seed=7)
    _, hm, hc, _, _ = m.predict(*inputs)
    a = m.sample_continua(n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc)
    assert torch.equal(a, m.sample_continua(n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc))
    assert not torch.equal(a, m.sample_continua(n_samples=S, seed=6, offset=10, hmean=hm, hcov=hc))
    # offset slices equal the whole call
    h = m.sample_latent(hm, hc, S, seed=5, offset=10)
    hs = m.sample_latent(hm[2:5].contiguous(), hc[2:5].contiguous(), S, seed=5, offset=12)
    assert torch.equal(hs, h[2:5])
    assert torch.equal(m.sample_latent(hm, hc, S + 300, seed=5, offset=10)[:, :S], h)   # S does not change the draws
    # two-step path, and from the flux
    assert torch.equal(a, m.continua_from_latent(h))
    c2, h2 = m.sample_continua(*inputs, n_samples=S, seed=5, offset=10, return_latent=True)
    assert torch.equal(c2, a) and torch.equal(h2, h)
    # the Nh prefix property: the leading 8 x 8 block of a 16 x 16 posterior draws what the 8 x 8 one draws
    rng = np.random.default_rng(3)
    G = rng.standard_normal((B, 16, 16))
    cov16 = (G @ G.transpose(0, 2, 1) / 16).astype(np.float32)
    mean16 = rng.standard_normal((B, 16)).astype(np.float32)
    m16, m8 = plain_model(dev, 10, 16), plain_model(dev, 10, 8)
    h16 = m16.sample_latent(T(mean16, dev), T(cov16, dev), S, seed=77, offset=3)
    h8 = m8.sample_latent(T(mean16[:, :8].copy(), dev), T(cov16[:, :8, :8].copy(), dev), S, seed=77, offset=3)
    assert torch.equal(h16[..., :8], h8)
    # graph capture + replay equals eager
    out = torch.empty((B, S, m.Npix), dtype=torch.float32, device=dev)
    m.sample_continua(n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc, out=out)       # warm-up: workspace allocated
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.sample_continua(n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)


class _ListLoader(object):
    """the reference's per-spectrum dataloader contract: loader[i] = (flux, error, zabs, mask, path)"""

    def __init__(self, inputs):
        self.inputs = inputs

    def __len__(self):
        return self.inputs[0].shape[0]

    def __getitem__(self, i):
        return tuple(x[i] for x in self.inputs) + (f"spec{i:03d}",)


def test_predict_to_npz_samples_do_not_depend_on_batch_size(dev, tmp_path):
    m, inputs = synthetic_posterior(dev, 300, 8, 10, seed=8)
    loader = _ListLoader(inputs)
    w3 = m.predict_to_npz(loader, str(tmp_path / "b3"), batch_size=3, n_samples=6, seed=21)
    w4 = m.predict_to_npz(loader, str(tmp_path / "b4"), batch_size=4096, n_samples=6, seed=21)
    w0 = m.predict_to_npz(loader, str(tmp_path / "b0"), batch_size=4096)
    assert w3 == w4 == w0 and len(w3) == 10
    _, hm, hc, _, _ = m.predict(*inputs)
    whole = m.sample_continua(n_samples=6, seed=21, offset=0, hmean=hm, hcov=hc).cpu().numpy()
    for i, name in enumerate(w3):
        a, b, c = (np.load(str(tmp_path / d / name)) for d in ("b3", "b4", "b0"))
        assert a["cont_samples"].shape == (6, 300)
        assert np.array_equal(a["cont_samples"], b["cont_samples"])
        assert np.array_equal(a["cont_samples"], whole[i])
        assert sorted(c.files) == ["cont", "hcov", "hmean", "ll", "uncertainty"]
        for k in c.files:
            assert np.array_equal(a[k], c[k]), k


# ------------------------------------------------------------------------------------------------------------ edges
def test_fully_masked_spectrum_samples_the_prior(dev):
    m, inputs = synthetic_posterior(dev, 300, 8, 3, seed=9, mask_rows=(1,))
    _, hm, hc, _, _ = m.predict(*inputs)
    assert np.allclose(hm[1].cpu().numpy(), 0, atol=1e-6)
    assert np.allclose(hc[1].cpu().numpy(), np.eye(8), atol=1e-6)
    h = m.sample_latent(hm, hc, 40, seed=4, offset=77).cpu().numpy()
    z = P.normals(4, [78], 40, 8)[0]
    assert np.max(np.abs(h[1] - z)) <= 1e-5


def test_high_snr_spectrum_draws_are_finite_and_reproduce_hcov(dev):
    import torch
    nh = 8
    m, inputs = synthetic_posterior(dev, 500, nh, 3, seed=10, snr=1e-4)
    _, hm, hc, _, _ = m.predict(*inputs)
    hc_np = hc.cpu().numpy()
    # hmean = 0: the draws are C z without the rounding of a large mean, so that C can be read back from them
    S = 64
    h = m.sample_latent(torch.zeros_like(hm), hc, S, seed=2, offset=0).cpu().numpy().astype(np.float64)
    assert np.isfinite(h).all()
    z = P.normals(2, np.arange(3), S, nh).astype(np.float64)
    for b in range(3):
        Cg = np.linalg.lstsq(z[b], h[b], rcond=None)[0].T          # h = z C^T
        Cp = P.chol64(hc_np[b])
        scale = np.max(np.abs(hc_np[b]))
        assert np.max(np.abs(Cp @ Cp.T - np.tril(hc_np[b]) - np.tril(hc_np[b], -1).T)) <= 1e-6 * scale
        assert np.max(np.abs(Cg @ Cg.T - Cp @ Cp.T)) <= 1e-6 * scale, b
    c = m.sample_continua(n_samples=4, seed=2, hmean=hm, hcov=hc)
    assert torch.isfinite(c).all()


def test_nan_posterior_poisons_only_its_own_rows(dev):
    import torch
    m, inputs = synthetic_posterior(dev, 300, 8, 4, seed=12)
    _, hm, hc, _, _ = m.predict(*inputs)
    ref_h = m.sample_latent(hm, hc, 9, seed=1)
    ref_c = m.continua_from_latent(ref_h)
    hc2 = hc.clone()
    hc2[2, 5, 6] = float("nan")
    h = m.sample_latent(hm, hc2, 9, seed=1)
    c = m.continua_from_latent(h)
    assert torch.isnan(h[2]).all() and torch.isnan(c[2]).all()
    keep = [0, 1, 3]
    assert torch.equal(h[keep], ref_h[keep]) and torch.equal(c[keep], ref_c[keep])
    hm2 = hm.clone()
    hm2[0, 3] = float("nan")
    h = m.sample_latent(hm2, hc, 9, seed=1)
    assert torch.isnan(h[0]).all() and torch.equal(h[1:], ref_h[1:])


def test_writer_past_two_to_the_31_elements(dev):
    import torch
    R, npix, nh = 262144, 8300, 8
    assert R * npix > 2 ** 31
    m = plain_model(dev, npix, nh, seed=99)
    g = torch.Generator(device=dev).manual_seed(5)
    h = torch.randn((R, nh), generator=g, device=dev)
    out = m.continua_from_latent(h)
    F, mu = m.F.cpu().numpy().astype(np.float64), m.mu.cpu().numpy().astype(np.float64)
    rows = [0, R // 2, R - 2, R - 1]
    want = mu + h[rows].cpu().numpy().astype(np.float64) @ F.T
    got = out[rows].cpu().numpy().astype(np.float64)
    assert (np.max(np.abs(got - want), axis=1) <= 2e-6 * np.max(np.abs(want), axis=1)).all()
    del out


def test_loud_failures(dev):
    import torch
    from qfa_amd._lib import QFAHipError
    m = plain_model(dev, 50, 8)
    hm, hc = identity_posterior(dev, 3, 8)
    with pytest.raises(QFAHipError):
        m.sample_latent(hm.cpu(), hc, 4)
    with pytest.raises(QFAHipError):
        m.sample_latent(hm, hc[:, :, :4].contiguous(), 4)
    with pytest.raises(QFAHipError):
        m.sample_latent(hm.double(), hc, 4)
    with pytest.raises(QFAHipError):
        m.sample_latent(hm, hc, 0)
    with pytest.raises(QFAHipError):
        m.continua_from_latent(torch.zeros((3, 7), device=dev))
    with pytest.raises(QFAHipError):
        m.sample_continua(n_samples=0, hmean=hm, hcov=hc)
    m.mu = None
    with pytest.raises(QFAHipError):
        m.continua_from_latent(torch.zeros((3, 8), device=dev))
