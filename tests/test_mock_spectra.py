"""Mock spectra and posterior-predictive replicates on the MI355X (QFA.sample_spectra / posterior_predictive,
qfa_mock_spectra_f32) against the numpy float64 port of the draw contract (tests/_mock_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import _mock_ref as R
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
    if x.dtype == np.int32:
        return torch.tensor(x, dtype=torch.int32, device=dev)
    return torch.tensor(x, dtype=torch.float32, device=dev)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def geometry(npix, nb, nh, B, seed, masks=True):
    """the numpy recipe's geometry (qfa_amd/synthetic.py) at a chosen (N_pix, N_b): z_qso ~ U(2, 3.5), blue pixels log-spaced
    from 1030 A up to Lyman alpha, sigma = mu / snr (0.8 + 0.4 u), Poisson(2) masked runs + 1 % dropped pixels, -999 under
    the mask.  Returns float32 / bool numpy arrays and the float64 1 + z of the factored form's float32 factors."""
    from qfa_amd import synthetic
    rng = np.random.default_rng(seed)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    ratio = (10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / synthetic.LYA).astype(np.float32)
    zq1 = (1.0 + rng.uniform(2.0, 3.5, size=B)).astype(np.float32)
    zp1 = zq1.astype(np.float64)[:, None] * ratio.astype(np.float64)[None, :]
    zabs = (zp1 - 1.0).astype(np.float32)
    snr = np.exp(rng.uniform(np.log(2.0), np.log(100.0), size=B))
    sigma = (mu[None, :] / snr[:, None] * (0.8 + 0.4 * rng.random((B, npix)))).astype(np.float32)
    mask = np.ones((B, npix), dtype=bool)
    if masks:
        for s in range(B):
            for _ in range(rng.poisson(2.0)):
                ln, st = int(rng.integers(10, 101)), int(rng.integers(0, npix))
                mask[s, st:st + ln] = False
        mask &= rng.random((B, npix)) >= 0.01
    sigma = np.where(mask, sigma, np.float32(-999.0)).astype(np.float32)
    return {"p": p, "mu": mu, "ratio": ratio, "zq1": zq1, "zp1": zp1, "zabs": zabs, "error": sigma, "mask": mask}


def make_model(dev, g, nb, nr, nh, tau=None):
    from qfa_amd import QFA
    m = QFA(nb, nr, nh, dev, model_params=g["p"]) if tau is None else QFA(nb, nr, nh, dev, tau=tau, model_params=g["p"])
    m.mu = T(g["mu"], dev)
    return m


def call_c(m, error, h, seed, row0, *, zabs=None, mask=None, zq1=None, ratio=None, A_blue=None, rows=None, row_stride=0,
           flux=None, delta=None, B=None, S=None, Nh=None, ws_bytes=None, null=()):
    """qfa_mock_spectra_f32 by hand; returns the status.  ``null``: names of required arguments to pass as NULL."""
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    ps = m._params_struct()
    bs = _lib.Batch()
    ptr = lambda t: None if t is None else t.data_ptr()
    bs.delta, bs.error, bs.zabs, bs.mask = None, ptr(error), ptr(zabs), ptr(mask)
    bs.A_blue, bs.zq1, bs.pix_ratio, bs.rows, bs.row_stride = ptr(A_blue), ptr(zq1), ptr(ratio), ptr(rows), int(row_stride)
    B = h.shape[0] if B is None else B
    S = h.shape[1] if S is None else S
    Nh = m.Nh if Nh is None else Nh
    need = lib.qfa_mock_workspace_bytes(m.Npix, m.Nh)
    ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    arg = lambda name, v: None if name in null else v
    st = lib.qfa_mock_spectra_f32(
        arg("p", C.byref(ps)), arg("mu", C.c_void_p(m.mu.data_ptr())), arg("b", C.byref(bs)), arg("tau", C.byref(m._tau_model)),
        arg("h", C.c_void_p(h.data_ptr())), B, S, m.Npix, m.Nb, Nh, C.c_uint64(seed), row0,
        C.c_void_p(ptr(flux)), C.c_void_p(ptr(delta)), arg("workspace", C.c_void_p(ws.data_ptr())),
        need if ws_bytes is None else ws_bytes, _lib.current_stream(m.device))
    torch.cuda.synchronize()
    return st


# ------------------------------------------------------------------------------------------------------------ 1. normals
@pytest.mark.parametrize("npix", [1, 3, 300, 1913])
def test_normals_bits_match_the_port(dev, npix):
    """mu = 0, F = 0, Psi = 0, omega = 0, sigma = 1: flux = e exactly; <= 1 ulp from the port (the float64 Box-Muller's libm)."""
    import torch
    from qfa_amd import QFA
    nh, B = 4, 3
    p = {"F": np.zeros((npix, nh), np.float32), "Psi": np.zeros(npix, np.float32), "omega": np.zeros(0, np.float32),
         "tau0": np.float32(0.02), "c0": np.float32(0.3), "beta": np.float32(2.0)}
    m = QFA(0, npix, nh, dev, model_params=p)
    m.mu = torch.zeros(npix, dtype=torch.float32, device=dev)
    err = torch.ones((B, npix), dtype=torch.float32, device=dev)
    for seed in (0, 2 ** 64 - 1):
        for row0 in (0, 2 ** 32 - 1, 2 ** 40):
            for S in (1, 3):
                flux, delta = m.sample_spectra(err, None, None, n_samples=S, seed=seed, offset=row0, return_delta=True)
                e = R.pixel_normals(seed, row0 + np.arange(B), S, npix)
                got = flux.cpu().numpy()
                assert got.shape == (B, S, npix)
                worst = ulps(got, e).max()
                print(f"npix {npix} seed {seed} row0 {row0} S {S}: max {worst:.2f} ulp")
                assert worst <= 1.0, (seed, row0, S)
                assert np.array_equal(delta.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------------------ 2. values
def custom_tau64(z):
    return 0.0045 * (1.0 + z) ** 3.1


@pytest.mark.parametrize("nh", [1, 8, 9, 32])
@pytest.mark.parametrize("npix,nb", [(300, 113), (257, 0), (64, 64), (1913, 720)])
def test_values_match_float64(dev, npix, nb, nh):
    """every unmasked element of flux and delta within 1e-5 T of the float64 port, T = A (|mu| + sum |F h|) + sqrt(D) |e|, in
    every input form, output pointers offset by 0..3 floats.
    Measured maxima of |err| / T on MI355X (over all sixteen cases): see DESIGN.md, section on mock spectra."""
    import torch
    B, S, seed, row0 = 5, 3, 1234, 2 ** 33 + 7
    g = geometry(npix, nb, nh, B, seed=npix + 3 * nh)
    m = make_model(dev, g, nb, npix - nb, nh)
    hm = torch.zeros((B, nh), dtype=torch.float32, device=dev)
    hc = torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1)
    h = m.sample_latent(hm, hc, S, seed=seed, offset=row0)
    h64 = h.cpu().numpy()
    err, mask, zabs = T(g["error"], dev), T(g["mask"], dev), T(g["zabs"], dev)
    want = R.spectra(g["p"], g["mu"], g["error"], g["zp1"], g["mask"], h64, seed, row0)
    A64 = np.exp(-custom_tau64(g["zp1"] - 1.0))
    want_a = R.spectra(g["p"], g["mu"], g["error"], g["zp1"], g["mask"], h64, seed, row0, A_blue=A64.astype(np.float32))
    # the resident form: rows of a larger, padded array in another order
    stride, N = npix + 5, B + 3
    rows = np.array([6, 0, 3, 7, 2], dtype=np.int32)
    err_res = np.full((N, stride), np.nan, dtype=np.float32)
    mask_res = np.zeros((N, stride), dtype=bool)
    zabs_res = np.full((N, max(nb, 1)), np.nan, dtype=np.float32)[:, :nb]
    err_res[rows, :npix], mask_res[rows, :npix], zabs_res[rows] = g["error"], g["mask"], g["zabs"]
    forms = {
        "zabs": dict(error=err, mask=mask, zabs=zabs),
        "factored": dict(error=err, mask=mask, zq1=T(g["zq1"], dev), ratio=T(g["ratio"], dev)),
        "A_blue": dict(error=err, mask=mask, zabs=zabs, A_blue=T(A64.astype(np.float32), dev)),
        "rows": dict(error=T(err_res, dev), mask=T(mask_res, dev), zabs=T(np.ascontiguousarray(zabs_res), dev),
                     rows=T(rows, dev), row_stride=stride),
    }
    use = np.broadcast_to(g["mask"][:, None, :], (B, S, npix))
    n = B * S * npix
    for off, (name, kw) in enumerate(forms.items()):
        if nb == 0:
            kw = {k: v for k, v in kw.items() if k not in ("zabs", "zq1", "ratio", "A_blue")}
        ref = want_a if name == "A_blue" else want
        bufs = [torch.full((n + 8,), -7.0, dtype=torch.float32, device=dev) for _ in range(2)]
        fo, do = (b[off:off + n] for b in bufs)
        assert call_c(m, kw.pop("error"), h, seed, row0, flux=fo, delta=do, **kw) == 0, name
        for key, out, buf in (("flux", fo, bufs[0]), ("delta", do, bufs[1])):
            got = out.cpu().numpy().astype(np.float64).reshape(B, S, npix)
            rel = np.abs(got - ref[key])[use] / ref["T"][use]
            print(f"npix {npix} nb {nb} nh {nh} {name} {key}: max |err| / T = {rel.max():.3e}")
            assert (rel <= 1e-5).all(), (name, key, rel.max())
            assert (got[~use] == -999.0).all(), (name, key)
            rest = buf.cpu().numpy()
            assert (rest[:off] == -7.0).all() and (rest[off + n:] == -7.0).all(), (name, key)


@pytest.mark.parametrize("npix,nb,nh,B", [(300, 20, 8, 40), (32, 32, 4, 40), (8, 5, 2, 600000)])
def test_factored_form_with_many_spectra_per_block(dev, npix, nb, nh, B):
    """The per-spectrum factors of the factored-z form are formed by one lane per spectrum and read by every lane of the wave:
    a block must serve more spectra than its boundary wave has lanes with blue pixels (5 of 64 at N_b = 20, 8 at N_pix = N_b =
    32; a block walks 16 spectra at S = 1), and more than 64 (B = 600 000 on one strip: 74 spectra per block).  Same bar as
    test_values_match_float64."""
    S, seed, row0 = 1, 99, 5
    g = geometry(npix, nb, nh, B, seed=npix + nb, masks=B <= 1000)
    m = make_model(dev, g, nb, npix - nb, nh)
    zf = (T(g["zq1"], dev), T(g["ratio"], dev))
    flux, delta, h = m.sample_spectra(T(g["error"], dev), None, T(g["mask"], dev), n_samples=S, seed=seed, offset=row0, zfac=zf,
                                      return_delta=True, return_latent=True)
    want = R.spectra(g["p"], g["mu"], g["error"], g["zp1"], g["mask"], h.cpu().numpy(), seed, row0)
    use = np.broadcast_to(g["mask"][:, None, :], (B, S, npix))
    for key, out in (("flux", flux), ("delta", delta)):
        got = out.cpu().numpy().astype(np.float64)
        rel = np.abs(got - want[key])[use] / want["T"][use]
        print(f"npix {npix} nb {nb} nh {nh} B {B} factored {key}: max |err| / T = {rel.max():.3e}")
        assert (rel <= 1e-5).all(), (key, rel.max(), np.unique(np.nonzero((np.abs(got - want[key]) > 1e-5 * want["T"]) & use)[0])[:20])
        assert (got[~use] == -999.0).all(), key


def test_custom_tau_callable_through_the_method(dev):
    """a tau callable is evaluated on zabs by the method and handed over as A_blue (the reference's constructor argument)"""
    import torch
    npix, nb, nh, B, S = 300, 113, 8, 4, 2
    g = geometry(npix, nb, nh, B, seed=77)
    m = make_model(dev, g, nb, npix - nb, nh, tau=lambda z: 0.0045 * (1.0 + z) ** 3.1)
    flux, h = m.sample_spectra(T(g["error"], dev), T(g["zabs"], dev), T(g["mask"], dev), n_samples=S, seed=3, return_latent=True)
    A64 = np.exp(-custom_tau64(g["zabs"].astype(np.float64)))
    want = R.spectra(g["p"], g["mu"], g["error"], g["zp1"], g["mask"], h.cpu().numpy(), 3, 0, A_blue=A64)
    use = np.broadcast_to(g["mask"][:, None, :], (B, S, npix))
    rel = np.abs(flux.cpu().numpy().astype(np.float64) - want["flux"])[use] / want["T"][use]
    assert (rel <= 1e-5).all(), rel.max()


# ------------------------------------------------------------------------------------------------------------ 3. masks
def test_masks_and_sentinels(dev):
    import torch
    npix, nb, nh, B, S = 300, 113, 8, 5, 3
    g = geometry(npix, nb, nh, B, seed=31, masks=False)
    m = make_model(dev, g, nb, npix - nb, nh)
    err, zabs = T(g["error"], dev), T(g["zabs"], dev)
    hm = torch.zeros((B, nh), dtype=torch.float32, device=dev)
    hc = torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1)
    h = m.sample_latent(hm, hc, S, seed=9, offset=4)
    f0, d0 = m.sample_spectra(err, zabs, None, seed=9, offset=4, h=h, return_delta=True)
    f1, d1 = m.sample_spectra(err, zabs, torch.ones((B, npix), dtype=torch.bool, device=dev), seed=9, offset=4, h=h,
                              return_delta=True)
    assert torch.equal(f0, f1) and torch.equal(d0, d1)
    assert torch.isfinite(f0).all() and (f0 != -999.0).all()
    rng = np.random.default_rng(5)
    mask = T(rng.random((B, npix)) > 0.3, dev)
    m3 = mask[:, None, :].expand(B, S, npix)
    for junk in (float("nan"), float("inf"), -999.0):
        e2 = torch.where(mask, err, torch.full_like(err, junk))
        f2, d2 = m.sample_spectra(e2, zabs, mask, seed=9, offset=4, h=h, return_delta=True)
        assert (f2[~m3] == -999.0).all() and (d2[~m3] == -999.0).all(), junk
        assert torch.equal(f2[m3], f0[m3]) and torch.equal(d2[m3], d0[m3]), junk
    # a NaN latent row poisons its own (b, s) row only
    hn = h.clone()
    hn[2, 1, 3] = float("nan")
    f3 = m.sample_spectra(err, zabs, mask, seed=9, offset=4, h=hn)
    f2 = m.sample_spectra(err, zabs, mask, seed=9, offset=4, h=h)
    assert torch.isnan(f3[2, 1][mask[2]]).all() and (f3[2, 1][~mask[2]] == -999.0).all()
    keep = torch.ones((B, S), dtype=torch.bool, device=dev)
    keep[2, 1] = False
    assert torch.equal(f3[keep], f2[keep]) and torch.isfinite(f3[keep]).all()


# ------------------------------------------------------------------------------------------------------------ 4. split
def test_split_independence_and_by_hand_composition(dev):
    import torch
    npix, nb, nh, B, S = 300, 113, 8, 5, 3
    g = geometry(npix, nb, nh, B, seed=41)
    m = make_model(dev, g, nb, npix - nb, nh)
    err, zabs, mask = T(g["error"], dev), T(g["zabs"], dev), T(g["mask"], dev)
    whole, dwhole, hwhole = m.sample_spectra(err, zabs, mask, n_samples=S, seed=17, offset=100, return_delta=True,
                                             return_latent=True)
    parts = [m.sample_spectra(err[a:b].contiguous(), zabs[a:b].contiguous(), mask[a:b].contiguous(), n_samples=S, seed=17,
                              offset=100 + a, return_delta=True) for a, b in ((0, 2), (2, 5))]
    assert torch.equal(torch.cat([x[0] for x in parts]), whole)
    assert torch.equal(torch.cat([x[1] for x in parts]), dwhole)
    assert not torch.equal(whole, m.sample_spectra(err, zabs, mask, n_samples=S, seed=18, offset=100))
    # by hand: sample_latent from the prior, then the C entry point
    hm = torch.zeros((B, nh), dtype=torch.float32, device=dev)
    hc = torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1)
    h = m.sample_latent(hm, hc, S, seed=17, offset=100)
    assert torch.equal(h, hwhole)
    fo = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
    assert call_c(m, err, h, 17, 100, zabs=zabs, mask=mask, flux=fo) == 0
    assert torch.equal(fo, whole)
    do = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
    assert call_c(m, err, h, 17, 100, zabs=zabs, mask=mask, delta=do) == 0          # flux == NULL
    assert torch.equal(do, dwhole)
    # the factored form through the method and through a resident batch give the same bits as each other
    from qfa_amd.resident import ResidentBatch
    zf = (T(g["zq1"], dev), T(g["ratio"], dev))
    ff = m.sample_spectra(err, None, mask, n_samples=S, seed=17, offset=100, zfac=zf)
    rb = ResidentBatch(None, None, err, mask, zf[0], zf[1], T(np.arange(B, dtype=np.int32), dev), npix, nb)   # no flux, no delta
    assert torch.equal(m.sample_spectra(batch=rb, n_samples=S, seed=17, offset=100), ff)
    out = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
    assert m.sample_spectra(err, zabs, mask, n_samples=S, seed=17, offset=100, out=out) is out and torch.equal(out, whole)


# ------------------------------------------------------------------------------------------------------------ 5. moments
def test_second_moments(dev):
    import torch
    npix, nb, nh, B, S = 300, 113, 8, 2, 4096
    g = geometry(npix, nb, nh, B, seed=51, masks=False)
    m = make_model(dev, g, nb, npix - nb, nh)
    flux = m.sample_spectra(T(g["error"], dev), T(g["zabs"], dev), None, n_samples=S, seed=23).double().cpu().numpy()
    ref = R.spectra(g["p"], g["mu"], g["error"], g["zp1"], None, np.zeros((B, 1, nh)), 23, 0)
    F = g["p"]["F"].astype(np.float64)
    G = F @ F.T
    pairs = [(i, (i * 7 + 13 * k + 1) % npix) for k, i in enumerate(range(3, npix, 15))]
    assert len(pairs) == 20 and all(i != j for i, j in pairs)
    for b in range(B):
        A, D = ref["A"][b], ref["D"][b]
        var = D + A * A * np.diag(G)
        x = flux[b] - flux[b].mean(0)
        sv = (x * x).sum(0) / (S - 1)
        assert (np.abs(sv - var) <= 5 * var * np.sqrt(2.0 / (S - 1))).all(), b
        assert (np.abs(flux[b].mean(0) - A * g["mu"]) <= 5 * np.sqrt(var / S)).all(), b
        for i, j in pairs:
            cov = A[i] * A[j] * G[i, j]
            sc = (x[:, i] * x[:, j]).sum() / (S - 1)
            assert abs(sc - cov) <= 5 * np.sqrt((var[i] * var[j] + cov * cov) / (S - 1)), (b, i, j)


# ------------------------------------------------------------------------------------------------------------ 6. calibration
def test_prior_mocks_are_calibrated_against_predict(dev):
    """h of 2048 prior mocks against the posterior predict() infers from them: E (h - hmean)^T hcov^-1 (h - hmean) = N_h"""
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid()
    npix, nh, B = len(wav), 8, 2048
    g = geometry(npix, nb, nh, B, seed=61)
    m = make_model(dev, g, nb, nr, nh)
    err, zabs, mask = T(g["error"], dev), T(g["zabs"], dev), T(g["mask"], dev)
    flux, h = m.sample_spectra(err, zabs, mask, seed=29, return_latent=True)
    _, hm, hc, _, _ = m.predict(flux[:, 0].contiguous(), err, zabs, mask)
    d = (h[:, 0] - hm).double().cpu().numpy()
    q = np.einsum("bi,bij,bj->b", d, np.linalg.inv(hc.double().cpu().numpy()), d)
    print(f"mean chi2 = {q.mean():.4f} (N_h = {nh}, bound {5 * np.sqrt(2 * nh / B):.4f})")
    assert abs(q.mean() - nh) <= 5 * np.sqrt(2.0 * nh / B)


# ------------------------------------------------------------------------------------------------------------ 7. / 8.
def test_posterior_predictive_is_the_composition(dev):
    import torch
    from qfa_amd import synthetic
    npix, nh, B, S = 400, 8, 6, 4
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=7)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=107)
    m = make_model(dev, {"p": p, "mu": mu}, nb, nr, nh)
    inputs = tuple(T(b[k], dev) for k in ("flux", "error", "zabs", "mask"))
    rep = m.posterior_predictive(*inputs, n_samples=S, seed=5, offset=10)
    _, hm, hc, _, _ = m.predict(*inputs)
    h = m.sample_latent(hm, hc, S, seed=5, offset=10)
    assert torch.equal(rep, m.sample_spectra(*inputs[1:], seed=5, offset=10, h=h))
    assert torch.equal(rep, m.sample_spectra(*inputs[1:], n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc))
    m3 = inputs[3][:, None, :].expand(B, S, npix)
    assert (rep[~m3] == -999.0).all() and torch.isfinite(rep[m3]).all()


class _ListLoader(object):
    """the reference's per-spectrum dataloader contract: loader[i] = (flux, error, zabs, mask, path)"""

    def __init__(self, inputs):
        self.inputs = inputs

    def __len__(self):
        return self.inputs[0].shape[0]

    def __getitem__(self, i):
        return tuple(x[i] for x in self.inputs) + (f"spec{i:03d}",)


def test_predict_to_npz_replicates_do_not_depend_on_batch_size(dev, tmp_path):
    from qfa_amd import synthetic
    npix, nh, B = 300, 8, 10
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=8)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=108)
    m = make_model(dev, {"p": p, "mu": mu}, nb, nr, nh)
    inputs = tuple(T(b[k], dev) for k in ("flux", "error", "zabs", "mask"))
    loader = _ListLoader(inputs)
    w3 = m.predict_to_npz(loader, str(tmp_path / "b3"), batch_size=3, n_replicates=2, seed=21)
    w4 = m.predict_to_npz(loader, str(tmp_path / "b4"), batch_size=4096, n_replicates=2, seed=21, n_samples=3)
    w0 = m.predict_to_npz(loader, str(tmp_path / "b0"), batch_size=4096)
    assert w3 == w4 == w0 and len(w3) == B
    whole = m.posterior_predictive(*inputs, n_samples=2, seed=21).cpu().numpy()
    for i, name in enumerate(w3):
        a, c, z = (np.load(str(tmp_path / d / name)) for d in ("b3", "b4", "b0"))
        assert a["flux_replicates"].shape == (2, npix)
        assert np.array_equal(a["flux_replicates"], c["flux_replicates"])
        assert np.array_equal(a["flux_replicates"], whole[i])
        assert "cont_samples" in c.files and "cont_samples" not in a.files
        assert sorted(z.files) == ["cont", "hcov", "hmean", "ll", "uncertainty"]
        for k in z.files:
            assert np.array_equal(a[k], z[k]), k


# ------------------------------------------------------------------------------------------------------------ 9. capture
def test_graph_capture_replays_the_eager_bits(dev):
    import torch
    npix, nb, nh, B, S = 300, 113, 8, 5, 3
    g = geometry(npix, nb, nh, B, seed=91)
    m = make_model(dev, g, nb, npix - nb, nh)
    err, mask = T(g["error"], dev), T(g["mask"], dev)
    zf = (T(g["zq1"], dev), T(g["ratio"], dev))
    hm = torch.zeros((B, nh), dtype=torch.float32, device=dev)
    hc = torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1)
    eager = m.sample_spectra(err, None, mask, n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc, zfac=zf)   # (workspace allocated)
    out = torch.zeros((B, S, npix), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        m.sample_spectra(err, None, mask, n_samples=S, seed=5, offset=10, hmean=hm, hcov=hc, zfac=zf, out=out)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------------------ 10. failures
def test_loud_failures(dev):
    import torch
    from qfa_amd._lib import QFAHipError
    npix, nb, nh, B, S = 64, 20, 8, 3, 2
    g = geometry(npix, nb, nh, B, seed=3)
    m = make_model(dev, g, nb, npix - nb, nh)
    err, zabs, mask = T(g["error"], dev), T(g["zabs"], dev), T(g["mask"], dev)
    h = torch.zeros((B, S, nh), dtype=torch.float32, device=dev)
    fo = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
    ok = dict(zabs=zabs, mask=mask, flux=fo)
    assert call_c(m, err, h, 0, 0, **ok) == 0
    assert call_c(m, err, h, 0, 0, zabs=zabs, flux=fo) == 0                           # mask == NULL is allowed
    for name in ("p", "mu", "b", "tau", "h", "workspace"):
        assert call_c(m, err, h, 0, 0, null=(name,), **ok) == -1, name
    assert call_c(m, None, h, 0, 0, **ok) == -1                                       # error
    assert call_c(m, err, h, 0, 0, zabs=zabs, mask=mask) == -1                        # neither flux nor delta
    assert call_c(m, err, h, 0, 0, mask=mask, flux=fo) == -1                          # blue pixels without zabs or factors
    assert call_c(m, err, h, 0, 0, mask=mask, flux=fo, zq1=T(g["zq1"], dev)) == -1    # half of the factored form
    assert call_c(m, err, h, 0, 0, B=-1, **ok) == -2
    assert call_c(m, err, h, 0, 0, S=0, **ok) == -2
    assert call_c(m, err, h, 0, 0, Nh=0, **ok) == -2
    assert call_c(m, err, h, 0, 0, Nh=33, **ok) == -2
    assert call_c(m, err, h, 0, -1, **ok) == -2
    assert call_c(m, err, h, 0, 0, row_stride=npix - 1, **ok) == -2
    from qfa_amd import _lib
    need = _lib.lib().qfa_mock_workspace_bytes(npix, nh)
    assert call_c(m, err, h, 0, 0, ws_bytes=need - 1, **ok) == -3
    fo.fill_(-5.0)
    assert call_c(m, err, h, 0, 0, B=0, **ok) == 0 and (fo == -5.0).all()             # B = 0 does nothing
    # the Python surface
    with pytest.raises(QFAHipError):
        m.sample_spectra(err.cpu(), zabs, mask)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err[:, :-1].contiguous(), zabs, mask)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err.double(), zabs, mask, h=h.double())
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask.float())
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, n_samples=0)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, seed=2 ** 64)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, seed=-1)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, offset=-1)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, n_samples=3, h=h)                           # h is (B, 2, Nh)
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, hmean=torch.zeros((B, nh), device=dev))      # hcov missing
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask, out=torch.empty((B, 2, npix), device=dev))   # n_samples = 1
    m.mu = None
    with pytest.raises(QFAHipError):
        m.sample_spectra(err, zabs, mask)
