"""The redshift finder on the GPU against the float64 restatement (tests/_zscan_ref.py): every element of the scan at the shapes
where its tiling can go wrong, the recovery of injected shifts, bit-level invariants (repeat calls, row independence across the
chunk boundary, the two input forms, the catalogue walk), masks and edges, and m = 0 against predict.

The bars are the issue's: |llr - llr_f64| <= 1e-5 max(|NLL_0|, |NLL_s|) per element and 5e-6 relative for nll0 -- the project's
per-spectrum NLL bar and its double on a difference of two."""
import numpy as np
import pytest
import torch

import _zscan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N_h, N_pix, m, N_b rule, B, tau model): every N_h in {1, 3, 8, 9, 16, 17, 32}, N_pix in {35, 96, 133, 200}, m in {0, 1, 7, 8, 16,
# 17, 40} (n_s = 1 .. 81: both sides of a 16-candidate tile, up to six tiles), N_b in {0, m, m + 1, 0.4 N_pix, N_pix}, B in {1, 5, 19},
# the four tau models; N_b = N_pix draws z_qso from 4.8 .. 5.0, where tau reaches 3 at the red end
CASES = [(1, 35, 0, "frac", 1, "becker"), (1, 35, 17, "m+1", 5, "fg"), (3, 35, 1, "0", 5, "kamble"), (3, 96, 7, "m", 19, "mock"),
         (8, 96, 8, "frac", 5, "becker"), (8, 133, 16, "m+1", 19, "fg"), (8, 200, 40, "npix", 5, "becker"), (9, 96, 17, "frac", 5, "kamble"),
         (9, 133, 40, "m", 1, "mock"), (9, 200, 7, "0", 19, "becker"), (16, 133, 8, "npix", 5, "fg"), (16, 200, 16, "frac", 19, "becker"),
         (16, 96, 40, "m+1", 5, "kamble"), (17, 133, 1, "frac", 5, "mock"), (17, 200, 17, "npix", 1, "becker"), (17, 96, 0, "npix", 19, "fg"),
         (32, 200, 40, "frac", 5, "becker"), (32, 133, 16, "0", 5, "kamble"), (32, 35, 7, "m", 19, "mock"), (32, 96, 8, "m+1", 1, "becker")]


def T(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(x), device=DEV, dtype=dtype)


def nb_of(rule, npix, m):
    return {"0": 0, "m": m, "m+1": m + 1, "frac": int(0.4 * npix), "npix": npix}[rule]


def make_model(params, mu, nb, tau="becker"):
    from qfa_amd import QFA
    npix, nh = params["F"].shape
    mdl = QFA(nb, npix - nb, nh, torch.device(DEV), tau=tau, model_params=params)
    mdl.mu = T(mu, torch.float32)
    return mdl


def gpu_scan(mdl, d, wav, m, rows=slice(None), flux=None, error=None, mask=None):
    f = d["flux"] if flux is None else flux
    e = d["error"] if error is None else error
    k = d["mask"] if mask is None else mask
    out = mdl.redshift_scan(T(f[rows]), T(e[rows]), T(k[rows]), zqso=d["zqso"][rows], wav_grid=wav, max_shift=m)
    torch.cuda.synchronize()
    return out


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.int32) else t.view(torch.int64)


def same_scan(a, b, rows_a=slice(None), rows_b=slice(None)):
    """every output of two scans, bit for bit (equal NaNs equal)"""
    return all(torch.equal(bits(getattr(a, n))[rows_a], bits(getattr(b, n))[rows_b])
               for n in ("llr", "nll0", "best_s", "best_llr", "offset", "sigma_pix"))


def check_outputs(scan, m):
    """what the outputs owe each other: llr[:, m] == 0, the arg-max in the rule's order, the parabola through the float32 llr"""
    llr = scan.llr.cpu().numpy()
    bs = scan.best_s.cpu().numpy()
    assert llr.shape[1] == 2 * m + 1 and np.all(llr[:, m] == 0.0)
    assert np.array_equal(bs, R.argbest(llr))
    assert np.array_equal(scan.best_llr.cpu().numpy(), llr[np.arange(len(bs)), bs + m])
    off, sig = R.parabola(llr, bs)
    assert np.array_equal(scan.offset.cpu().numpy(), off, equal_nan=True)
    assert np.allclose(scan.sigma_pix.cpu().numpy(), sig, rtol=1e-14, atol=0, equal_nan=True)
    edge = np.abs(bs) == m
    assert np.all(np.isnan(off[edge])) and np.array_equal(scan.at_edge(), edge | (m == 0))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "nh%d_px%d_m%d_nb%s_B%d_%s" % c)
def test_every_element_against_float64(case):
    nh, npix, m, rule, B, tau = case
    nb = nb_of(rule, npix, m)
    params, mu, wav, _ = R.model(npix, nb, nh, seed=npix + nh)
    t = np.random.default_rng(m + nh).integers(-m, m + 1, size=B)
    zq = (4.8, 5.0) if rule == "npix" else (2.2, 3.4)
    d = R.draw(params, mu, wav, B, 7 * npix + nh + m, t, zq=zq, tau_which=tau)
    if rule == "npix":
        from oracle import qfa_oracle as O
        assert np.max(O.tau_eff(R.z_pixels(d["zqso"], wav).astype(np.float64), "becker")) >= 3.0
    rl, r0, rn = R.scan(params, mu, d["flux"], d["error"], d["mask"], d["zqso"], wav, m, tau)
    scan = gpu_scan(make_model(params, mu, nb, tau), d, wav, m)
    check_outputs(scan, m)
    llr, nll0 = scan.llr.cpu().numpy().astype(np.float64), scan.nll0.cpu().numpy().astype(np.float64)
    scale = np.maximum(np.abs(r0)[:, None], np.abs(rn))
    e_llr, e_nll = np.abs(llr - rl) / (R.BAR * scale), np.abs(nll0 - r0) / (R.NLL_BAR * np.abs(r0))
    print("%s: llr at %.3f of its bar, nll0 at %.3f of its bar" % ("nh%d_px%d_m%d_nb%s_B%d_%s" % case, e_llr.max(), e_nll.max()))
    assert np.all(e_llr <= 1.0) and np.all(e_nll <= 1.0)


@pytest.mark.parametrize("i", range(len(R.RECOVERY)))
def test_recovery_of_injected_shifts(i):
    c = R.recovery_case(i)
    m = c["m"]
    top = np.sort(c["nll"], axis=1)
    bar = R.BAR * np.abs(c["nll"]).max(axis=1)
    assert np.all(top[:, 1] - top[:, 0] > 100.0 * bar)             # the precondition: the reference alone separates the top two
    scan = gpu_scan(make_model(c["params"], c["mu"], c["nb"]), c, c["wav"], m)
    check_outputs(scan, m)
    bs = scan.best_s.cpu().numpy()
    assert np.array_equal(bs, np.argmin(c["nll"], axis=1) - m) and np.array_equal(bs, c["shift"])
    off, sig = R.parabola(c["llr"], c["shift"])
    inner = np.abs(c["shift"]) < m
    assert np.all(np.isfinite(off[inner])) and np.sum(inner) > len(bs) // 2
    g_off, g_sig = scan.offset.cpu().numpy(), scan.sigma_pix.cpu().numpy()
    print("set", i, "max |d off|", float(np.max(np.abs(g_off - off)[inner])), "max |d sig|", float(np.max(np.abs(g_sig - sig)[inner])))
    assert np.all(np.abs(g_off - off)[inner] <= 1e-3) and np.all(np.abs(g_sig - sig)[inner] <= 1e-3)
    assert np.all(np.isnan(g_off[~inner])) and np.all(np.isnan(g_sig[~inner]))
    # the host arithmetic on the device's outputs: the refined redshift undoes the injected shift to the parabola's offset
    assert np.allclose(scan.z(), (1.0 + c["zqso"]) * 10.0 ** (-(bs + np.where(inner, g_off, 0.0)) * c["dloglam"]) - 1.0, rtol=1e-15)
    ev = scan.log_evidence().cpu().numpy()
    assert np.all(ev >= scan.best_llr.cpu().numpy() - np.log(2 * m + 1) - 1e-9)


def test_two_calls_rows_alone_and_both_input_forms():
    from qfa_amd.resident import ResidentBatch
    c = R.recovery_case(1)                                         # N_pix 96, N_h 9, m 17: three candidate tiles, the last one ragged
    m, B = c["m"], len(c["flux"])
    mdl = make_model(c["params"], c["mu"], c["nb"])
    a, b = gpu_scan(mdl, c, c["wav"], m), gpu_scan(mdl, c, c["wav"], m)
    assert same_scan(a, b)
    for r in (0, 13, B - 1):
        assert same_scan(gpu_scan(mdl, c, c["wav"], m, rows=slice(r, r + 1)), a, rows_b=slice(r, r + 1))
    assert same_scan(gpu_scan(mdl, c, c["wav"], m, rows=slice(3, 12)), a, rows_b=slice(3, 12))
    # the resident form: rows of padded storage, in another order
    stride, nb = 128, c["nb"]
    pad = lambda x, v, dt: T(np.concatenate([x, np.full((B, stride - x.shape[1]), v, dtype=x.dtype)], axis=1), dt)
    perm = np.random.default_rng(5).permutation(B).astype(np.int32)
    rb = ResidentBatch(pad(c["flux"], np.nan, torch.float32), None, pad(c["error"], np.nan, torch.float32), pad(c["mask"], True, torch.bool),
                       T((1.0 + c["zqso"]).astype(np.float32)), T((c["wav"][:nb] / R.LYA).astype(np.float32)), T(perm), 96, nb)
    r = mdl.redshift_scan(batch=rb, zqso=c["zqso"][perm], wav_grid=c["wav"], max_shift=m)
    torch.cuda.synchronize()
    assert same_scan(r, a, rows_b=torch.as_tensor(perm.astype(np.int64), device=DEV))


def test_rows_across_the_chunk_boundary():
    """B = chunk + 1 (the chunk read off the library's size function): the spectrum of the second chunk, the last of the first and
    the first give the bits they give alone.  (501 candidates leave a window of 12 pixels: the bits are the point here, not the shift.)"""
    from qfa_amd import _lib
    npix, nb, nh, m = R.CHUNK_SHAPE
    bc = R.chunk_size(_lib.lib().qfa_zscan_workspace_bytes, npix, nh, m)
    B = bc + 1
    params, mu, wav, _ = R.model(npix, nb, nh, seed=9)
    d = R.draw(params, mu, wav, B, 10, np.random.default_rng(11).integers(-m, m + 1, size=B))
    mdl = make_model(params, mu, nb)
    a = gpu_scan(mdl, d, wav, m)
    check_outputs(a, m)
    assert np.all(np.isfinite(a.llr.cpu().numpy()))
    for r in (0, bc - 1, bc):
        assert same_scan(gpu_scan(mdl, d, wav, m, rows=slice(r, r + 1)), a, rows_b=slice(r, r + 1))


def test_catalog_does_not_depend_on_batch_size():
    from qfa_amd.dataloader import DeviceDataloader
    npix, nh, m, B = 160, 4, 6, 23
    wav, _ = R.grid(npix)
    nb = int(np.sum(wav < R.LYA))
    params, mu, wav, _ = R.model(npix, nb, nh, seed=21)
    d = R.draw(params, mu, wav, B, 22, np.random.default_rng(23).integers(-m, m + 1, size=B))
    loader = DeviceDataloader(d["flux"], d["error"], d["zqso"], wav, 8, torch.device(DEV), shuffle=False, mode="predict")
    mdl = make_model(params, mu, nb)
    a = mdl.redshift_catalog(loader, m, batch_size=4096)
    b = mdl.redshift_catalog(loader, m, batch_size=5)
    torch.cuda.synchronize()
    assert same_scan(a, b) and a.names == b.names and len(a.names) == B
    assert np.array_equal(a.zqso, d["zqso"]) and np.all(np.isfinite(a.nll0.cpu().numpy()))
    t = a.to_table()
    assert len(t["file"]) == B and np.array_equal(t["best_s"], a.best_s.cpu().numpy())


def test_masks_and_edges():
    c = R.recovery_case(0)                                         # N_pix 160, N_h 4, m 6
    m, npix = c["m"], 160
    mdl = make_model(c["params"], c["mu"], c["nb"])
    a = gpu_scan(mdl, c, c["wav"], m)
    # NaN / inf / -999 under the mask and outside the window change no bit
    flux, error = c["flux"].copy(), c["error"].copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf, -999.0)):
        flux[k::4][~c["mask"][k::4]] = v
        error[(k + 1) % 4::4][~c["mask"][(k + 1) % 4::4]] = v
    assert same_scan(gpu_scan(mdl, c, c["wav"], m, flux=flux, error=error), a)
    # an all-masked spectrum gives zeros and touches no other
    mask = c["mask"].copy()
    mask[2] = False
    mask[3, m:npix - m] = False                                    # used pixels outside the window only
    flux[2] = np.nan
    z = gpu_scan(mdl, c, c["wav"], m, flux=flux, error=error, mask=mask)
    for r in (2, 3):
        assert np.all(z.llr[r].cpu().numpy() == 0.0) and float(z.nll0[r]) == 0.0 and int(z.best_s[r]) == 0 and float(z.best_llr[r]) == 0.0
    keep = torch.as_tensor([r for r in range(len(flux)) if r not in (2, 3)], device=DEV)
    assert same_scan(z, a, rows_a=keep, rows_b=keep)
    # sigma = 0 at both edges of the window stays finite
    error = c["error"].copy()
    mask = c["mask"].copy()
    error[:, [m, npix - m - 1]] = 0.0
    mask[:, [m, npix - m - 1]] = True
    s0 = gpu_scan(mdl, c, c["wav"], m, error=error, mask=mask)
    assert np.all(np.isfinite(s0.llr.cpu().numpy())) and np.all(np.isfinite(s0.nll0.cpu().numpy()))
    rl, r0, rn = R.scan(c["params"], c["mu"], c["flux"], error, mask, c["zqso"], c["wav"], m)
    assert np.all(np.abs(s0.llr.cpu().numpy() - rl) <= R.BAR * np.maximum(np.abs(r0)[:, None], np.abs(rn)))
    # a non-finite value in a used pixel of the window poisons that spectrum alone
    flux = c["flux"].copy()
    k = int(np.nonzero(c["mask"][5, m:npix - m])[0][0]) + m
    flux[5, k] = np.inf
    p = gpu_scan(mdl, c, c["wav"], m, flux=flux)
    assert np.all(np.isnan(p.llr[5].cpu().numpy())) and np.isnan(float(p.nll0[5])) and int(p.best_s[5]) == 0
    keep = torch.as_tensor([r for r in range(len(flux)) if r != 5], device=DEV)
    assert same_scan(p, a, rows_a=keep, rows_b=keep)


def test_true_shift_at_the_edge():
    npix, nb, nh, m = 160, 64, 4, 6
    params, mu, wav, _ = R.model(npix, nb, nh, seed=31)
    t = np.array([m, -m, m, -m, 0, 3])
    d = R.draw(params, mu, wav, len(t), 32, t)
    scan = gpu_scan(make_model(params, mu, nb), d, wav, m)
    assert np.array_equal(scan.best_s.cpu().numpy(), t)
    assert scan.at_edge().tolist() == [True, True, True, True, False, False]
    off = scan.offset.cpu().numpy()
    assert np.all(np.isnan(off[:4])) and np.all(np.isfinite(off[4:]))
    assert np.array_equal(scan.shift()[:4], t[:4].astype(np.float64))


@pytest.mark.parametrize("shape", [(133, 53, 8), (96, 38, 17)], ids=lambda s: "px%d_nb%d_nh%d" % s)
def test_zero_shift_is_predicts_ll(shape):
    npix, nb, nh = shape
    params, mu, wav, _ = R.model(npix, nb, nh, seed=41)
    d = R.draw(params, mu, wav, 7, 42, 0)
    mdl = make_model(params, mu, nb)
    scan = gpu_scan(mdl, d, wav, 0)
    z = R.z_pixels(d["zqso"], wav)[:, :nb]
    ll = mdl.predict(T(d["flux"]), T(d["error"]), T(z), T(d["mask"]))[0].reshape(-1).cpu().numpy().astype(np.float64)
    nll0 = scan.nll0.cpu().numpy().astype(np.float64)
    print("m = 0 against predict: max |d| / (bar |ll|) =", float(np.max(np.abs(nll0 - ll) / (R.NLL_BAR * np.abs(ll)))))
    assert np.all(np.abs(nll0 - ll) <= R.NLL_BAR * np.abs(ll))
    assert np.all(scan.llr.cpu().numpy() == 0.0) and np.all(scan.best_s.cpu().numpy() == 0)
