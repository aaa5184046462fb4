"""numpy float64 restatement of the DLA finder's rule (include/qfa_hip.h, qfa_dla_profiles_f32 / qfa_template_scan_f32), built from
the oracle's pixel terms and Woodbury core and the absorber restatement's transmission; plus the test data the two test files
share: model-drawn spectra with an injected DLA on a grid node."""
import numpy as np

from oracle import qfa_oracle as O
from _absorber_ref import C_KMS, transmission

LYA = 1215.67
BAR = 1e-5                      # |llr - llr_f64| <= BAR max(|NLL0|, |NLL'|): the per-spectrum NLL bar (5e-6) on a difference of two


def centres(lam_hi, dv_kms, nz):
    return lam_hi * np.exp(-np.arange(nz, dtype=np.float64) * dv_kms / C_KMS)


def profiles(wav_grid, lam_hi, dv_kms, nz, logn_lo, dlogn, n_logn, b_kms=30.0, lyb=True):
    """(nz n_logn, Npix) float64: candidate c = i n_logn + j in a spectrum at rest (z_qso = 0: 1 + z_a = lam_i / 1215.67)"""
    wav = np.asarray(wav_grid, dtype=np.float64)
    V = np.empty((nz * n_logn, len(wav)))
    for i, lam in enumerate(centres(lam_hi, dv_kms, nz)):
        for j in range(n_logn):
            V[i * n_logn + j] = transmission(wav, [lam / LYA - 1.0], [logn_lo + j * dlogn], b_kms, lyb)
    return V


def scan_one(params, mu, flux, error, zabs, mask, V, tau_which="becker", tau_series=1):
    """(nll0, nll (nc,)) of one spectrum in float64; V (nc, Npix); the mean-optical-depth model as the oracle names it"""
    p = {k: np.asarray(params[k], dtype=np.float64) for k in ("F", "Psi", "omega", "tau0", "c0", "beta")}
    w = np.asarray(mask, dtype=bool)
    x = np.where(w, np.asarray(flux, dtype=np.float64), 0.0)
    sg = np.where(w, np.asarray(error, dtype=np.float64), 1.0)
    A, zdep, _ = O.pixel_terms(p, sg, zabs, tau_which, tau_series)
    nb = p["omega"].shape[0]
    G = A * A * p["Psi"]
    G[:nb] += p["omega"] * zdep[:nb]
    mu = np.asarray(mu, dtype=np.float64)
    nll0 = O._lowrank_core(p["F"], A, G + sg * sg, w, x - A * mu)[-1]
    nll = np.array([O._lowrank_core(p["F"], v * A, v * v * G + sg * sg, w, x - v * A * mu)[-1] for v in np.asarray(V, dtype=np.float64)])
    return nll0, nll


def scan(params, mu, flux, error, zabs, mask, V, tau_which="becker", tau_series=1):
    """llr (B, nc), nll0 (B,), nll (B, nc) in float64"""
    out = [scan_one(params, mu, flux[s], error[s], zabs[s], mask[s], V, tau_which, tau_series) for s in range(len(flux))]
    nll0 = np.array([o[0] for o in out])
    nll = np.stack([o[1] for o in out])
    return nll0[:, None] - nll, nll0, nll


def scan_one_batched(params, mu, flux, error, zabs, mask, V, tau_which="becker", tau_series=1, block=2048):
    """scan_one for a long table: the same float64 quantities for `block` candidates at once -- the moments C' - I and b' by one
    matrix product against the products f_a f_b of F and against F, then numpy's batched Cholesky and solve;
    b'^T C'^-1 b' = |L^-1 b'|^2.  Working memory is a few (block, N_h, N_h) float64 arrays: about 50 MB at N_h = 32, whatever nc.
    An unmasked non-finite pixel is not this function's business (the batched Cholesky raises on it)."""
    p = {k: np.asarray(params[k], dtype=np.float64) for k in ("F", "Psi", "omega", "tau0", "c0", "beta")}
    w = np.asarray(mask, dtype=bool)
    x = np.where(w, np.asarray(flux, dtype=np.float64), 0.0)
    sg = np.where(w, np.asarray(error, dtype=np.float64), 1.0)
    A, zdep, _ = O.pixel_terms(p, sg, zabs, tau_which, tau_series)
    nb = p["omega"].shape[0]
    G = A * A * p["Psi"]
    G[:nb] += p["omega"] * zdep[:nb]
    mu = np.asarray(mu, dtype=np.float64)
    F = p["F"]
    k = F.shape[1]
    pairs = (F[:, :, None] * F[:, None, :]).reshape(len(F), k * k)
    n = float(np.sum(w))

    def nll_of(v):                                                 # v (m, Npix)
        Ap = v * A
        D = v * v * G + sg * sg
        wD = np.where(w, 1.0 / np.where(w, D, 1.0), 0.0)
        d = np.where(w, x - Ap * mu, 0.0)
        L = np.linalg.cholesky(((wD * Ap * Ap) @ pairs).reshape(len(v), k, k) + np.eye(k))
        z = np.linalg.solve(L, ((wD * Ap * d) @ F)[:, :, None])[:, :, 0]
        quad = np.sum(wD * d * d, axis=1) - np.sum(z * z, axis=1)
        logdet = np.sum(np.where(w, np.log(np.where(w, D, 1.0)), 0.0), axis=1) + 2.0 * np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), axis=1)
        return 0.5 * (quad + n * O.LOG2PI + logdet)

    V = np.asarray(V)
    nll0 = float(nll_of(np.ones((1, len(w))))[0])
    nll = np.concatenate([nll_of(V[c:c + block].astype(np.float64)) for c in range(0, len(V), block)])
    return nll0, nll


def scan_batched(params, mu, flux, error, zabs, mask, V, tau_which="becker", tau_series=1, block=2048):
    """scan through scan_one_batched: llr (B, nc), nll0 (B,), nll (B, nc) in float64"""
    out = [scan_one_batched(params, mu, flux[s], error[s], zabs[s], mask[s], V, tau_which, tau_series, block) for s in range(len(flux))]
    nll0 = np.array([o[0] for o in out])
    nll = np.stack([o[1] for o in out])
    return nll0[:, None] - nll, nll0, nll


def chunk_size(ws_bytes, npix, nh, nc, limit=64):
    """the number of spectra Bc that one chunk of the scan's batch walk holds, read off the library's own size function
    (`ws_bytes(B, Npix, Nh, nc)`: qfa_template_scan_workspace_bytes): the workspace grows strictly with B while B <= Bc and is
    constant after.  Returns the smallest b with ws(b + 1) == ws(b), after checking both halves of that statement up to `limit`."""
    ws = [int(ws_bytes(b, npix, nh, nc)) for b in range(1, limit + 2)]
    assert all(v > 0 for v in ws)
    flat = [i for i in range(limit) if ws[i + 1] == ws[i]]
    assert flat, "the workspace still grows at B = %d" % limit
    bc = flat[0] + 1
    assert all(ws[i + 1] > ws[i] for i in range(bc - 1)) and all(v == ws[bc - 1] for v in ws[bc - 1:])
    return bc


# the chunked case both test files use: (133, 64, 32), a 256 x 64 table, nine spectra
CHUNK_SHAPE = (133, 64, 32)
CHUNK_GRID = (256, 64)
CHUNK_B = 9


def draw(params, mu, wav, nb, B, seed, snr=(20.0, 100.0), masks=True, tau_which="becker", tau_series=1):
    """B spectra drawn from the model (flux, error, zabs float32; mask bool; zqso float64), the way synthetic.make_batch_numpy draws
    them, with the S/N range as an argument; masked pixels hold -999"""
    rng = np.random.default_rng(seed)
    n = len(wav)
    F, Psi, om = (np.asarray(params[k], dtype=np.float64) for k in ("F", "Psi", "omega"))
    mu = np.asarray(mu, dtype=np.float64)
    zq = rng.uniform(2.2, 3.4, size=B)
    zabs = ((1.0 + zq)[:, None] * wav[None, :nb] / LYA - 1.0).astype(np.float32)
    A, zdep = np.ones((B, n)), np.zeros((B, n))
    for s in range(B):
        A[s], zdep[s], _ = O.pixel_terms(params, np.zeros(n), zabs[s], tau_which, tau_series)
    s2n = np.exp(rng.uniform(np.log(snr[0]), np.log(snr[1]), size=B))
    sigma = np.abs(mu)[None, :] / s2n[:, None] * (0.8 + 0.4 * rng.random((B, n)))
    flux = A * (mu[None, :] + rng.standard_normal((B, F.shape[1])) @ F.T + np.sqrt(Psi)[None, :] * rng.standard_normal((B, n)))
    flux[:, :nb] += np.sqrt(om[None, :] * zdep[:, :nb]) * rng.standard_normal((B, nb))
    flux += sigma * rng.standard_normal((B, n))
    mask = np.ones((B, n), dtype=bool)
    if masks:
        for s in range(B):
            st = int(rng.integers(0, n))
            mask[s, st:st + max(2, n // 40)] = False
        mask &= rng.random((B, n)) >= 0.01
    return dict(flux=flux, error=sigma, zabs=zabs, mask=mask, zqso=zq)


def inject(data, wav, lam_nodes, logn_nodes, seed, logn_min=20.7, b_kms=30.0, lyb=True):
    """multiplies every spectrum by a DLA on a grid node (log N_HI >= logn_min); returns float32 flux / error with -999 under the
    mask and the node (i, j) of every spectrum"""
    rng = np.random.default_rng(seed + 1000)
    B = len(data["flux"])
    jj = np.nonzero(np.asarray(logn_nodes) >= logn_min - 1e-9)[0]
    ni, nj = rng.integers(0, len(lam_nodes), size=B), jj[rng.integers(0, len(jj), size=B)]
    flux = data["flux"].copy()
    for s in range(B):
        flux[s] *= transmission(wav, [lam_nodes[ni[s]] / LYA - 1.0], [logn_nodes[nj[s]]], b_kms, lyb)
    m = data["mask"]
    return np.where(m, flux, -999.0).astype(np.float32), np.where(m, data["error"], -999.0).astype(np.float32), ni, nj


# the SDSS case both test files use: the shipped parameters, the grid of synthetic.wavelength_grid(), 33 x 7 candidates
SDSS_GRID = dict(lam_hi=1190.0, dv_kms=1084.0, nz=33, logn_lo=20.0, dlogn=0.2, n_logn=7)
SDSS_SEEDS = (11, 12)
SDSS_B = 17


def sdss_case(shipped, seed):
    """the injected SDSS batch of `seed`, its float64 table and the restatement's scan"""
    from qfa_amd import synthetic
    params, mu = shipped
    wav, nb, _ = synthetic.wavelength_grid()
    g = SDSS_GRID
    lam = centres(g["lam_hi"], g["dv_kms"], g["nz"])
    logn = g["logn_lo"] + np.arange(g["n_logn"]) * g["dlogn"]
    d = draw(params, mu, wav, nb, SDSS_B, seed)
    flux, error, ni, nj = inject(d, wav, lam, logn, seed)
    V = profiles(wav, **g).astype(np.float32)
    llr, nll0, nll = scan(params, mu, flux, error, d["zabs"], d["mask"], V)
    return dict(wav=wav, nb=nb, flux=flux, error=error, zabs=d["zabs"], mask=d["mask"], zqso=d["zqso"], node=ni * g["n_logn"] + nj,
                V=V, llr=llr, nll0=nll0, nll=nll, lam=lam, logn=logn)
