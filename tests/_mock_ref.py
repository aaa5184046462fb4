"""numpy float64 port of the mock-spectrum draw contract of include/qfa_hip.h (qfa_mock_spectra_f32), on top of the Philox /
Box-Muller port in _philox_ref.py.  Test infrastructure only: the library never calls it."""
import numpy as np

import _philox_ref as P

BECKER = (0.751, 1.0 / 4.5, 2.90, -0.132)            # (amp, scale, expo, offset), series 1
SENTINEL = np.float32(-999.0)


def pixel_counters(rows, n_samples, npix):
    """Philox counters (len(rows), S, ceil(npix / 4), 4) uint32 of the pixel stream: (0x80000000 | (p >> 2), s, r lo, r hi)."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    nq = (npix + 3) // 4
    q = (np.arange(nq, dtype=np.uint64) | np.uint64(0x80000000))[None, None, :]
    s = np.arange(n_samples, dtype=np.uint64)[None, :, None]
    r = rows[:, None, None]
    shape = (len(rows), n_samples, nq)
    return np.stack([np.broadcast_to(q, shape), np.broadcast_to(s, shape), np.broadcast_to(r & P.MASK32, shape),
                     np.broadcast_to(r >> np.uint64(32), shape)], axis=-1).astype(np.uint32)


def latent_counters(rows, n_samples, nh):
    """the counters of the latent stream (qfa_sample_latent_f32): first word j >> 2"""
    c = pixel_counters(rows, n_samples, nh)
    c[..., 0] &= np.uint32(0x7FFFFFFF)
    return c


def pixel_normals(seed, rows, n_samples, npix):
    """e (len(rows), S, npix) float32: e[r, s, p] = z[p & 3] of the Philox call of counter (0x80000000 | (p >> 2), s, r)."""
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    x = P.philox4x32_10(pixel_counters(rows, n_samples, npix), key).astype(np.float64)
    u = (x + 0.5) * 2.0 ** -32
    rad0, t0 = np.sqrt(-2.0 * np.log(u[..., 0])), 2 * np.pi * u[..., 1]
    rad1, t1 = np.sqrt(-2.0 * np.log(u[..., 2])), 2 * np.pi * u[..., 3]
    z = np.stack([rad0 * np.cos(t0), rad0 * np.sin(t0), rad1 * np.cos(t1), rad1 * np.sin(t1)], axis=-1)
    return z.reshape(len(rows), n_samples, -1)[..., :npix].astype(np.float32)


def blue_terms(params, zp1, tau=BECKER, A_blue=None):
    """A = exp(-tau(z)) and zdep = (1 - c0 - exp(-tau0 (1 + z)^beta))^2 on the blue side; zp1 = 1 + z (B, Nb) float64."""
    amp, scale, expo, off = tau
    A = np.exp(-(amp * (zp1 * scale) ** expo + off)) if A_blue is None else np.asarray(A_blue, dtype=np.float64)
    tau0, beta, c0 = (float(params[k]) for k in ("tau0", "beta", "c0"))
    return A, (1.0 - c0 - np.exp(-tau0 * zp1 ** beta)) ** 2


def spectra(params, mu, error, zp1, mask, h, seed, row0, tau=BECKER, A_blue=None):
    """The contract in float64 from the float32 inputs.  error (B, Npix), zp1 = 1 + zabs (B, Nb) float64, mask (B, Npix) bool or
    None, h (B, S, Nh).  Returns dict(flux, delta (B, S, Npix) float64, the sentinel under the mask), T = the sum of |terms|
    A (|mu| + sum_j |F h|) + sqrt(D) |e|, e, A (B, Npix), D (B, Npix), use (B, Npix))."""
    F = np.asarray(params["F"], dtype=np.float64)
    Psi = np.asarray(params["Psi"], dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    error = np.asarray(error, dtype=np.float32)
    h = np.asarray(h, dtype=np.float64)
    B, npix = error.shape
    S = h.shape[1]
    nb = 0 if zp1 is None else zp1.shape[1]
    A, zterm = np.ones((B, npix)), np.zeros((B, npix))
    if nb > 0:
        Ab, zd = blue_terms(params, np.asarray(zp1, dtype=np.float64), tau, A_blue)
        A[:, :nb] = Ab
        zterm[:, :nb] = np.asarray(params["omega"], dtype=np.float64)[None, :] * zd
    use = np.ones((B, npix), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    sg = np.where(use, error, np.float32(0)).astype(np.float64)          # what `error` holds under the mask is never used
    D = A * A * Psi[None, :] + zterm + sg * sg
    e = pixel_normals(seed, row0 + np.arange(B), S, npix).astype(np.float64)
    c = mu[None, None, :] + h @ F.T
    cabs = np.abs(mu)[None, None, :] + np.abs(h) @ np.abs(F).T
    sd = np.sqrt(D)[:, None, :]
    flux = A[:, None, :] * c + sd * e
    T = A[:, None, :] * cabs + sd * np.abs(e)
    delta = flux - (mu * A)[:, None, :]
    u3 = np.broadcast_to(use[:, None, :], flux.shape)
    return {"flux": np.where(u3, flux, -999.0), "delta": np.where(u3, delta, -999.0), "T": T, "e": e, "A": A, "D": D, "use": use}
