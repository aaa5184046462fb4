"""References for the helper and optimiser entry points (tests/test_helper_kernels.py, tests/test_helper_ref_cpu.py): plain
numpy, no torch.

What the oracle already states is imported, not restated.  Three references are added:

* ``adam_f32``     the update of include/qfa_hip.h (qfa_adam_clip_f32) with EVERY operation in np.float32 -- the reference's own
                   float32 arithmetic (QFA/optimizer.py:47-52 on float32 tensors, QFA/model.py:237-241).  What it differs from
                   float64 by is the unit the kernels' error is measured in.
* ``finalize_ref`` qfa_finalize_grads_f32 in float64, the three modes of scalar slot 6 (include/qfa_hip.h, qfa_accum_floats).
* ``zfactor_ref``  qfa_zabs_factor_f32 with the header's float32 operations.

The case builders at the end are shared by the CPU pins and the GPU tests, so that both look at the same numbers.
"""
from __future__ import annotations

import numpy as np

from oracle import qfa_oracle as O

edge_mean = O._edge_mean
clip_params = O.clip_params
adam_update = O.adam_update
woodbury_inverse = O.woodbury_inverse
woodbury_logdet = O.woodbury_logdet
boxcar_reflect = O.boxcar_reflect
mu_estimate = O.mu_estimate
delta_from_flux = O.delta_from_flux
zabs_from_zqso = O.zabs_from_zqso
tau_eff = O.tau_eff
tau_hi = O.tau_hi
omega_zdep = O.omega_zdep

f32 = np.float32


def ulp32(x):
    """Spacing of float32 at |x| (float64 array): the unit of the 'n ulp' bars."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(f32)).astype(np.float64)


def adam_f32(p, g, m, v, lr, b1, b2, eps, wd, i, lo, hi):
    """(p_out, m_new, v_new), every operation rounded to float32, in the order of include/qfa_hip.h.  The scalars are formed
    in double and rounded once, where a Python float meets a float32 tensor in the reference: (float)(1 - b1),
    (float)(1 - b1^(i+1)), ...  lo > hi: no clamp."""
    p, g, m, v = (np.asarray(x, dtype=f32) for x in (p, g, m, v))
    lr_, b1_, b2_, eps_, wd_ = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
    bc1, bc2 = f32(1.0 - b1 ** (i + 1)), f32(1.0 - b2 ** (i + 1))
    with np.errstate(all="ignore"):
        gi = g + wd_ * p
        mi = omb1 * gi + b1_ * m
        vi = omb2 * gi * gi + b2_ * v
        q = p - lr_ * (mi / bc1) / (np.sqrt(vi / bc2) + eps_)
        if lo <= hi:
            q = np.where(q < f32(lo), f32(lo), np.where(q > f32(hi), f32(hi), q))
    for x in (gi, mi, vi, q):
        assert x.dtype == f32
    return q.astype(f32), mi, vi


def adam_f64(p, g, m, v, lr, b1, b2, eps, wd, i, lo, hi):
    """The same update through the oracle's float64 ``adam_update`` (+ np.clip): (p_out, m_new, v_new)."""
    with np.errstate(all="ignore"):
        newp, newm, newv = O.adam_update({"x": m}, {"x": v}, i, {"x": p}, {"x": g}, lr, b1, b2, eps, wd)
    q = newp["x"]
    if lo <= hi:
        q = np.clip(q, float(f32(lo)), float(f32(hi)))
    return q, newm["x"], newv["x"]


def accum_layout(Npix, Nb, Nh):
    """Slices of the packed buffer [accF Npix*Nh | sumA Npix | gPsi Npix | gOmega Nb | cnt Npix | 8 scalars]."""
    o, out = 0, {}
    for name, n in (("F", Npix * Nh), ("A", Npix), ("Psi", Npix), ("omega", Nb), ("cnt", Npix), ("S", 8)):
        out[name] = slice(o, o + n)
        o += n
    return out, o


def finalize_ref(accum, F, Npix, Nb, Nh, normalize):
    """float64 dict {F, Psi, omega, tau0, c0, beta, loss} of qfa_finalize_grads_f32.  Slot 6 of the scalars selects the mode:
    0 = the reference's (sum / count, 0/0 = NaN; scalars / n_spectra_with_blue), = slot 5 = exact (gF = -accF, everything
    / n_spectra), anything else = mixed: NaN everywhere, the loss included.  normalize = 0: the raw sums."""
    a = np.asarray(accum, dtype=np.float64)
    sl, tot = accum_layout(Npix, Nb, Nh)
    assert a.shape == (tot,)
    accF, accA, accPsi, accOm, cnt, S = (a[sl[k]] for k in ("F", "A", "Psi", "omega", "cnt", "S"))
    accF = accF.reshape(Npix, Nh)
    F = np.asarray(F, dtype=np.float64).reshape(Npix, Nh)
    with np.errstate(all="ignore"):
        loss = S[4] / S[5] if normalize else S[4]
        if S[6] == 0.0:
            gF = F * accA[:, None] - accF
            gPsi, gOm, sc = accPsi.copy(), accOm.copy(), S[:3].copy()
            if normalize:
                gF, gPsi, gOm, sc = gF / cnt[:, None], gPsi / cnt, gOm / cnt[:Nb], sc / S[3]
        else:
            n = S[5] if normalize else 1.0
            gF, gPsi, gOm, sc = -accF / n, accPsi / n, accOm / n, S[:3] / n
            if S[6] != S[5]:
                gF, gPsi, gOm, sc, loss = (np.full_like(x, np.nan) for x in (gF, gPsi, gOm, sc, np.asarray(loss)))
    return {"F": gF, "Psi": gPsi, "omega": gOm, "tau0": np.asarray(sc[0]), "c0": np.asarray(sc[1]), "beta": np.asarray(sc[2]),
            "loss": np.asarray(loss)}


def zfactor_ref(zabs, tol):
    """(zq1 (B,), pix_ratio (Nb,), nbad) of qfa_zabs_factor_f32: zq1 = 1 + zabs[:, 0] in float32; pix_ratio = (1 + zabs[0]) /
    (1 + zabs[0, 0]) in float64, rounded once; nbad counts |(1 + z) - zq1 pix_ratio| > tol (1 + z) in float32, a NaN counts."""
    z = np.asarray(zabs, dtype=f32)
    with np.errstate(all="ignore"):
        zq1 = f32(1.0) + z[:, 0]
        ratio = ((1.0 + z[0].astype(np.float64)) / (1.0 + np.float64(z[0, 0]))).astype(f32)
        a = f32(1.0) + z
        d = a - zq1[:, None] * ratio[None, :]
        nbad = int(np.sum(~(np.abs(d) <= f32(tol) * a)))
    assert a.dtype == f32 and d.dtype == f32
    return zq1, ratio, nbad


def zfactor_margin(zabs, tol):
    """Smallest | |d| / (tol a) - 1 | over the elements, d formed exactly (float64): the compiler may contract a - zq1 ratio
    into one fma, which moves d by half a float32 ulp of the product; a count is only comparable when no element sits that
    close to the threshold."""
    z = np.asarray(zabs, dtype=f32).astype(np.float64)
    zq1, ratio, _ = zfactor_ref(zabs, tol)
    with np.errstate(all="ignore"):
        a = 1.0 + z
        r = np.abs(a - zq1.astype(np.float64)[:, None] * ratio.astype(np.float64)[None, :]) / (float(f32(tol)) * a)
    r = r[np.isfinite(r)]
    return float(np.min(np.abs(r - 1.0))) if r.size else np.inf


# ------------------------------------------------------------------------------------------------ shared cases
WOODBURY_SHAPES = [(1, 1), (5, 1), (7, 3), (33, 17), (40, 32), (300, 32), (1100, 8)]


def woodbury_case(n, k):
    """M ~ N(0, 1) rounded to float32, D log-uniform in 1e-3 .. 1e2; the dense float64 inverse and log-determinant of
    M M^T + diag D built from the float32 inputs."""
    rng = np.random.default_rng(1000 * n + k)
    M = rng.standard_normal((n, k)).astype(f32)
    D = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), n)).astype(f32)
    S = M.astype(np.float64) @ M.astype(np.float64).T + np.diag(D.astype(np.float64))
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    return M, D, np.linalg.inv(S), float(logdet)


def adam_case(n, seed, special=True):
    """One tensor of an Adam case: p, g, m, v float32 with non-zero optimiser state.  |g| in 0.5 .. 2 with the sign of m, and
    |p| in 0.2 .. 1.5, so that neither g + wd p nor (1-b1) g + b1 m cancels: every float32 evaluation order then stays within a
    few ulp of the float64 value and the elementwise bar compares roundings, not conditioning.  special: element n // 3 of g is
    NaN and element (2 n) // 3 is 1e20 (n >= 3; n = 2 gets both, n = 1 the 1e20 for odd seeds and the NaN for even ones)."""
    rng = np.random.default_rng(seed)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = (sgn * rng.uniform(0.5, 2.0, n)).astype(f32)
    m = (sgn * rng.uniform(0.01, 0.5, n)).astype(f32)
    v = rng.uniform(0.01, 2.0, n).astype(f32)
    p = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.2, 1.5, n)).astype(f32)
    if special and n >= 2:
        g[n // 3] = np.nan
        g[(2 * n) // 3 if n >= 3 else 1] = 1e20
    elif special and n == 1:
        g[0] = 1e20 if seed % 2 else np.nan
    return p, g, m, v
