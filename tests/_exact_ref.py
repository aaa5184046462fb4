"""Float64 closed form of the exact gradient mode (QFA.exact_gradients, include/qfa_hip.h QFA_F_EXACT_GRAD).

The gradient of the loss the step reports, loss = sum_s NLL_s / B, in the low-rank form of DESIGN.md section 2, with the
reference's mask semantics (a masked pixel has zero weight: it is left out of Sigma).  Per spectrum, with M = diag(A) F,
C = I + M^T D^-1 M, y = C^-1 b, u = Sigma^-1 delta, dG = (diag(Sigma^-1) - u^2) / 2:

    gF_i   = wD_i A_i^2 f_i^T C^-1 - A_i u_i y^T
    gPsi_i = A_i^2 dG_i                 gOmega_i = dG_i zd_i
    r = 1 - c0 - exp(-t),  t = tau0 (1+z)^beta,  zd = r^2,  e' = dG omega 2 r          (blue pixels)
    g_tau0 = sum e' exp(-t) (1+z)^beta    g_beta = sum e' exp(-t) t ln(1+z)    g_c0 = -sum e'

The batch gradient is the sum over spectra divided by B; an element no spectrum observes gets 0.
"""
from __future__ import annotations

import numpy as np

from oracle import qfa_oracle as orc


def exact_single(params, delta, error, zabs, mask, tau_which="becker", A_blue=None, tau_series=1):
    """One spectrum: (nll, grads, absum) -- raw (un-normalised) exact gradients and, for the scalar sums, the sum of the
    absolute values of their terms (the scale a float32 implementation is judged against)."""
    p = orc._as_params(params, np.float64)
    F = p["F"]
    Nb = p["omega"].shape[0]
    w = np.asarray(mask, dtype=bool)
    A, zdep, D = orc.pixel_terms(params, error, zabs, tau_which, tau_series, np.float64, A_blue)
    wD, d, M, C, y, u, nll = orc._lowrank_core(F, A, D, w, np.asarray(delta, dtype=np.float64))
    Cinv = np.linalg.inv(C)
    q = np.einsum("ia,ab,ib->i", F, Cinv, F)
    dS = wD - (wD * A) ** 2 * q
    dG = np.where(w, 0.5 * (dS - u * u), 0.0)
    gF = (wD * A * A)[:, None] * (F @ Cinv) - (A * u)[:, None] * y[None, :]
    gPsi = A * A * dG
    gOm = dG[:Nb] * zdep[:Nb]
    z = np.asarray(zabs, dtype=np.float64)
    t = p["tau0"] * (1.0 + z) ** p["beta"]
    ex = np.exp(-t)
    r = 1.0 - p["c0"] - ex
    e = dG[:Nb] * p["omega"] * 2.0 * r
    term_tau0 = e * ex * (1.0 + z) ** p["beta"]
    term_beta = e * ex * t * np.log(1.0 + z)
    grads = {"F": gF, "Psi": gPsi, "omega": gOm, "tau0": np.float64(term_tau0.sum()),
             "c0": np.float64(-e.sum()), "beta": np.float64(term_beta.sum())}
    absum = {"tau0": float(np.abs(term_tau0).sum()), "c0": float(np.abs(e).sum()), "beta": float(np.abs(term_beta).sum())}
    return nll, grads, absum


def exact_forward(params, delta, error, zabs, mask, tau_which="becker", A_blue=None, normalize=True, tau_series=1):
    """Batch: (loss, grads, absum).  loss = mean NLL; grads = sum over spectra / B (normalize=False: the raw sums);
    absum: the scalar terms' sum of absolute values over the batch, divided likewise."""
    B = len(delta)
    sums, absum, loss = None, {"tau0": 0.0, "c0": 0.0, "beta": 0.0}, 0.0
    for s in range(B):
        nll, g, a = exact_single(params, delta[s], error[s], zabs[s], mask[s], tau_which,
                                 None if A_blue is None else A_blue[s], tau_series)
        loss += nll
        sums = {k: np.array(v, dtype=np.float64) for k, v in g.items()} if sums is None else \
            {k: sums[k] + g[k] for k in sums}
        for k in absum:
            absum[k] += a[k]
    n = float(B) if normalize else 1.0
    return loss / B, {k: v / n for k, v in sums.items()}, {k: v / n for k, v in absum.items()}
