"""Float64 closed form of the EM update of the factor loadings F (QFA.em_statistics / em_update_F, include/qfa_hip.h
qfa_em_stats_f32 / qfa_em_update_f_f32), in the notation of DESIGN.md sections 2 and 14.

Per spectrum s at the current parameters: wD = mask / D, C = I + sum_i wD A^2 f f^T, y = C^-1 b, E_s = C^-1 + y y^T.  Then
    S2_i = sum_s wD_si A_si^2 E_s      S1_i = sum_s wD_si A_si delta_si y_s      cnt_i = sum_s mask_si
    F_i <- F_i + damping ((S2_i + ridge I)^-1 S1_i - F_i)        rows with cnt_i = 0 stay as they are
and S2_i f_i - S1_i is the exact-mode gradient d(sum_s NLL_s)/df_i (tests/_exact_ref.py).
"""
from __future__ import annotations

import numpy as np

from oracle import qfa_oracle as orc


def em_statistics(params, delta, error, zabs, mask, tau_which="becker", A_blue=None):
    """Batch sums: dict S2 (Npix, Nh, Nh), S1 (Npix, Nh), cnt (Npix,), nll_sum, n, nll (B,)."""
    p = orc._as_params(params, np.float64)
    F = p["F"]
    npix, nh = F.shape
    S2 = np.zeros((npix, nh, nh))
    S1 = np.zeros((npix, nh))
    cnt = np.zeros(npix)
    nlls = np.zeros(len(delta))
    for s in range(len(delta)):
        w = np.asarray(mask[s], dtype=bool)
        A, _, D = orc.pixel_terms(params, error[s], zabs[s], tau_which, 1, np.float64, None if A_blue is None else A_blue[s])
        wD, d, _, C, y, _, nll = orc._lowrank_core(F, A, D, w, np.asarray(delta[s], dtype=np.float64))
        E = np.linalg.inv(C) + np.outer(y, y)
        S2 += (wD * A * A)[:, None, None] * E[None, :, :]
        S1 += (wD * A * d)[:, None] * y[None, :]
        cnt += w
        nlls[s] = nll
    return {"S2": S2, "S1": S1, "cnt": cnt, "nll_sum": float(nlls.sum()), "n": float(len(delta)), "nll": nlls}


def em_update(F, st, ridge=0.0, damping=1.0):
    """(new F, number of rows skipped): rows with cnt = 0 or a system that is not positive definite are kept."""
    F = np.asarray(F, dtype=np.float64)
    out = F.copy()
    nh = F.shape[1]
    skipped = 0
    for i in range(F.shape[0]):
        if not st["cnt"][i] > 0:
            skipped += 1
            continue
        try:
            L = np.linalg.cholesky(st["S2"][i] + ridge * np.eye(nh))
        except np.linalg.LinAlgError:
            skipped += 1
            continue
        x = np.linalg.solve(L.T, np.linalg.solve(L, st["S1"][i]))
        out[i] = F[i] + damping * (x - F[i])
    return out, skipped


def em_step(params, delta, error, zabs, mask, ridge=0.0, damping=1.0, tau_which="becker"):
    """(mean NLL at `params`, params with the updated F, statistics, rows skipped)"""
    st = em_statistics(params, delta, error, zabs, mask, tau_which)
    newF, skipped = em_update(params["F"], st, ridge, damping)
    q = dict(params)
    q["F"] = newF
    return st["nll_sum"] / st["n"], q, st, skipped
