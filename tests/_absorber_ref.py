"""numpy float64 restatement of the absorber / bad-wavelength masking rule (include/qfa_hip.h, qfa_absorber_mask_f32), written
from the header: the Tepper-Garcia form of the Voigt function with its small-P series and its far wing, the transmission of a
list of absorbers, the pixel decisions, the outputs and the record.  Plain loops over spectra and absorbers; everything is float64
until the outputs are rounded to float32."""
import numpy as np

from _preprocess_ref import run_counts

SENTINEL = np.float32(-999.0)
C_KMS = 299792.458
TAU_COEF = 1.497e-15
LINES = ((1215.67, 0.4164, 6.265e8), (1025.72, 0.07912, 1.897e8))       # lam0, f, Gamma of Ly-alpha, Ly-beta
P_SERIES, P_WING = 0.0625, 750.0
G = (2.0, -4.0, 5.0 / 3.0, 14.0 / 15.0, -8.0 / 5.0, 352.0 / 315.0, -169.0 / 315.0, 38.0 / 189.0, -884.0 / 14175.0,
     2584.0 / 155925.0)


def damping(lam0, gamma, b_kms):
    """a of a line"""
    return gamma * lam0 * 1e-13 / (4.0 * np.pi * b_kms)


def voigt_main(ka, P):
    with np.errstate(all="ignore"):
        H0, Q = np.exp(-P), 1.5 / P
        return H0 - (ka / P) * (H0 * H0 * (4.0 * P * P + 7.0 * P + 4.0 + Q) - Q - 1.0)


def voigt_series(ka, P):
    g = np.zeros_like(P)
    for c in G[::-1]:
        g = g * P + c
    return np.exp(-P) - ka * g


def voigt_h(a, x):
    """H(a, x) of the rule; x an array"""
    ka = a / np.sqrt(np.pi)
    P = np.asarray(x, dtype=np.float64) ** 2
    with np.errstate(all="ignore"):
        wing = (ka / P) * (1.0 + 1.5 / P)
    return np.where(P < P_SERIES, voigt_series(ka, P), np.where(P > P_WING, wing, voigt_main(ka, P)))


def line_x(lam_obs, lam0, z_abs, b_kms):
    return (C_KMS / b_kms) * (lam_obs / (lam0 * (1.0 + z_abs)) - 1.0)


def tau_coef(log_nhi, f, lam0, b_kms):
    return TAU_COEF * 10.0 ** log_nhi * f * lam0 / b_kms


def transmission(lam_obs, z_abs, log_nhi, b_kms=30.0, lyb=True, voigt=voigt_h):
    """T at the observed wavelengths behind the absorbers (z_abs[j], log_nhi[j]) in list order"""
    lam_obs = np.asarray(lam_obs, dtype=np.float64)
    tau = np.zeros_like(lam_obs)
    for za, lg in zip(z_abs, log_nhi):
        for lam0, f, gamma in LINES[:2 if lyb else 1]:
            with np.errstate(all="ignore"):
                tau = tau + tau_coef(lg, f, lam0, b_kms) * voigt(damping(lam0, gamma, b_kms), line_x(lam_obs, lam0, za, b_kms))
    with np.errstate(all="ignore"):
        return np.exp(-tau)


def in_intervals(x, intervals):
    hit = np.zeros(len(x), dtype=bool)
    for lo, hi in np.asarray(intervals, dtype=np.float64).reshape(-1, 2):
        hit |= (x >= lo) & (x < hi)
    return hit


def mask_ref(flux, error, zqso, wav_grid, abs_offsets=None, abs_z=None, abs_lognhi=None, obs=None, rest_offsets=None, rest=None,
             t_min=0.8, b_kms=30.0, lyb=True, correct=True, snr_window=(1270.0, 1600.0)):
    """The outputs of the rule, plus what the tests' bars need: `T` in float64, and per spectrum `snr_abs` (the sum of |terms| of
    the S/N sum) and `n_snr` (their number)."""
    flux, error = np.asarray(flux, dtype=np.float32), np.asarray(error, dtype=np.float32)
    grid = np.asarray(wav_grid, dtype=np.float64)
    N, npix = flux.shape
    out = dict(flux=np.full((N, npix), SENTINEL), error=np.full((N, npix), SENTINEL), trans=np.ones((N, npix), np.float32),
               T=np.ones((N, npix)), snr=np.full(N, np.nan), snr_abs=np.zeros(N), n_snr=np.zeros(N, np.int64),
               valid_in=np.zeros((N, npix), dtype=bool))
    for k in ("n_valid", "n_lead", "n_trail", "num_mask", "n_absorber_masked", "n_interval_masked"):
        out[k] = np.zeros(N, np.int32)
    in_snr = (grid >= snr_window[0]) & (grid < snr_window[1])
    for i in range(N):
        lam = grid * (1.0 + float(zqso[i]))
        za, lg = [], []
        if abs_offsets is not None:
            a, b = int(abs_offsets[i]), int(abs_offsets[i + 1])
            za, lg = abs_z[a:b], abs_lognhi[a:b]
        T = transmission(lam, za, lg, b_kms, lyb)
        valid = (flux[i] != SENTINEL) & (error[i] != SENTINEL)
        with np.errstate(invalid="ignore"):
            m_abs = (T < t_min) | ~np.isfinite(T)
        m_int = np.zeros(npix, dtype=bool)
        if obs is not None:
            m_int |= in_intervals(lam, obs)
        if rest_offsets is not None:
            m_int |= in_intervals(grid, np.asarray(rest).reshape(-1, 2)[int(rest_offsets[i]):int(rest_offsets[i + 1])])
        keep = valid & ~m_abs & ~m_int
        if correct:
            with np.errstate(all="ignore"):
                out["flux"][i, keep] = (flux[i, keep].astype(np.float64) / T[keep]).astype(np.float32)
                out["error"][i, keep] = (error[i, keep].astype(np.float64) / T[keep]).astype(np.float32)
        else:
            out["flux"][i, keep], out["error"][i, keep] = flux[i, keep], error[i, keep]
        with np.errstate(over="ignore"):
            out["trans"][i] = T.astype(np.float32)
        out["T"][i], out["valid_in"][i] = T, valid
        v_out = (out["flux"][i] != SENTINEL) & (out["error"][i] != SENTINEL)
        out["n_valid"][i], out["n_lead"][i], out["n_trail"][i], out["num_mask"][i] = run_counts(v_out)
        out["n_absorber_masked"][i] = int((valid & m_abs).sum())
        out["n_interval_masked"][i] = int((valid & ~m_abs & m_int).sum())
        ssn = sab = np.float64(0.0)
        ns = 0
        for k in np.nonzero(v_out & in_snr)[0]:
            with np.errstate(invalid="ignore"):
                t = np.float64(out["flux"][i, k]) / np.float64(out["error"][i, k])
            ssn, sab, ns = ssn + t, sab + abs(t), ns + 1
        out["snr"][i] = ssn / ns if ns else np.nan
        out["snr_abs"][i], out["n_snr"][i] = sab, ns
    return out


def assert_away_from_threshold(ref, t_min=0.8, tol=1e-9):
    """no absorber decision of the restatement at a valid pixel sits within `tol` of t_min"""
    T = ref["T"][ref["valid_in"]]
    assert not np.any(np.abs(T - t_min) <= tol), "a T sits on t_min: pick another seed"


def voigt_faddeeva(a, x):
    """the Voigt function itself: H(a, x) = Re w(x + i a)"""
    from scipy.special import wofz
    return np.real(wofz(np.asarray(x, dtype=np.float64) + 1j * a))


def accuracy_against_faddeeva(log_nhi, b_kms, lyb=True, t_min=0.8, z_abs=2.5):
    """max |T_rule - T_Faddeeva| over the observed wavelengths where the rule keeps the pixel (T_rule >= t_min), for one absorber
    (Ly-alpha, and Ly-beta under `lyb`): 3400 .. 5200 A in steps of 0.02 A, and 2 000 more points across every step in which T_rule crosses
    t_min, so that the edge of the mask is approached to 1e-5 A.  Returns (max |dT|, the smallest T_rule - t_min reached, points)."""
    lam = np.arange(3400.0, 5200.0, 0.02)
    T = transmission(lam, [z_abs], [log_nhi], b_kms, lyb)
    cross = np.nonzero((T[:-1] >= t_min) != (T[1:] >= t_min))[0]
    lam = np.sort(np.concatenate([lam] + [np.linspace(lam[c], lam[c + 1], 2002)[1:-1] for c in cross]))
    T = transmission(lam, [z_abs], [log_nhi], b_kms, lyb)
    Tw = transmission(lam, [z_abs], [log_nhi], b_kms, lyb, voigt=voigt_faddeeva)
    keep = T >= t_min
    return float(np.max(np.abs(T[keep] - Tw[keep]))), float(np.min(T[keep] - t_min)), int(keep.sum())
