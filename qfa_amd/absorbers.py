"""Catalogued absorbers and bad wavelengths on the device (include/qfa_hip.h ``qfa_absorber_mask_f32`` states the rule).

The stage between ``preprocess`` and everything after it: pixels that a catalogued damped Lyman-alpha system, a sky line (observed
frame, common to all spectra) or a BAL trough (rest frame, per spectrum) has spoiled become the ``-999`` sentinel, which every
kernel of the package treats as weight zero; the rest is divided by the absorbers' Voigt profile.  Catalogue driven: nothing is
found from the data.  Works on any ``(N, Npix)`` rest-frame arrays -- ``preprocess`` output (``Preprocessed.mask_absorbers``) or
data already in the reference's file format."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError

C_KMS = 299792.458
BAL_LINES = (1549.06, 1396.76, 1240.81, 1215.67)        # C IV, Si IV, N V, Ly-alpha
MAX_NPIX = 16384
_I32_FIELDS = ("n_valid", "n_lead", "n_trail", "num_mask", "n_absorber_masked", "n_interval_masked")


class AbsorberCatalog(object):
    """Absorbers per spectrum as a CSR list: ``offsets`` (int64, N + 1), ``z_abs`` and ``log_nhi`` (float64); spectrum i owns the
    entries ``offsets[i] .. offsets[i + 1] - 1``.  Built from per-row lists of ``(z_abs, log_nhi)`` pairs, or from a table keyed by
    file name (``from_table``).  ``unmatched`` lists the table's names that matched no row."""

    def __init__(self, rows, unmatched=()):
        rows = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rows]
        self.offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        both = np.concatenate(rows) if rows else np.zeros((0, 2))
        self.z_abs = np.ascontiguousarray(both[:, 0]) if len(both) else np.zeros(0)
        self.log_nhi = np.ascontiguousarray(both[:, 1]) if len(both) else np.zeros(0)
        self.unmatched = list(unmatched)
        if not (np.all(np.isfinite(self.z_abs)) and np.all(np.isfinite(self.log_nhi))):
            raise QFAHipError("absorber catalogue: z_abs and log_nhi must be finite")
        if np.any(self.z_abs <= -1.0):
            raise QFAHipError("absorber catalogue: 1 + z_abs must be positive")

    def __len__(self):
        return len(self.offsets) - 1

    def row(self, i):
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return np.stack([self.z_abs[a:b], self.log_nhi[a:b]], axis=1)

    def rows(self, lo, hi):
        """the catalogue of the spectra lo .. hi - 1"""
        return AbsorberCatalog([self.row(i) for i in range(lo, hi)])

    @staticmethod
    def _key(name):
        name = str(name)
        return name[:-4] if name.endswith(".npz") else name

    @classmethod
    def from_table(cls, names, table):
        """``names``: the spectra, in row order.  ``table``: a DataFrame or mapping with columns ``file``, ``z_abs``, ``log_nhi``
        (``io.read_absorber_csv``), any number of rows per file, kept in the table's order; a trailing ``.npz`` is ignored on
        both sides.  Rows with no entry get empty lists."""
        files = [cls._key(f) for f in np.asarray(table["file"]).reshape(-1)]
        z, lg = np.asarray(table["z_abs"], dtype=np.float64).reshape(-1), np.asarray(table["log_nhi"], dtype=np.float64).reshape(-1)
        by_file = {}
        for f, a, b in zip(files, z, lg):
            by_file.setdefault(f, []).append((a, b))
        keys = [cls._key(n) for n in names]
        known = set(keys)
        unmatched = [f for f in dict.fromkeys(files) if f not in known]
        return cls([by_file.get(k, []) for k in keys], unmatched)


def bal_intervals(v_min, v_max, lines=BAL_LINES):
    """BAL troughs in km/s of outflow velocity (``v_min < v_max``, scalars or equal-length arrays) to rest-frame intervals
    ``[lam (1 - v_max / c), lam (1 - v_min / c))`` for every line: float64 ``(len(v) len(lines), 2)``, trough-major."""
    v_min, v_max = np.atleast_1d(np.asarray(v_min, dtype=np.float64)), np.atleast_1d(np.asarray(v_max, dtype=np.float64))
    if v_min.shape != v_max.shape or v_min.ndim != 1:
        raise ValueError("v_min and v_max must have one length")
    if not (np.all(np.isfinite(v_min)) and np.all(np.isfinite(v_max)) and np.all(v_min < v_max)):
        raise ValueError("BAL troughs need finite v_min < v_max")
    lam = np.asarray(lines, dtype=np.float64).reshape(-1)
    lo = lam[None, :] * (1.0 - v_max[:, None] / C_KMS)
    hi = lam[None, :] * (1.0 - v_min[:, None] / C_KMS)
    return np.stack([lo, hi], axis=-1).reshape(-1, 2)


def _intervals(x, what):
    iv = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 2))
    if not np.all(np.isfinite(iv)) or np.any(iv[:, 0] >= iv[:, 1]):
        raise QFAHipError(f"{what}: intervals must be finite with lo < hi")
    return iv


def _rest_csr(rest, n):
    """per-spectrum rest-frame intervals: a list of N (., 2) arrays, or (offsets, intervals)"""
    if isinstance(rest, tuple) and len(rest) == 2 and np.ndim(rest[0]) == 1 and len(rest[0]) == n + 1 and np.ndim(rest[1]) == 2:
        off, iv = np.asarray(rest[0]).astype(np.int64), _intervals(rest[1], "rest")
        if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != len(iv):
            raise QFAHipError("rest: offsets must start at 0, be non-decreasing and end at the number of intervals")
        return off, iv
    if len(rest) != n:
        raise QFAHipError(f"rest: {len(rest)} interval lists for {n} spectra")
    parts = [_intervals(r, "rest") for r in rest]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return off, (np.concatenate(parts) if parts else np.zeros((0, 2)))


def _check_params(t_min, b_kms, snr_window):
    if not (0.0 <= float(t_min) < 1.0):
        raise QFAHipError(f"t_min = {t_min}, must lie in [0, 1)")
    if not (float(b_kms) > 0.0 and np.isfinite(float(b_kms))):
        raise QFAHipError(f"b_kms = {b_kms}, must be positive and finite")
    if not (np.isfinite(snr_window[0]) and np.isfinite(snr_window[1]) and snr_window[0] < snr_window[1]):
        raise QFAHipError("snr_window must be finite with lo < hi")


def mask_absorbers(flux, error, zqso, wav_grid, *, dla=None, sky=None, rest=None, t_min=0.8, b_kms=30., lyb=True, correct=True,
                   snr_window=(1270., 1600.), out=None, return_trans=False, device):
    """Mask and correct N spectra on ``wav_grid`` (the rule: include/qfa_hip.h, ``qfa_absorber_mask_f32``).  ``flux``, ``error``
    (N, Npix) float32, ``zqso`` (N): host arrays or device tensors.  ``dla``: an ``AbsorberCatalog`` (or per-row lists of
    ``(z_abs, log_nhi)``); ``sky``: (n, 2) observed-frame intervals ``[lo, hi)`` common to all spectra; ``rest``: per-spectrum
    rest-frame intervals, a list of N (., 2) arrays or ``(offsets, intervals)``.  ``correct=False`` masks only.  ``out`` = (flux,
    error): two (N, Npix) float32 device tensors to fill, which may be the inputs themselves.
    Returns ``(flux, error, record)`` -- or ``(flux, error, trans, record)`` under ``return_trans`` -- with ``record`` a dict of
    device tensors: ``snr`` (float64) and the int32 counts ``n_valid``, ``n_lead``, ``n_trail``, ``num_mask``,
    ``n_absorber_masked``, ``n_interval_masked``.  Raises ``QFAHipError`` on a CPU device (there is no fallback)."""
    from .preprocess import _dev
    device = torch.device(device)
    if device.type != "cuda":
        raise QFAHipError("mask_absorbers needs a HIP device (torch device 'cuda'); qfa_amd has no CPU fallback")
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    npix = len(grid)
    if not 1 <= npix <= MAX_NPIX:
        raise QFAHipError(f"len(wav_grid) = {npix}, supported 1..{MAX_NPIX}")
    _check_params(t_min, b_kms, snr_window)
    f_d, e_d = _dev(flux, torch.float32, device, "flux"), _dev(error, torch.float32, device, "error")
    if f_d.ndim != 2 or f_d.shape[1] != npix or tuple(e_d.shape) != tuple(f_d.shape):
        raise QFAHipError("flux / error must be (N, len(wav_grid))")
    n = int(f_d.shape[0])
    zq = _dev(zqso, torch.float64, device, "zqso").reshape(-1)
    if zq.shape[0] != n:
        raise QFAHipError(f"zqso must be ({n},)")
    dev_of = lambda x: torch.as_tensor(x, device=device)
    a_off = a_z = a_lg = None
    if dla is not None:
        cat = dla if isinstance(dla, AbsorberCatalog) else AbsorberCatalog(dla)
        if len(cat) != n:
            raise QFAHipError(f"dla: a catalogue of {len(cat)} rows for {n} spectra")
        if len(cat.z_abs):
            a_off, a_z, a_lg = dev_of(cat.offsets), dev_of(cat.z_abs), dev_of(cat.log_nhi)
    o_iv, n_obs = None, 0
    if sky is not None:
        iv = _intervals(sky, "sky")
        if len(iv):
            o_iv, n_obs = dev_of(iv), len(iv)
    r_off = r_iv = None
    if rest is not None:
        off, iv = _rest_csr(rest, n)
        if len(iv):
            r_off, r_iv = dev_of(off), dev_of(iv)
    if out is not None:
        fo, eo = out
        for t, name in ((fo, "out[0]"), (eo, "out[1]")):
            _lib.require_device_tensor(t, torch.float32, name)
            if tuple(t.shape) != (n, npix) or t.device != f_d.device:
                raise QFAHipError(f"{name} must be ({n}, {npix}) on {f_d.device}")
    else:
        fo, eo = torch.empty_like(f_d), torch.empty_like(e_d)
    tr = torch.empty((n, npix), dtype=torch.float32, device=device) if return_trans else None
    rf = torch.empty((n, 1), dtype=torch.float64, device=device)
    ri = torch.empty((n, len(_I32_FIELDS)), dtype=torch.int32, device=device)
    q = _lib.AbsorberParams(float(t_min), float(b_kms), float(snr_window[0]), float(snr_window[1]),
                            (_lib.ABS_LYB if lyb else 0) | (_lib.ABS_CORRECT if correct else 0))
    h = _lib.lib()
    wsb = int(h.qfa_absorber_workspace_bytes(n, npix))
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=device)
    g_d = dev_of(grid)
    p = _lib._ptr
    with torch.cuda.device(device):
        _lib.check(h.qfa_absorber_mask_f32(p(f_d), p(e_d), p(zq), p(g_d), n, npix, p(a_off), p(a_z), p(a_lg), p(o_iv), n_obs,
                                           p(r_off), p(r_iv), C.byref(q), p(fo), p(eo), p(tr), p(rf), p(ri), p(ws), wsb,
                                           _lib.current_stream(device)), "qfa_absorber_mask_f32")
    if out is not None:
        for t in out:                                          # written through raw pointers: tell torch
            torch.autograd.graph.increment_version(t)
    record = {name: ri[:, c].contiguous() for c, name in enumerate(_I32_FIELDS)}
    record["snr"] = rf[:, 0].contiguous()
    return (fo, eo, tr, record) if return_trans else (fo, eo, record)
