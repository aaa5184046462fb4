"""The quasar-redshift finder on the device (include/qfa_hip.h ``qfa_redshift_scan_f32`` states the rule).

Every other stage takes the catalogue redshift as exact.  On a rest-frame grid that is uniform in log wavelength a change of the
redshift by one grid step is an integer pixel shift between data and model, so the likelihood of a spectrum under the trained model
can be scanned over ``2 max_shift + 1`` candidate redshifts without interpolation.  ``RedshiftFinder`` holds the two methods of
``QFA`` (``redshift_scan``, ``redshift_catalog``); ``RedshiftScan`` is the result, and its ``z()`` is what a second ``preprocess``
takes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError
from .absorbers import C_KMS

LYA = 1215.67
MAX_SHIFT = 4096
GRID_TOL = 1e-6
LN10 = float(np.log(10.0))
f32 = torch.float32


def check_grid(wav_grid, npix, max_shift):
    """the host-side refusals of a scan, raised as QFAHipError before any device work; returns (grid float64, dloglam): the grid's
    mean log10 step.  A grid whose log steps differ from their mean by more than 1e-6 of it has no exact pixel shift."""
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    m = int(max_shift)
    if len(grid) != int(npix):
        raise QFAHipError(f"len(wav_grid) = {len(grid)}, the model has {npix} pixels")
    if not 0 <= m <= MAX_SHIFT:
        raise QFAHipError(f"max_shift = {max_shift}: supported 0..{MAX_SHIFT}")
    if 2 * m + 1 > len(grid):
        raise QFAHipError(f"max_shift = {m}: 2 max_shift + 1 = {2 * m + 1} candidates need that many pixels, the grid has {len(grid)}")
    if len(grid) < 2:
        raise QFAHipError("wav_grid: at least two pixels are needed to define the grid's step")
    if not np.all(np.isfinite(grid)) or not np.all(grid > 0.0):
        raise QFAHipError("wav_grid must be positive and finite")
    steps = np.diff(np.log10(grid))
    d = float(np.mean(steps))
    if not d > 0.0 or float(np.max(np.abs(steps - d))) > GRID_TOL * d:
        raise QFAHipError("wav_grid is not uniform in log wavelength (steps within 1e-6 of their mean): there is no exact pixel shift")
    return grid, d


def parabola(ym, y0, yp):
    """(offset, sigma) of the parabola through (-1, ym), (0, y0), (1, yp), float64: the vertex and 1 / sqrt(-curvature); NaN where the
    curvature is not negative -- the kernel's rule (k_zscan_best)"""
    ym, y0, yp = (np.asarray(v, dtype=np.float64) for v in (ym, y0, yp))
    cv = (ym - y0) + (yp - y0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = cv < 0.0
        off = np.where(ok, 0.5 * (ym - yp) / np.where(ok, cv, -1.0), np.nan)
        sig = np.where(ok, 1.0 / np.sqrt(np.where(ok, -cv, 1.0)), np.nan)
    return off, sig


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)



class RedshiftScan(object):
    """Result of ``QFA.redshift_scan``: ``llr`` (B, 2 m + 1) float32, NLL_0 - NLL_s of candidate ``s = column - m`` (data pixel p is
    model pixel p + s); ``nll0`` (B,) the NLL at the catalogue redshift over the window; ``best_s`` (B,) int32 and ``best_llr`` (B,)
    the kernel's arg-max; ``offset`` / ``sigma_pix`` (B,) float64 the parabola's vertex relative to ``best_s`` and its width in
    pixels (NaN at the edges); ``zqso`` (B,) float64 numpy, the catalogue redshifts; ``dloglam`` the grid's log10 step.  The tensors
    are device tensors as the scan returns them (numpy arrays serve as well)."""

    def __init__(self, llr, nll0, best_s, best_llr, offset, sigma_pix, zqso, dloglam):
        self.llr, self.nll0, self.best_s, self.best_llr, self.offset, self.sigma_pix = llr, nll0, best_s, best_llr, offset, sigma_pix
        self.zqso = np.asarray(_np(zqso), dtype=np.float64).reshape(-1)
        self.dloglam = float(dloglam)
        self.names = None
        if len(llr.shape) != 2 or llr.shape[0] != len(self.zqso) or llr.shape[1] % 2 != 1:
            raise QFAHipError(f"llr: shape {tuple(llr.shape)} for {len(self.zqso)} spectra (an odd number of candidates is expected)")

    @property
    def max_shift(self):
        return (int(self.llr.shape[1]) - 1) // 2

    def shift(self):
        """(B,) float64: best_s + offset in pixels, best_s alone where the offset is NaN"""
        s, o = _np(self.best_s).astype(np.float64), _np(self.offset).astype(np.float64)
        return s + np.where(np.isfinite(o), o, 0.0)

    def z(self):
        """(B,) float64: (1 + z_cat) 10^(-shift dloglam) - 1"""
        return (1.0 + self.zqso) * 10.0 ** (-self.shift() * self.dloglam) - 1.0

    def dv_kms(self):
        """(B,) float64: the velocity offset of the refined redshift, -shift dloglam ln(10) c"""
        return -self.shift() * self.dloglam * LN10 * C_KMS

    def sigma_z(self):
        """(B,) float64: the redshift error from the parabola's width, (1 + z) ln(10) dloglam sigma_pix"""
        return (1.0 + self.z()) * LN10 * self.dloglam * _np(self.sigma_pix).astype(np.float64)

    def sigma_kms(self):
        return _np(self.sigma_pix).astype(np.float64) * self.dloglam * LN10 * C_KMS

    def at_edge(self):
        """(B,) bool: the best candidate is the first or the last of the scan (the true shift may lie outside it)"""
        m = self.max_shift
        return np.abs(_np(self.best_s).astype(np.int64)) == m if m > 0 else np.ones(len(self.zqso), dtype=bool)

    def log_evidence(self):
        """logsumexp(llr) - log(n_s), float64 (B,): the log of the evidence ratio of "some shift of the scan" against the catalogue
        redshift under a flat prior over the candidates"""
        x = self.llr if isinstance(self.llr, torch.Tensor) else torch.as_tensor(np.asarray(self.llr))
        x = x.to(torch.float64)
        return torch.logsumexp(x, dim=1) - float(np.log(x.shape[1]))

    def to_table(self, names=None):
        """the catalogue columns ``io.write_redshift_csv`` takes, one row per spectrum"""
        names = self.names if names is None else names
        if names is None or len(names) != len(self.zqso):
            raise QFAHipError(f"to_table: {0 if names is None else len(names)} names for {len(self.zqso)} spectra")
        return {"file": np.asarray([str(n) for n in names]), "z_cat": self.zqso, "z": self.z(), "sigma_z": self.sigma_z(),
                "dv_kms": self.dv_kms(), "sigma_kms": self.sigma_kms(), "best_s": _np(self.best_s).astype(np.int64),
                "offset": _np(self.offset).astype(np.float64), "best_llr": _np(self.best_llr).astype(np.float64),
                "at_edge": self.at_edge().astype(np.int64)}

    def arrays(self):
        """what redshift_scan.npz holds"""
        return {"llr": _np(self.llr), "nll0": _np(self.nll0), "best_s": _np(self.best_s), "best_llr": _np(self.best_llr),
                "offset": _np(self.offset), "sigma_pix": _np(self.sigma_pix), "zqso": self.zqso, "dloglam": np.float64(self.dloglam),
                "z": self.z()}

    @classmethod
    def concat(cls, scans):
        """the scans of consecutive slices as one"""
        cat = lambda name: torch.cat([getattr(s, name) for s in scans], dim=0)
        return cls(cat("llr"), cat("nll0"), cat("best_s"), cat("best_llr"), cat("offset"), cat("sigma_pix"),
                   np.concatenate([s.zqso for s in scans]), scans[0].dloglam)


class RedshiftFinder(object):
    """the redshift-finder methods of ``QFA`` (model.py)"""

    def redshift_scan(self, flux=None, error=None, mask=None, *, zqso, wav_grid, max_shift, batch=None):
        """The likelihood of every spectrum at the pixel shifts ``-max_shift .. max_shift`` (qfa_redshift_scan_f32).  The batch as
        raw flux, error and mask (B, Npix), or ``batch`` = a ResidentBatch; ``zqso`` (B,) the catalogue redshifts; ``wav_grid``
        (Npix,) the rest-frame grid, uniform in log wavelength.  Returns a ``RedshiftScan``."""
        if self.mu is None:
            raise QFAHipError("redshift_scan needs model.mu (load_from_npz or train first)")
        if self._tau_callable is not None:
            raise QFAHipError("redshift_scan: a custom tau callable has no in-kernel form")
        grid, dloglam = check_grid(wav_grid, self.Npix, max_shift)
        m = int(max_shift)
        zq = np.asarray(_np(zqso), dtype=np.float64).reshape(-1)
        B = int(batch.B) if batch is not None else (int(flux.shape[0]) if isinstance(flux, torch.Tensor) and flux.dim() == 2 else -1)
        if len(zq) != B:
            raise QFAHipError(f"zqso: {len(zq)} redshifts for {B} spectra")
        if B < 1:
            raise QFAHipError("redshift_scan: an empty batch")
        dev = self.device
        ps = self._params_struct()
        if batch is not None:
            bs, keep = self._batch_struct_rows(batch, raw_flux=True)
            if self.Nb > 0 and bs.zq1 is None:
                raise QFAHipError("redshift_scan: the resident batch must carry zq1 (the factored-z form)")
        else:
            for t, name in ((flux, "flux"), (error, "error"), (mask, "mask")):
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, self.Npix):
                    raise QFAHipError(f"{name}: expected a ({B}, {self.Npix}) tensor")
            bs, keep = self._flux_batch(flux, error, mask)
            bs.zabs = bs.A_blue = bs.zq1 = bs.pix_ratio = None
        ratio = torch.as_tensor((grid / LYA).astype(np.float32), device=dev)
        if batch is None and self.Nb > 0:
            zq1 = torch.as_tensor((1.0 + zq).astype(np.float32), device=dev)
            keep.append(zq1)
            bs.zq1, bs.pix_ratio = zq1.data_ptr(), ratio.data_ptr()
        mu = self.mu.to(device=dev, dtype=f32).contiguous()
        h = _lib.lib()
        need = int(h.qfa_zscan_workspace_bytes(B, self.Npix, self.Nh, m))
        if need == 0:
            raise QFAHipError(f"redshift_scan: unsupported shape B={B} Npix={self.Npix} Nh={self.Nh} max_shift={m}")
        ws = self._scratch("zscan_ws", need)
        ns = 2 * m + 1
        llr = torch.empty((B, ns), dtype=f32, device=dev)
        nll0 = torch.empty((B,), dtype=f32, device=dev)
        best_s = torch.empty((B,), dtype=torch.int32, device=dev)
        best_llr = torch.empty((B,), dtype=f32, device=dev)
        off = torch.empty((B,), dtype=torch.float64, device=dev)
        sig = torch.empty((B,), dtype=torch.float64, device=dev)
        p = _lib._ptr
        with torch.cuda.device(dev):
            _lib.check(h.qfa_redshift_scan_f32(C.byref(ps), p(mu), C.byref(bs), C.byref(self._tau_model), p(ratio), m, B, self.Npix,
                                               self.Nb, self.Nh, p(llr), p(nll0), p(best_s), p(best_llr), p(off), p(sig), p(ws),
                                               ws.numel(), 0, _lib.current_stream(dev)), "qfa_redshift_scan_f32")
        del keep
        return RedshiftScan(llr, nll0, best_s, best_llr, off, sig, zq, dloglam)

    def redshift_catalog(self, dataloader, max_shift, batch_size=4096):
        """``redshift_scan`` of a whole dataloader: one ``RedshiftScan`` of all its spectra in loader order (a spectrum's row depends
        on that spectrum alone, so the result does not depend on ``batch_size``).  It walks the loader as ``bal_catalog`` does (the
        resident rows form when the loader has one).  Under data parallelism every rank scans its own shard, as ``dla_scan`` does.
        ``names`` of the result: the loader's paths in row order."""
        if not hasattr(dataloader, "wav_grid") or not hasattr(dataloader, "zqso"):
            raise QFAHipError("redshift_catalog: the dataloader must carry wav_grid and zqso (a DeviceDataloader)")
        zq_all = np.asarray(dataloader.zqso, dtype=np.float64).reshape(-1)
        scans, names = [], []
        for s, inputs, paths in self._loader_slices(dataloader, int(batch_size)):
            names += list(paths)
            inp = {k: v for k, v in inputs.items() if k != "zabs"}
            n = inp["batch"].B if "batch" in inp else int(inp["flux"].shape[0])
            scans.append(self.redshift_scan(**inp, zqso=zq_all[s:s + n], wav_grid=dataloader.wav_grid, max_shift=max_shift))
        if not scans:
            raise QFAHipError("redshift_catalog: the dataloader is empty")
        scan = RedshiftScan.concat(scans)
        scan.names = [str(x) for x in names]
        return scan
