"""The DLA finder on the device (include/qfa_hip.h ``qfa_dla_profiles_f32`` / ``qfa_template_scan_f32`` state the rule).

The stage that produces the catalogue ``mask_absorbers`` applies: every spectrum is scanned over a grid of candidate absorbers
(redshift x column density), the model is multiplied by each candidate's Voigt profile, and the gain in log-likelihood under the
trained continuum model is the statistic (the Gaussian-process finder of Garnett et al. 2017 and Ho, Bird & Garnett 2020).
``DLAFinder`` holds the three methods of ``QFA`` (``dla_profiles``, ``template_scan``, ``dla_scan``); ``DLAScan`` is the result."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError
from .absorbers import AbsorberCatalog, C_KMS

LYA = 1215.67
MAX_NZ, MAX_NLOGN = 4096, 64
f32 = torch.float32


def grid_centres(lam_hi, dv_kms, nz):
    """the rest-frame Ly-alpha centres of the candidate grid, float64 (nz,)"""
    return float(lam_hi) * np.exp(-np.arange(int(nz), dtype=np.float64) * float(dv_kms) / C_KMS)


def check_grid(wav_grid, lam_hi, dv_kms, nz, logn_lo, dlogn, n_logn, b_kms):
    """the bounds of the C check (qfa_dla_profiles_f32), raised as QFAHipError before any device work"""
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    if not (1 <= int(nz) <= MAX_NZ and 1 <= int(n_logn) <= MAX_NLOGN):
        raise QFAHipError(f"nz = {nz}, n_logn = {n_logn}: supported 1..{MAX_NZ}, 1..{MAX_NLOGN}")
    vals = [float(v) for v in (lam_hi, dv_kms, logn_lo, dlogn, b_kms)]
    if not all(np.isfinite(vals)) or not (vals[0] > 0.0 and vals[1] >= 0.0 and vals[4] > 0.0):
        raise QFAHipError("lam_hi > 0, dv_kms >= 0, b_kms > 0 and every grid parameter finite are required")
    lam = grid_centres(lam_hi, dv_kms, nz)
    if len(grid) < 1 or not (grid[0] <= lam[-1] and lam[0] <= grid[-1]):
        raise QFAHipError(f"the candidate centres {lam[-1]:.2f} .. {lam[0]:.2f} must lie inside wav_grid")
    return grid


class DLAScan(object):
    """Result of ``QFA.dla_scan``: ``llr`` (B, nz, n_logn) float32 device tensor, the log-likelihood ratio of every candidate;
    ``nll0`` (B,) the null NLL (``predict``'s ``ll``); ``best_c`` / ``best_llr`` (B,) the kernel's arg-max (the lowest index among
    equals, -1 / NaN if every candidate is NaN); ``zqso`` (B,) float64 numpy; the grid ``lam`` (nz,) and ``log_nhi`` (n_logn,)."""

    def __init__(self, llr, nll0, best_c, best_llr, zqso, lam, log_nhi):
        self.llr, self.nll0, self.best_c, self.best_llr = llr, nll0, best_c, best_llr
        self.zqso = np.asarray(zqso, dtype=np.float64).reshape(-1)
        self.lam, self.log_nhi = np.asarray(lam, dtype=np.float64), np.asarray(log_nhi, dtype=np.float64)
        if tuple(llr.shape) != (len(self.zqso), len(self.lam), len(self.log_nhi)):
            raise QFAHipError(f"llr: shape {tuple(llr.shape)} for {len(self.zqso)} spectra on a {len(self.lam)} x {len(self.log_nhi)} grid")

    def z_abs(self):
        """(B, nz) float64: the absorber redshift of every centre in every spectrum, (1 + z_qso) lam_i / 1215.67 - 1"""
        return (1.0 + self.zqso)[:, None] * self.lam[None, :] / LYA - 1.0

    def best(self):
        """per spectrum ``(z_abs, log_nhi, llr)`` of the arg-max as numpy arrays (NaN where no candidate is finite)"""
        c = self.best_c.cpu().numpy().astype(np.int64)
        ok = c >= 0
        i, j = np.where(ok, c // len(self.log_nhi), 0), np.where(ok, c % len(self.log_nhi), 0)
        z = np.where(ok, self.z_abs()[np.arange(len(c)), i], np.nan)
        return z, np.where(ok, self.log_nhi[j], np.nan), self.best_llr.cpu().numpy().astype(np.float64)

    def log_evidence(self, log_prior_odds=0.0):
        """log of the posterior odds of "one absorber somewhere on the grid" against "none", with a uniform prior over the grid:
        log_prior_odds + logsumexp(llr) - log(nz n_logn), float64 on the device; (B,)"""
        x = self.llr.to(torch.float64).reshape(self.llr.shape[0], -1)
        return torch.logsumexp(x, dim=1) - float(np.log(x.shape[1])) + float(log_prior_odds)

    def to_catalog(self, names=None, min_llr=0.0):
        """An ``AbsorberCatalog`` of the arg-max of every spectrum whose best llr exceeds ``min_llr`` (at most one absorber per
        spectrum), in row order: what ``mask_absorbers`` and ``Preprocessed.mask_absorbers`` take.  ``names`` is kept as
        ``catalog.names`` for ``to_table``."""
        z, lg, v = self.best()
        keep = np.isfinite(v) & (v > float(min_llr))
        cat = AbsorberCatalog([[(z[i], lg[i])] if keep[i] else [] for i in range(len(z))])
        cat.names = None if names is None else [str(n) for n in names]
        cat.llr = v
        return cat

    def to_table(self, names, min_llr=0.0):
        """the candidates as the columns ``io.read_absorber_csv`` reads: dict of ``file``, ``z_abs``, ``log_nhi`` (and ``llr``)"""
        z, lg, v = self.best()
        keep = np.isfinite(v) & (v > float(min_llr))
        names = np.asarray([str(n) for n in names])
        return {"file": names[keep], "z_abs": z[keep], "log_nhi": lg[keep], "llr": v[keep]}

    def arrays(self):
        return {"llr": self.llr.cpu().numpy(), "nll0": self.nll0.cpu().numpy(), "best_c": self.best_c.cpu().numpy(),
                "best_llr": self.best_llr.cpu().numpy(), "zqso": self.zqso, "lam": self.lam, "log_nhi": self.log_nhi}


class DLAFinder(object):
    """the DLA-finder methods of ``QFA`` (model.py)"""

    def dla_profiles(self, wav_grid, *, lam_hi, dv_kms, nz, logn_lo=20.0, dlogn=0.1, n_logn=1, b_kms=30., lyb=True):
        """The template table of the candidate grid, (nz n_logn, Npix) float32 on the device (qfa_dla_profiles_f32): candidate
        ``i n_logn + j`` is an absorber with its Ly-alpha centre at rest-frame ``lam_hi exp(-i dv_kms / c)`` and
        ``log N_HI = logn_lo + j dlogn``."""
        grid = check_grid(wav_grid, lam_hi, dv_kms, nz, logn_lo, dlogn, n_logn, b_kms)
        if len(grid) != self.Npix:
            raise QFAHipError(f"len(wav_grid) = {len(grid)}, the model has {self.Npix} pixels")
        g = torch.as_tensor(grid, device=self.device)
        V = torch.empty((int(nz) * int(n_logn), self.Npix), dtype=f32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().qfa_dla_profiles_f32(C.c_void_p(g.data_ptr()), self.Npix, float(lam_hi), float(dv_kms), int(nz),
                                                       float(logn_lo), float(dlogn), int(n_logn), float(b_kms), 1 if lyb else 0,
                                                       C.c_void_p(V.data_ptr()), _lib.current_stream(self.device)),
                       "qfa_dla_profiles_f32")
        return V

    def template_scan(self, flux=None, error=None, zabs=None, mask=None, templates=None, zfac=None, batch=None):
        """The likelihood-ratio scan of a batch over a table of templates (qfa_template_scan_f32): ``templates`` (nc, Npix) float32
        on the device.  The batch as ``predict`` takes it (raw flux; ``zfac`` = (zq1, pix_ratio); ``batch`` = a ResidentBatch);
        a plain ``zabs`` is read as it is (no automatic factoring: the two forms share one arithmetic).
        Returns ``(llr (B, nc), nll0 (B,), best_c (B,) int32, best_llr (B,))``."""
        if self.mu is None:
            raise QFAHipError("template_scan needs model.mu (load_from_npz or train first)")
        if self._tau_callable is not None:
            raise QFAHipError("template_scan: a custom tau callable has no in-kernel form")
        V = templates
        _lib.require_device_tensor(V, f32, "templates")
        if V.dim() != 2 or V.shape[1] != self.Npix or V.shape[0] < 1:
            raise QFAHipError(f"templates: shape {tuple(V.shape)}, expected (nc >= 1, {self.Npix})")
        nc = int(V.shape[0])
        ps = self._params_struct()
        if batch is not None:
            B = batch.B
            bs, keep = self._batch_struct_rows(batch, raw_flux=True)
        else:
            B = self._check_batch_shapes(flux, error, zabs, mask)
            bs, keep = self._batch_struct(flux, error, zabs, mask, zfac, auto_factor=False)
            if bs.zq1 is not None:
                bs.zabs = None                                  # one form only: the factored pair
        mu = self.mu.to(device=self.device, dtype=f32).contiguous()
        h = _lib.lib()
        need = int(h.qfa_template_scan_workspace_bytes(int(B), self.Npix, self.Nh, nc))
        if need == 0:
            raise QFAHipError(f"template_scan: unsupported shape B={B} Npix={self.Npix} Nh={self.Nh} nc={nc}")
        ws = self._scratch("dla_ws", need)
        dev = self.device
        llr = torch.empty((B, nc), dtype=f32, device=dev)
        nll0 = torch.empty((B,), dtype=f32, device=dev)
        best_c = torch.empty((B,), dtype=torch.int32, device=dev)
        best_llr = torch.empty((B,), dtype=f32, device=dev)
        p = _lib._ptr
        with torch.cuda.device(dev):
            _lib.check(h.qfa_template_scan_f32(C.byref(ps), p(mu), C.byref(bs), C.byref(self._tau_model), p(V), nc, int(B), self.Npix,
                                               self.Nb, self.Nh, p(llr), p(nll0), p(best_c), p(best_llr), p(ws), ws.numel(), 0,
                                               _lib.current_stream(dev)), "qfa_template_scan_f32")
        return llr, nll0, best_c, best_llr

    def dla_scan(self, flux=None, error=None, zabs=None, mask=None, *, zqso, wav_grid, lam_hi, dv_kms, nz, logn_lo=20.0, dlogn=0.1,
                 n_logn=1, b_kms=30., lyb=True, zfac=None, batch=None, templates=None):
        """``dla_profiles`` (or a table made by it, ``templates``) + ``template_scan``; ``zqso`` (B,) gives the candidates their
        redshifts.  Returns a ``DLAScan``."""
        if templates is None:
            templates = self.dla_profiles(wav_grid, lam_hi=lam_hi, dv_kms=dv_kms, nz=nz, logn_lo=logn_lo, dlogn=dlogn, n_logn=n_logn,
                                          b_kms=b_kms, lyb=lyb)
        else:
            check_grid(wav_grid, lam_hi, dv_kms, nz, logn_lo, dlogn, n_logn, b_kms)
        if int(templates.shape[0]) != int(nz) * int(n_logn):
            raise QFAHipError(f"templates: {int(templates.shape[0])} rows for a {nz} x {n_logn} grid")
        llr, nll0, best_c, best_llr = self.template_scan(flux, error, zabs, mask, templates, zfac=zfac, batch=batch)
        zq = zqso.detach().cpu().numpy() if isinstance(zqso, torch.Tensor) else np.asarray(zqso)
        if zq.reshape(-1).shape[0] != llr.shape[0]:
            raise QFAHipError(f"zqso: {zq.reshape(-1).shape[0]} redshifts for {llr.shape[0]} spectra")
        log_nhi = float(logn_lo) + np.arange(int(n_logn), dtype=np.float64) * float(dlogn)
        return DLAScan(llr.view(llr.shape[0], int(nz), int(n_logn)), nll0, best_c, best_llr, zq, grid_centres(lam_hi, dv_kms, nz), log_nhi)
