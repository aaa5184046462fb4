"""The BAL finder: balnicity index, absorption index and trough velocities per spectrum under the model's posterior continuum
(include/qfa_hip.h, ``qfa_bal_scan_f32`` and ``qfa_bal_mask_f32`` state the rules).

``mask_absorbers(rest=...)`` takes per-spectrum rest-frame intervals -- what BAL troughs are -- and ``absorbers.bal_intervals`` makes
them from trough velocities; this module measures the troughs.  ``QFA.bal_scan`` forms r = flux / continuum on the red side for every
draw of the continuum, finds the runs of r below ``thr`` in the velocity window of every line and integrates them into the indices
(BI: Weymann et al. 1991; AI: Hall et al. 2002, Trump et al. 2006); ``BALScan.to_intervals`` hands the troughs to ``mask_absorbers``.
A BAL quasar's continuum is biased low by its own troughs until they are masked: ``n_iter`` > 1 repeats predict -> scan -> mask with
the mask made on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError, _ptr
from .absorbers import BAL_LINES, C_KMS, bal_intervals

f32 = torch.float32
DEFAULT_LINES = (1549.06, 1396.76)                      # C IV, Si IV
DEFAULT_INDICES = {"BI": (3000.0, 25000.0, 2000.0, "after"), "AI": (0.0, 25000.0, 450.0, "whole")}


def check_indices(indices):
    """{name: (v_lo, v_hi, w_min, mode)} as given or the default BI / AI, checked: an ordered dict of 1..4 definitions"""
    ind = dict(DEFAULT_INDICES if indices is None else indices)
    if not 1 <= len(ind) <= _lib.BAL_MAX_INDICES:
        raise QFAHipError(f"indices: {len(ind)} definitions, supported 1..{_lib.BAL_MAX_INDICES}")
    out = {}
    for name, d in ind.items():
        try:
            v_lo, v_hi, w_min, mode = float(d[0]), float(d[1]), float(d[2]), str(d[3]).lower()
        except (TypeError, IndexError, ValueError) as e:
            raise QFAHipError(f"index {name!r}: expected (v_lo, v_hi, w_min, 'whole' | 'after')") from e
        if mode not in _lib.BAL_MODES or not (np.isfinite([v_lo, v_hi, w_min]).all() and v_lo < v_hi and w_min >= 0.0):
            raise QFAHipError(f"index {name!r}: {d}: needs finite v_lo < v_hi, w_min >= 0 and mode 'whole' or 'after'")
        out[str(name)] = (v_lo, v_hi, w_min, mode)
    return out


def check_scan_params(lines, thr, smooth, max_gap):
    lines = tuple(float(x) for x in np.atleast_1d(np.asarray(lines, dtype=np.float64)))
    if not 1 <= len(lines) <= _lib.BAL_MAX_LINES:
        raise QFAHipError(f"lines: {len(lines)} lines, supported 1..{_lib.BAL_MAX_LINES}")
    if not all(np.isfinite(x) and x > 0.0 for x in lines):
        raise QFAHipError("lines must be positive and finite")
    if not (float(thr) > 0.0 and np.isfinite(float(thr))):
        raise QFAHipError(f"thr = {thr}, must be positive and finite")
    if int(smooth) != smooth or not 1 <= int(smooth) <= 15 or int(smooth) % 2 == 0:
        raise QFAHipError(f"smooth = {smooth}, expected an odd width 1..15")
    if int(max_gap) != max_gap or not 0 <= int(max_gap) <= 16:
        raise QFAHipError(f"max_gap = {max_gap}, expected 0..16")
    return lines


def velocity_window(wav_grid, line, v_lo, v_hi, Nb=0):
    """``(p_lo, p_hi, vedge)`` of one line: the pixels p >= Nb whose velocity span overlaps (v_lo, v_hi) and the float64 edge table
    (p_hi - p_lo + 1) the kernel reads, window pixel i = pixel p_hi - 1 - i.  v = C_KMS (1 - wav / line) at the pixel centres; an
    edge is the mean of the two centres beside it, at the grid's ends the centre plus or minus half the step to its only neighbour.
    Raises if the window reaches into the model's blue side (0 < Nb), where the continuum needs a transmission model."""
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    if len(grid) < 2 or not (np.all(np.isfinite(grid)) and np.all(grid > 0.0) and np.all(np.diff(grid) > 0.0)):
        raise QFAHipError("wav_grid must hold at least two finite, positive, increasing wavelengths")
    v = C_KMS * (1.0 - grid / float(line))                         # falls with p
    mid = (v[1:] + v[:-1]) / 2.0
    upper = np.concatenate([[v[0] + (v[0] - v[1]) / 2.0], mid])    # the pixel's edge at higher velocity
    lower = np.concatenate([mid, [v[-1] - (v[-2] - v[-1]) / 2.0]])
    inside = np.nonzero((upper > float(v_lo)) & (lower < float(v_hi)))[0]
    if len(inside) == 0:
        return int(Nb), int(Nb), np.zeros(1, dtype=np.float64)
    p_lo, p_hi = int(inside[0]), int(inside[-1]) + 1
    if p_lo < int(Nb):
        raise QFAHipError(f"line {line}: the window ({v_lo}, {v_hi}) km/s reaches pixel {p_lo} on the blue side of the model "
                          f"(Nb = {Nb}): the continuum there needs a transmission model")
    if p_hi - p_lo > _lib.BAL_MAX_WIN:
        raise QFAHipError(f"line {line}: a window of {p_hi - p_lo} pixels, the limit is {_lib.BAL_MAX_WIN}")
    vedge = np.concatenate([lower[p_lo:p_hi][::-1], [upper[p_lo]]])
    return p_lo, p_hi, np.ascontiguousarray(vedge, dtype=np.float64)


class BALScan(object):
    """Result of ``QFA.bal_scan``.  Device tensors: ``value``, ``var`` (B, S, L, I) float64, ``n_pix``, ``n_runs``, ``n_bridged``
    (B, S, L, I) int32, ``n_used``, ``n_troughs`` (B, S, L) int32, ``troughs`` (B, S, L, 8, 2) float64 [v_min, v_max] in km/s, NaN
    where unfilled; ``lines`` (L,) in Angstrom, ``index_names`` (I,), ``indices`` their definitions, ``trough_index`` the index whose
    qualifying runs are the troughs.  After ``n_iter`` > 1: ``mask`` the mask of the last predict and ``n_masked`` (B,) the pixels it
    lacks."""

    def __init__(self, value, var, counts, line_counts, troughs, lines, indices, trough_index, thr, mask=None, n_masked=None):
        self.value, self.var, self.counts, self.line_counts, self.troughs = value, var, counts, line_counts, troughs
        self.lines = tuple(float(x) for x in lines)
        self.indices = dict(indices)
        self.index_names = tuple(self.indices)
        self.trough_index, self.thr = str(trough_index), float(thr)
        self.mask, self.n_masked = mask, n_masked
        B, S, L, I = value.shape
        if L != len(self.lines) or I != len(self.index_names) or tuple(troughs.shape) != (B, S, L, _lib.BAL_MAX_TROUGHS, 2) \
                or tuple(counts.shape) != (B, S, L, I, 3) or tuple(line_counts.shape) != (B, S, L, 2) or tuple(var.shape) != (B, S, L, I):
            raise QFAHipError("BALScan: inconsistent shapes")

    n_pix = property(lambda self: self.counts[..., 0])
    n_runs = property(lambda self: self.counts[..., 1])
    n_bridged = property(lambda self: self.counts[..., 2])
    n_used = property(lambda self: self.line_counts[..., 0])
    n_troughs = property(lambda self: self.line_counts[..., 1])
    B = property(lambda self: int(self.value.shape[0]))
    S = property(lambda self: int(self.value.shape[1]))

    def _index(self, name):
        if name not in self.index_names:
            raise QFAHipError(f"no index {name!r} in this scan: {self.index_names}")
        return self.index_names.index(name)

    def index(self, name):
        """(B, S, L) the values of the index ``name``, km/s"""
        return self.value[..., self._index(name)]

    def bi(self):
        return self.index("BI")

    def ai(self):
        return self.index("AI")

    def err(self, name=None):
        """the noise error sqrt(var): (B, S, L, I), or (B, S, L) of the index ``name``"""
        e = torch.sqrt(self.var)
        return e if name is None else e[..., self._index(name)]

    def std_over_draws(self):
        """(B, L, I) standard deviation of the values over the S draws: the continuum posterior's error bar"""
        if self.S < 2:
            raise QFAHipError("std_over_draws needs at least two draws (n_samples >= 2)")
        return self.value.std(1, unbiased=True)

    def is_bal(self, index="BI", min_value=0.0, nsigma=0.0):
        """(B, L) bool: the mean of the index over the draws exceeds ``min_value`` and ``nsigma`` times its error (the noise error and,
        with S >= 2, the scatter over the draws, in quadrature)"""
        x = self._index(index)
        v = self.value[..., x].mean(1)
        e2 = self.var[..., x].mean(1)
        if self.S >= 2:
            e2 = e2 + self.value[..., x].var(1, unbiased=True)
        return (v > float(min_value)) & (v > float(nsigma) * torch.sqrt(e2))

    def _troughs_of(self, line, draw, min_value):
        """per spectrum the (., 2) troughs of ``line`` in ``draw``, none where the trough index of the spectrum is <= min_value"""
        tr = self.troughs[:, int(draw), int(line)].cpu().numpy()
        val = self.value[:, int(draw), int(line), self._index(self.trough_index)].cpu().numpy()
        out = []
        for b in range(self.B):
            t = tr[b][np.isfinite(tr[b, :, 0])]
            out.append(t if val[b] > float(min_value) else t[:0])
        return out

    def to_intervals(self, line=0, draw=0, min_value=0.0, pad_kms=0.0, lines=BAL_LINES):
        """The per-spectrum list ``mask_absorbers(rest=...)`` takes: for every trough [v_min, v_max] of ``line`` in ``draw`` the
        intervals ``bal_intervals(v_min - pad_kms, v_max + pad_kms, lines)``; a spectrum whose trough index is not above
        ``min_value`` gets none.  ``line`` = None: the troughs of every scanned line."""
        which = range(len(self.lines)) if line is None else [int(line)]
        per_line = [self._troughs_of(l, draw, min_value) for l in which]
        out = []
        for b in range(self.B):
            t = np.concatenate([pl[b] for pl in per_line]).reshape(-1, 2)
            out.append(bal_intervals(t[:, 0] - float(pad_kms), t[:, 1] + float(pad_kms), lines) if len(t) else np.zeros((0, 2)))
        return out

    def to_table(self, names, draw=0, min_value=0.0):
        """the troughs as ``io.write_bal_csv`` takes them: file, line, v_min, v_max and the spectrum's bi, ai of that line (NaN for
        an index the scan does not hold)"""
        names = [str(n) for n in names]
        if len(names) != self.B:
            raise QFAHipError(f"to_table: {len(names)} names for {self.B} spectra")
        col = lambda n: self.index(n)[:, int(draw)].cpu().numpy() if n in self.index_names else np.full((self.B, len(self.lines)), np.nan)
        bi, ai = col("BI"), col("AI")
        rows = {k: [] for k in ("file", "line", "v_min", "v_max", "bi", "ai")}
        for l, lam in enumerate(self.lines):
            for b, t in enumerate(self._troughs_of(l, draw, min_value)):
                for v0, v1 in t:
                    for k, x in zip(rows, (names[b], lam, v0, v1, bi[b, l], ai[b, l])):
                        rows[k].append(x)
        return {k: np.asarray(v, dtype=str if k == "file" else np.float64) for k, v in rows.items()}

    def arrays(self):
        """what bal_scan.npz holds"""
        n = lambda t: t.cpu().numpy()
        return {"value": n(self.value), "var": n(self.var), "n_pix": n(self.n_pix), "n_runs": n(self.n_runs), "n_bridged": n(self.n_bridged),
                "n_used": n(self.n_used), "n_troughs": n(self.n_troughs), "troughs": n(self.troughs),
                "lines": np.asarray(self.lines), "index_names": np.asarray(self.index_names),
                "index_defs": np.asarray([[d[0], d[1], d[2], float(_lib.BAL_MODES[d[3]])] for d in self.indices.values()]),
                "trough_index": np.asarray(self.trough_index), "thr": np.float64(self.thr)}

    @classmethod
    def concat(cls, scans):
        """the scans of consecutive slices as one"""
        s0 = scans[0]
        cat = lambda name: torch.cat([getattr(s, name) for s in scans], dim=0)
        opt = lambda name: None if getattr(s0, name) is None else cat(name)
        return cls(cat("value"), cat("var"), cat("counts"), cat("line_counts"), cat("troughs"), s0.lines, s0.indices, s0.trough_index,
                   s0.thr, opt("mask"), opt("n_masked"))


def bal_mask(mask, wav_grid, troughs, *, draw=0, lines=BAL_LINES, pad_kms=0.0, out=None):
    """qfa_bal_mask_f32: ``mask`` (B, Npix) bool device tensor or None (all set) with the pixels inside the troughs of ``draw``
    cleared -- ``troughs`` (B, S, L, 8, 2) as ``BALScan.troughs`` -- for every line of ``lines``.  Returns ``(mask_out, n_masked)``."""
    _lib.require_device_tensor(troughs, torch.float64, "troughs")
    if troughs.dim() != 5 or tuple(troughs.shape[3:]) != (_lib.BAL_MAX_TROUGHS, 2):
        raise QFAHipError(f"troughs: shape {tuple(troughs.shape)}, expected (B, S, L, {_lib.BAL_MAX_TROUGHS}, 2)")
    dev = troughs.device
    B, S, L = (int(x) for x in troughs.shape[:3])
    grid = np.ascontiguousarray(np.asarray(wav_grid, dtype=np.float64).reshape(-1))
    npix = len(grid)
    lam = np.ascontiguousarray(np.asarray(lines, dtype=np.float64).reshape(-1))
    if not 1 <= len(lam) <= _lib.BAL_MAX_LINES:
        raise QFAHipError(f"lines: {len(lam)} lines, supported 1..{_lib.BAL_MAX_LINES}")
    if mask is not None:
        _lib.require_device_tensor(mask, torch.bool, "mask")
        if tuple(mask.shape) != (B, npix):
            raise QFAHipError(f"mask: shape {tuple(mask.shape)}, expected ({B}, {npix})")
    if out is None:
        out = torch.empty((B, npix), dtype=torch.bool, device=dev)
    else:
        _lib.require_device_tensor(out, torch.bool, "out")
        if tuple(out.shape) != (B, npix):
            raise QFAHipError(f"out: shape {tuple(out.shape)}, expected ({B}, {npix})")
    nm = torch.zeros((B,), dtype=torch.int32, device=dev)
    g_d = torch.as_tensor(grid, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qfa_bal_mask_f32(_ptr(mask), _ptr(g_d), _ptr(troughs), B, S, L, int(draw), npix,
                                               lam.ctypes.data_as(C.POINTER(C.c_double)), len(lam), float(pad_kms), _ptr(out), _ptr(nm),
                                               _lib.current_stream(dev)), "qfa_bal_mask_f32")
    return out, nm


class BALFinder(object):
    """``bal_scan`` / ``bal_catalog``: a plain base class of ``qfa_amd.model.QFA`` that uses the model's plumbing as any other method
    of it does."""

    def _bal_windows(self, grid, lines, indices):
        """[(p_lo, p_hi, vedge on the device)] per line, once per ``bal_scan``; raises for a window on the blue side"""
        v_lo_all, v_hi_all = min(d[0] for d in indices.values()), max(d[1] for d in indices.values())
        out = []
        for lam in lines:
            p_lo, p_hi, vedge = velocity_window(grid, lam, v_lo_all, v_hi_all, self.Nb)
            out.append((p_lo, p_hi, torch.as_tensor(vedge, device=self.device)))
        return out

    def _bal_call(self, bs, h, B, windows, lines, indices, thr, smooth, max_gap, cont_min, trough_index):
        """one call of qfa_bal_scan_f32; h (B, S, Nh) on the device, ``windows`` from ``_bal_windows``"""
        dev = self.device
        S = int(h.shape[1])
        q = _lib.BalParams()
        q.n_lines, q.n_indices = len(lines), len(indices)
        for l, (p_lo, p_hi, t) in enumerate(windows):
            q.p_lo[l], q.p_hi[l], q.vedge[l] = p_lo, p_hi, t.data_ptr()
        for x, d in enumerate(indices.values()):
            q.index[x] = _lib.BalIndex(d[0], d[1], d[2], _lib.BAL_MODES[d[3]])
        q.thr, q.smooth, q.max_gap = float(thr), int(smooth), int(max_gap)
        q.trough_index = list(indices).index(trough_index)
        L, I = len(lines), len(indices)
        value = torch.empty((B, S, L, I), dtype=torch.float64, device=dev)
        var = torch.empty((B, S, L, I), dtype=torch.float64, device=dev)
        counts = torch.empty((B, S, L, I, 3), dtype=torch.int32, device=dev)
        line_counts = torch.empty((B, S, L, 2), dtype=torch.int32, device=dev)
        troughs = torch.empty((B, S, L, _lib.BAL_MAX_TROUGHS, 2), dtype=torch.float64, device=dev)
        mu = self.mu.to(device=dev, dtype=f32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().qfa_bal_scan_f32(
                _lib.require_device_tensor(self.F, f32, "F"), _ptr(mu), C.byref(bs), _lib.require_device_tensor(h, f32, "h"), B, S,
                self.Npix, self.Nb, self.Nh, C.byref(q), float(cont_min), 0, _ptr(value), _ptr(var), _ptr(counts), _ptr(line_counts),
                _ptr(troughs), _lib.current_stream(dev)), "qfa_bal_scan_f32")
        return BALScan(value, var, counts, line_counts, troughs, lines, indices, trough_index, thr)

    def bal_scan(self, flux=None, error=None, mask=None, *, wav_grid, lines=DEFAULT_LINES, indices=None, thr=0.9, smooth=1, max_gap=0,
                 cont_min=0.0, h=None, hmean=None, hcov=None, n_samples=0, seed=0, offset=0, zabs=None, zfac=None, batch=None, n_iter=1,
                 mask_lines=BAL_LINES, pad_kms=0.0, trough_index=None):
        """BI, AI and the trough velocities of a batch under the posterior continuum (the contract is in include/qfa_hip.h,
        qfa_bal_scan_f32).  ``wav_grid`` (Npix,) gives every line its velocity window; ``lines`` (1..4) in Angstrom, all on the red
        side of the model; ``indices``: {name: (v_lo, v_hi, w_min, 'after' | 'whole')}, default BI and AI; ``trough_index``: the index
        whose qualifying runs are listed as troughs (default 'AI' if present, else the last).  The latent
        (``QFA._resolve_latent``): ``h`` | ``hmean`` | ``hmean`` + ``hcov`` + ``n_samples``, else ``predict`` runs on the
        inputs first (``zabs`` or ``zfac`` only serve that ``predict``).  Every input form of a batch: the tensors, or ``batch`` = a
        ``ResidentBatch``.  ``n_iter`` > 1 repeats predict -> scan -> mask: the pixels inside draw 0's troughs of all scanned lines,
        imaged onto every line of ``mask_lines`` and widened by ``pad_kms``, are cleared from a copy of ``mask`` on the device
        (qfa_bal_mask_f32) and the next PREDICT runs with that mask, so that the troughs no longer pull the continuum down; every
        scan reads the caller's ``mask`` (a masked trough could not be measured).  It needs the tensor form and no latent given (a
        resident batch carries its mask with it).  Returns the ``BALScan`` of the last iteration, with ``mask`` (the last predict's)
        and ``n_masked``."""
        if self.mu is None:
            raise QFAHipError("bal_scan needs model.mu (load_from_npz or train first)")
        lines = check_scan_params(lines, thr, smooth, max_gap)
        indices = check_indices(indices)
        if trough_index is None:
            trough_index = "AI" if "AI" in indices else list(indices)[-1]
        if trough_index not in indices:
            raise QFAHipError(f"trough_index {trough_index!r} is not one of {tuple(indices)}")
        grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
        if len(grid) != self.Npix:
            raise QFAHipError(f"len(wav_grid) = {len(grid)}, the model has {self.Npix} pixels")
        windows = self._bal_windows(grid, lines, indices)       # (raises for a blue-side window before anything runs)
        n_iter = int(n_iter)
        if n_iter < 1:
            raise QFAHipError(f"n_iter = {n_iter}, expected >= 1")
        if n_iter > 1:
            if batch is not None:
                raise QFAHipError("bal_scan: n_iter > 1 takes the tensor form (a resident batch carries its own mask)")
            if h is not None or hmean is not None:
                raise QFAHipError("bal_scan: n_iter > 1 runs predict itself: give no latent")
        self._params_struct()
        if batch is not None:
            B = batch.B
        else:
            if not isinstance(flux, torch.Tensor) or flux.dim() != 2:
                raise QFAHipError("bal_scan: flux must be a (B, Npix) tensor")
            B = int(flux.shape[0])
            for t, name in ((flux, "flux"), (error, "error"), (mask if mask is not None else flux, "mask")):
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, self.Npix):
                    raise QFAHipError(f"{name}: expected a ({B}, {self.Npix}) tensor")
        n_masked, pmask = None, mask                            # pmask: what predict sees; the scan always reads the caller's mask
        for it in range(n_iter):
            h_it, _, _ = self._resolve_latent("bal_scan", B, h=h, hmean=hmean, hcov=hcov, n_samples=n_samples, seed=seed, offset=offset,
                                              unc=None, predict_inputs=dict(flux=flux, error=error, zabs=zabs, mask=pmask, zfac=zfac,
                                                                            batch=batch))
            bs, keep = self._batch_struct_rows(batch, raw_flux=True) if batch is not None else self._flux_batch(flux, error, mask)
            bs.A_blue = bs.zabs = bs.zq1 = bs.pix_ratio = None      # (not read by the call)
            scan = self._bal_call(bs, h_it if h is not None else h_it.contiguous(), B, windows, lines, indices, thr, smooth, max_gap, cont_min, trough_index)
            del keep
            if it + 1 < n_iter:                                 # (from the caller's mask every time: the troughs are measured anew)
                pmask, n_masked = bal_mask(mask, grid, scan.troughs, draw=0, lines=mask_lines, pad_kms=pad_kms)
        if n_iter > 1:
            scan.mask, scan.n_masked = pmask, n_masked
        return scan

    def bal_catalog(self, dataloader, *, lines=DEFAULT_LINES, indices=None, thr=0.9, smooth=1, max_gap=0, cont_min=0.0, n_samples=0,
                    seed=0, n_iter=1, mask_lines=BAL_LINES, pad_kms=0.0, trough_index=None, batch_size=4096):
        """``bal_scan`` of a whole dataloader: one ``BALScan`` of all its spectra in loader order, S = max(1, n_samples) draws, the
        global row of a spectrum being its draw offset (the result does not depend on ``batch_size``).  It walks the loader as
        ``observed_stack`` does (the resident rows form when the loader has one; ``n_iter`` > 1 materialises the tensors with the
        loader's ``get_rows``).  Under data parallelism every rank scans its own shard, as ``dla_scan`` does.  ``names`` of the
        result: the loader's paths in row order."""
        if not hasattr(dataloader, "wav_grid"):
            raise QFAHipError("bal_catalog: the dataloader must carry wav_grid (a DeviceDataloader)")
        kw = dict(wav_grid=dataloader.wav_grid, lines=lines, indices=indices, thr=thr, smooth=smooth, max_gap=max_gap, cont_min=cont_min,
                  n_samples=int(n_samples), seed=seed, mask_lines=mask_lines, pad_kms=pad_kms, trough_index=trough_index)
        row0 = int(getattr(dataloader, "_row0", 0))
        scans, names = [], []
        if int(n_iter) > 1:
            if not hasattr(dataloader, "get_rows"):
                raise QFAHipError("bal_catalog: n_iter > 1 needs a loader with get_rows (the tensor form)")
            n = len(dataloader)
            for s in range(0, n, int(batch_size)):
                f, e, z, m, paths = dataloader.get_rows(s, min(s + int(batch_size), n))
                names += list(paths)
                scans.append(self.bal_scan(f, e, m, zabs=z, offset=row0 + s, n_iter=int(n_iter), **kw))
        else:
            for s, inputs, paths in self._loader_slices(dataloader, int(batch_size)):
                names += list(paths)
                _, hmean, hcov, _, _ = self.predict(**inputs)
                inp = {k: v for k, v in inputs.items() if k != "zabs"}
                scans.append(self.bal_scan(**inp, hmean=hmean, hcov=hcov if int(n_samples) > 0 else None, offset=row0 + s, **kw))
        if not scans:
            raise QFAHipError("bal_catalog: the dataloader is empty")
        scan = BALScan.concat(scans)
        scan.names = [str(x) for x in names]                    # the loader's paths, in row order (``to_table(scan.names)``)
        return scan
