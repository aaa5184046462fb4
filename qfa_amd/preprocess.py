"""Observed-frame spectra onto the common rest-frame grid, on the device (include/qfa_hip.h ``qfa_preprocess_f32`` states the rule).

Every other entry point of the package assumes the reference's contract -- rest frame, one common log-lambda grid, normalised
at 1280 A, ``-999`` sentinels, a catalogue with ``snr`` and ``num_mask`` (reference QFA/dataloader.py:21-24,49).  ``preprocess``
takes spectra as a survey delivers them (observed wavelength, flux, inverse variance, pixel flags, z; ragged) and returns the two
``(N, Npix)`` float32 device arrays ``DeviceDataloader`` accepts plus the catalogue's columns; ``Preprocessed.write_npz`` is the
file form the reference's ``--type train --catalog ... --data_dir ...`` reads.

    python -m qfa_amd.preprocess --catalog observed.csv --data_dir raw/ --output_dir prepared/ [--lammin 1030 --lammax 1600
                                                                                               --loglam_delta 1e-4 ...]
                                [--dla_catalog dla.csv --sky_mask sky.txt --dla_tmin 0.8 --dla_b 30 --no_dla_correct]
                                [--bal_catalog bal.csv --bal_pad_kms 0]
                                [--calibration cal.npz]

With ``--dla_catalog`` / ``--sky_mask`` the catalogued absorbers and bad observed wavelengths are masked and corrected
(``qfa_amd.absorbers``) before the files are written; with ``--calibration`` the spectra are first divided by that calibration
vector (``qfa_amd.calibration``, the file of ``io.write_calibration``).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError

MAX_NPIX, MAX_N_IN = 16384, 32768
_I32_FIELDS = ("n_valid", "n_lead", "n_trail", "num_mask", "ok")


def edges_from_grid(wav_grid):
    """Rest-frame output edges of a grid (float64, Npix + 1): the geometric midpoints of neighbouring pixel centres, and half a
    step of log10(lambda) beyond each end."""
    g = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    if len(g) < 2:
        raise ValueError("a grid of one pixel has no step: pass out_edges")
    lg = np.log10(g)
    mid = 0.5 * (lg[:-1] + lg[1:])
    return 10.0 ** np.concatenate([[lg[0] - 0.5 * (lg[1] - lg[0])], mid, [lg[-1] + 0.5 * (lg[-1] - lg[-2])]])


class Preprocessed(object):
    """What ``preprocess`` returns: ``flux``, ``error`` (N, Npix) float32 with the reference's ``-999`` sentinels, and per spectrum
    ``zqso``, ``norm``, ``snr`` (float64), ``num_mask``, ``n_valid``, ``n_lead``, ``n_trail`` (int32), ``ok`` (bool), on
    whatever device the tensors live on (the host logic below works on CPU tensors too); ``wav_grid`` is a numpy array."""

    def __init__(self, flux, error, zqso, norm, snr, num_mask, n_valid, n_lead, n_trail, ok, wav_grid):
        self.flux, self.error, self.zqso, self.norm, self.snr = flux, error, zqso, norm, snr
        self.num_mask, self.n_valid, self.n_lead, self.n_trail, self.ok = num_mask, n_valid, n_lead, n_trail, ok
        self.wav_grid = np.asarray(wav_grid, dtype=np.float64)
        n = int(flux.shape[0])
        if tuple(error.shape) != tuple(flux.shape) or flux.ndim != 2 or flux.shape[1] != len(self.wav_grid):
            raise QFAHipError("flux / error must be (N, len(wav_grid))")
        for name in ("zqso", "norm", "snr", "num_mask", "n_valid", "n_lead", "n_trail", "ok"):
            if tuple(getattr(self, name).shape) != (n,):
                raise QFAHipError(f"{name} must be ({n},)")

    def __len__(self):
        return int(self.flux.shape[0])

    def _host(self, name):
        return getattr(self, name).detach().cpu().numpy()

    def select(self, snr_min=-np.inf, snr_max=np.inf, z_min=-np.inf, z_max=np.inf, num_mask=np.inf):
        """Row indices (numpy int64, ascending) of the spectra that are ``ok`` and pass the reference's catalogue criteria
        (QFA/dataloader.py:49): snr and z inside their limits, at most ``num_mask`` masked regions.  A NaN snr passes nothing."""
        snr, z, nm, ok = self._host("snr"), self._host("zqso"), self._host("num_mask"), self._host("ok").astype(bool)
        with np.errstate(invalid="ignore"):
            keep = ok & (snr >= snr_min) & (snr <= snr_max) & (z >= z_min) & (z <= z_max) & (nm <= num_mask)
        return np.nonzero(keep)[0].astype(np.int64)

    def mask_absorbers(self, **kw):
        """Catalogued absorbers and bad wavelengths (``qfa_amd.absorbers.mask_absorbers``, whose keywords these are) applied to
        these spectra: a new ``Preprocessed`` with the masked / corrected arrays and ``snr``, ``num_mask``, ``n_valid``,
        ``n_lead``, ``n_trail`` recomputed on them, ``norm`` and ``ok`` carried over, and the per-spectrum counts
        ``n_absorber_masked`` / ``n_interval_masked`` as attributes."""
        from .absorbers import mask_absorbers
        if kw.pop("return_trans", False):
            raise QFAHipError("Preprocessed.mask_absorbers returns a Preprocessed: call absorbers.mask_absorbers for the transmission")
        kw.setdefault("device", self.flux.device)
        fo, eo, rec = mask_absorbers(self.flux, self.error, self.zqso, self.wav_grid, **kw)
        new = Preprocessed(fo, eo, self.zqso, self.norm, rec["snr"], rec["num_mask"], rec["n_valid"], rec["n_lead"], rec["n_trail"],
                           self.ok, self.wav_grid)
        new.n_absorber_masked, new.n_interval_masked = rec["n_absorber_masked"], rec["n_interval_masked"]
        return new

    def calibrate(self, table, **kw):
        """These spectra divided by a calibration vector (``qfa_amd.calibration.calibrate``, whose keywords these are; ``table``: an
        ``ObservedStack`` or the dict of ``io.read_calibration``): a new ``Preprocessed`` with the calibrated arrays and the count
        ``n_uncalibrated`` as an attribute.  ``norm`` and ``snr`` are unchanged by a common factor and are carried over."""
        from .calibration import calibrate
        kw.setdefault("device", self.flux.device)
        fo, eo, nu = calibrate(self.flux, self.error, self.zqso, self.wav_grid, table, **kw)
        new = Preprocessed(fo, eo, self.zqso, self.norm, self.snr, self.num_mask, self.n_valid, self.n_lead, self.n_trail, self.ok,
                           self.wav_grid)
        new.n_uncalibrated = nu
        return new

    @staticmethod
    def _file_names(names):
        return [n if str(n).endswith(".npz") else f"{n}.npz" for n in map(str, names)]

    def catalog(self, names):
        """The ``file, snr, z, num_mask`` table ``io.select_from_catalog`` reads, one row per ``ok`` spectrum (the others have no
        file: ``write_npz`` does not write them)."""
        import pandas as pd
        if len(names) != len(self):
            raise ValueError(f"{len(names)} names for {len(self)} spectra")
        ok = self._host("ok").astype(bool)
        files = np.array(self._file_names(names), dtype=object)
        return pd.DataFrame({"file": files[ok], "snr": self._host("snr")[ok], "z": self._host("zqso")[ok],
                             "num_mask": self._host("num_mask")[ok].astype(np.int64)})

    def write_npz(self, output_dir, names):
        """One reference-format file per ``ok`` spectrum (``flux``, ``error``, ``z``, ``snr``; reference QFA/dataloader.py:18-30)
        and ``catalog.csv`` in ``output_dir``; returns the catalogue's path."""
        cat = self.catalog(names)
        os.makedirs(output_dir, exist_ok=True)
        rows = np.nonzero(self._host("ok").astype(bool))[0]
        flux, error = self._host("flux"), self._host("error")
        for r, (_, c) in zip(rows, cat.iterrows()):
            np.savez(os.path.join(output_dir, c["file"]), flux=flux[r], error=error[r], z=np.float64(c["z"]),
                     snr=np.float64(c["snr"]))
        path = os.path.join(output_dir, "catalog.csv")
        cat.to_csv(path, index=False)
        return path


def _dev(x, dtype, device, name):
    """contiguous device tensor of a host array or a tensor (a tensor must already have the dtype: no silent conversion pass)"""
    if isinstance(x, torch.Tensor):
        if x.dtype != dtype:
            raise QFAHipError(f"{name}: dtype {x.dtype}, expected {dtype}")
        return x.to(device).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x, dtype=torch.empty(0, dtype=dtype).numpy().dtype), device=device)


def preprocess(wave, flux, ivar, offsets, zqso, wav_grid, *, bad=None, min_coverage=0.5, norm_window=(1270., 1290.),
               norm_min_pixels=5, snr_window=(1270., 1600.), device, out=None, out_edges=None):
    """Rebin N ragged observed-frame spectra onto ``wav_grid`` (rest frame), normalise them and take their S/N and run counts
    (the rule: include/qfa_hip.h, ``qfa_preprocess_f32``).  ``wave`` (float64), ``flux``, ``ivar`` (float32), optional ``bad``
    (uint8 / bool, non-zero = unusable) are concatenated over the spectra, ``offsets`` (int64, N + 1) cuts them, ``zqso`` (N);
    host arrays or device tensors.  ``out`` = (flux, error): two (N, Npix) float32 device tensors to fill in place.
    ``out_edges`` (Npix + 1, rest frame, increasing) overrides the edges derived from ``wav_grid`` (``edges_from_grid``).
    Returns a ``Preprocessed`` on ``device``; raises ``QFAHipError`` on a CPU device (there is no fallback)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise QFAHipError("preprocess needs a HIP device (torch device 'cuda'); qfa_amd has no CPU fallback")
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    npix = len(grid)
    edges = edges_from_grid(grid) if out_edges is None else np.asarray(out_edges, dtype=np.float64).reshape(-1)
    if len(edges) != npix + 1 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0) or not edges[0] > 0:
        raise QFAHipError("out_edges must be len(wav_grid) + 1 finite, positive, increasing wavelengths")
    off_h = (offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)).astype(np.int64).reshape(-1)
    if len(off_h) < 1:
        raise QFAHipError("offsets must hold N + 1 entries")
    n = len(off_h) - 1
    total = int(wave.shape[0])
    lens = np.diff(off_h)
    if off_h[0] < 0 or np.any(lens < 0) or off_h[-1] > total:
        raise QFAHipError("offsets must be non-decreasing and lie inside the input arrays")
    max_n_in = int(lens.max()) if n else 0
    if max_n_in > MAX_N_IN:
        raise QFAHipError(f"a spectrum has {max_n_in} input pixels, the limit is {MAX_N_IN}")
    if not 1 <= npix <= MAX_NPIX:
        raise QFAHipError(f"len(wav_grid) = {npix}, supported 1..{MAX_NPIX}")
    if int(flux.shape[0]) != total or int(ivar.shape[0]) != total or (bad is not None and int(bad.shape[0]) != total):
        raise QFAHipError("wave, flux, ivar and bad must have one length")
    zq = _dev(zqso, torch.float64, device, "zqso").reshape(-1)
    if zq.shape[0] != n:
        raise QFAHipError(f"zqso must be ({n},)")
    w_d, f_d, v_d = _dev(wave, torch.float64, device, "wave"), _dev(flux, torch.float32, device, "flux"), \
        _dev(ivar, torch.float32, device, "ivar")
    b_d = None
    if bad is not None:
        if isinstance(bad, torch.Tensor):
            b_d = bad.to(device).contiguous()
            b_d = b_d.view(torch.uint8) if b_d.dtype == torch.bool else b_d
            if b_d.dtype != torch.uint8:
                raise QFAHipError(f"bad: dtype {b_d.dtype}, expected uint8 or bool")
        else:
            b_d = torch.as_tensor(np.ascontiguousarray(np.asarray(bad) != 0).view(np.uint8), device=device)
    off_d = torch.as_tensor(off_h, device=device)
    e_d, g_d = torch.as_tensor(edges, device=device), torch.as_tensor(grid, device=device)
    if out is not None:
        fo, eo = out
        for t, name in ((fo, "out[0]"), (eo, "out[1]")):
            _lib.require_device_tensor(t, torch.float32, name)
            if tuple(t.shape) != (n, npix) or t.device != w_d.device:
                raise QFAHipError(f"{name} must be ({n}, {npix}) on {w_d.device}")
    else:
        fo = torch.empty((n, npix), dtype=torch.float32, device=device)
        eo = torch.empty((n, npix), dtype=torch.float32, device=device)
    rf = torch.empty((n, 2), dtype=torch.float64, device=device)
    ri = torch.empty((n, len(_I32_FIELDS)), dtype=torch.int32, device=device)
    q = _lib.PreprocessParams(float(min_coverage), float(norm_window[0]), float(norm_window[1]), float(snr_window[0]),
                              float(snr_window[1]), int(norm_min_pixels))
    h = _lib.lib()
    wsb = h.qfa_preprocess_workspace_bytes(n, npix, max_n_in)
    ws = torch.empty((max(int(wsb), 16),), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(h.qfa_preprocess_f32(_lib._ptr(w_d), _lib._ptr(f_d), _lib._ptr(v_d), _lib._ptr(b_d), _lib._ptr(off_d),
                                        _lib._ptr(zq), n, max_n_in, _lib._ptr(e_d), _lib._ptr(g_d), npix, C.byref(q),
                                        _lib._ptr(fo), _lib._ptr(eo), _lib._ptr(rf), _lib._ptr(ri), _lib._ptr(ws), int(wsb),
                                        _lib.current_stream(device)), "qfa_preprocess_f32")
    if out is not None:
        for t in out:                                          # written through raw pointers: tell torch
            torch.autograd.graph.increment_version(t)
    rec = {name: ri[:, c].contiguous() for c, name in enumerate(_I32_FIELDS)}
    return Preprocessed(fo, eo, zq, rf[:, 0].contiguous(), rf[:, 1].contiguous(), rec["num_mask"], rec["n_valid"],
                        rec["n_lead"], rec["n_trail"], rec["ok"] != 0, grid)


def main(argv=None):
    """file to file: read observed per-spectrum files, ``preprocess``, ``write_npz``"""
    import argparse
    import pandas as pd
    from . import io
    ap = argparse.ArgumentParser(prog="python -m qfa_amd.preprocess", description=main.__doc__)
    ap.add_argument("--catalog", required=True, help="csv whose first column lists the observed-frame files")
    ap.add_argument("--data_dir", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--lammin", type=float, default=1030.)
    ap.add_argument("--lammax", type=float, default=1600.)
    ap.add_argument("--loglam_delta", type=float, default=1e-4)
    ap.add_argument("--min_coverage", type=float, default=0.5)
    ap.add_argument("--norm_window", type=float, nargs=2, default=(1270., 1290.))
    ap.add_argument("--norm_min_pixels", type=int, default=5)
    ap.add_argument("--snr_window", type=float, nargs=2, default=(1270., 1600.))
    ap.add_argument("--nprocs", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dla_catalog", default=None, help="csv with columns file, z_abs, log_nhi: mask and correct these absorbers")
    ap.add_argument("--sky_mask", default=None, help="two-column file of observed-frame intervals [lo, hi) in Angstrom to mask")
    ap.add_argument("--dla_tmin", type=float, default=0.8, help="mask where the absorbers' transmission is below this")
    ap.add_argument("--dla_b", type=float, default=30., help="Doppler parameter of the absorbers, km/s")
    ap.add_argument("--no_dla_correct", action="store_true", help="mask only: do not divide by the absorbers' profile")
    ap.add_argument("--bal_catalog", default=None, help="csv with columns file, v_min, v_max (io.write_bal_csv): mask these BAL troughs")
    ap.add_argument("--bal_pad_kms", type=float, default=0., help="widen every BAL trough by this many km/s on both sides")
    ap.add_argument("--calibration", default=None, help="npz of io.write_calibration: divide the spectra by this calibration vector")
    a = ap.parse_args(argv)
    names = [str(x) for x in pd.read_csv(a.catalog).iloc[:, 0].values]
    wave, flux, ivar, bad, offsets, zqso = io.read_observed_npz([os.path.join(a.data_dir, n) for n in names], a.nprocs)
    grid = io.wavelength_grid(a.lammin, a.lammax, a.loglam_delta)
    pre = preprocess(wave, flux, ivar, offsets, zqso, grid, bad=bad, min_coverage=a.min_coverage, norm_window=tuple(a.norm_window),
                     norm_min_pixels=a.norm_min_pixels, snr_window=tuple(a.snr_window), device=a.device)
    if a.calibration is not None:
        pre = pre.calibrate(io.read_calibration(a.calibration))
    if a.dla_catalog is not None or a.sky_mask is not None or a.bal_catalog is not None:
        from .absorbers import AbsorberCatalog
        dla = None
        if a.dla_catalog is not None:
            dla = AbsorberCatalog.from_table([os.path.basename(n) for n in names], io.read_absorber_csv(a.dla_catalog))
            if dla.unmatched:
                print(f"{len(dla.unmatched)} file names of {a.dla_catalog} match no spectrum, the first: {dla.unmatched[0]}")
        sky = io.read_intervals(a.sky_mask) if a.sky_mask is not None else None
        rest = None
        if a.bal_catalog is not None:
            rest = io.bal_rest_intervals([os.path.basename(n) for n in names], io.read_bal_csv(a.bal_catalog), a.bal_pad_kms)
        pre = pre.mask_absorbers(dla=dla, sky=sky, rest=rest, t_min=a.dla_tmin, b_kms=a.dla_b, correct=not a.no_dla_correct,
                                 snr_window=tuple(a.snr_window))
    path = pre.write_npz(a.output_dir, [os.path.basename(n) for n in names])
    print(f"{int(pre.ok.sum())} of {len(pre)} spectra written to {a.output_dir}; catalogue {path}")
    return 0


class _CallableModule(type(os)):
    """The issue of names: the package exports the function ``preprocess`` lazily (``qfa_amd/__init__.py``, ``_LAZY``), and
    importing this module binds the MODULE to the same attribute ``qfa_amd.preprocess``.  Calling the module calls the function,
    so ``qfa_amd.preprocess(...)`` means one thing whether or not the module has been imported yet."""

    def __call__(self, *args, **kw):
        return preprocess(*args, **kw)


sys.modules[__name__].__class__ = _CallableModule


if __name__ == "__main__":
    raise SystemExit(main())
