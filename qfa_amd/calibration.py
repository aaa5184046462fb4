"""The observed-frame residual stack: the flux-calibration vector and the sky-line mask from the data themselves (include/qfa_hip.h,
``qfa_obs_stack_f32`` and ``qfa_calibrate_f32`` state the rules).

Sky-line residuals, Galactic Ca H&K and the spectrograph's calibration residual spoil the same OBSERVED wavelengths of every spectrum.
``QFA.observed_residuals`` / ``QFA.observed_stack`` stack r = flux / continuum -- the posterior continuum ``mu + F h``, never written
-- in bins of observed wavelength over all spectra (``ObservedStack``).  Its mean is the calibration vector
(``ObservedStack.calibration``), bins whose scatter or mean stand out are the lines to mask (``ObservedStack.find_lines``: the
``sky=`` intervals of ``mask_absorbers``), and ``calibrate`` divides spectra by the vector.  No transmission model is applied: on
the blue side of Lyman-alpha the stack holds <T> x calibration, so a calibration is measured with ``rest_range`` on the red side."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError, _ptr
from .stacks import _DrawStack

MAX_BINS = 32768
f32 = torch.float32


def obs_grid(lam_min, nbin, dloglam=None, dlam=None):
    """(u0, du, nbin, mode) of ``nbin`` bins from ``lam_min`` Angstrom on: ``dloglam`` -- bins of log10(lambda), u = log10 -- or
    ``dlam`` -- bins of lambda in Angstrom.  The one place in Python where the bounds of the C checks are written."""
    if (dloglam is None) == (dlam is None):
        raise QFAHipError("observed-frame bins: give dloglam or dlam, one of them")
    lam_min, nbin = float(lam_min), int(nbin)
    if not (lam_min > 0.0 and np.isfinite(lam_min)):
        raise QFAHipError(f"observed-frame bins: lam_min = {lam_min}")
    mode = "log" if dlam is None else "linear"
    u0 = float(np.log10(lam_min)) if mode == "log" else lam_min
    du = float(dloglam if mode == "log" else dlam)
    return _check_grid(u0, du, nbin, mode)


def _check_grid(u0, du, nbin, mode):
    if mode not in _lib.OBS_MODES:
        raise QFAHipError(f"observed-frame bins: mode {mode!r}, expected 'log' or 'linear'")
    u0, du, nbin = float(u0), float(du), int(nbin)
    if not (du > 0.0 and np.isfinite(du) and np.isfinite(1.0 / du) and np.isfinite(u0) and 1 <= nbin <= MAX_BINS):
        raise QFAHipError(f"observed-frame bins: u0 = {u0}, du = {du}, nbin = {nbin} (1..{MAX_BINS})")
    return u0, du, nbin, mode


def coordinates(wav_grid, zqso, mode):
    """(pix_u, spec_u) float64 as the kernels take them: log10(wav_grid) and log10(1 + z) (NaN where 1 + z <= 0: the spectrum is not
    stacked), or wav_grid and 1 + z"""
    grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
    if not (np.all(np.isfinite(grid)) and np.all(grid > 0.0) and np.all(np.diff(grid) >= 0.0)):
        raise QFAHipError("wav_grid must be finite, positive and non-decreasing")
    zq1 = 1.0 + np.asarray(zqso, dtype=np.float64).reshape(-1)
    if mode == "log":
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.log10(grid), np.where(zq1 > 0.0, np.log10(np.where(zq1 > 0.0, zq1, 1.0)), np.nan)
    return grid, zq1


class ObservedStack(_DrawStack):
    """The stack of r = flux / continuum in bins of observed wavelength (include/qfa_hip.h, qfa_obs_stack_f32): ``buf`` = (S, 4, nbin)
    float64 [sum w | sum w r | sum w r^2 | n] per draw of the continuum over the bins [u0 + k du, u0 + (k + 1) du) of u = log10(lambda)
    (``mode`` 'log') or u = lambda ('linear'); u0 and du are float64 as given.  ``calibration``, ``chi2`` and ``find_lines`` work on
    the sums averaged over the draws."""

    def __init__(self, buf, u0, du, nbin, mode="log"):
        self.u0, self.du, self.nbin, self.mode = _check_grid(u0, du, nbin, mode)
        if buf.dtype != torch.float64 or buf.dim() != 3 or buf.shape[0] < 1 or tuple(buf.shape[1:]) != (4, self.nbin) \
                or not buf.is_contiguous():
            raise QFAHipError(f"ObservedStack: buffer {tuple(buf.shape)} {buf.dtype}, expected contiguous float64 (S, 4, {self.nbin})")
        self.z0, self.dz, self._nbins = self.u0, self.du, self.nbin      # (what _DrawStack's own methods read)
        self.buf = buf

    @classmethod
    def zeros(cls, S, u0, du, nbin, mode="log", device="cpu"):
        return cls(torch.zeros((int(S), 4, int(nbin)), dtype=torch.float64, device=device), u0, du, nbin, mode)

    def _like(self, buf):
        return ObservedStack(buf, self.u0, self.du, self.nbin, self.mode)

    @property
    def bins(self):
        return (self.u0, self.du, self.nbin, self.mode)

    def _wave(self, k):
        u = self.u0 + self.du * k
        return np.power(10.0, u) if self.mode == "log" else u

    @property
    def wave_edges(self):
        """(nbin + 1,) float64 numpy: the bins' edges in Angstrom"""
        return self._wave(np.arange(self.nbin + 1, dtype=np.float64))

    @property
    def wave_centers(self):
        """(nbin,) float64 numpy: the bins' centres (of u) in Angstrom"""
        return self._wave(np.arange(self.nbin, dtype=np.float64) + 0.5)

    @property
    def sum_w(self):
        return self.buf[:, 0]

    @property
    def n(self):
        """(S, nbin) number of pixels stacked"""
        return self.buf[:, 3]

    def mean(self):
        """(S, nbin) weighted mean residual sum w r / sum w (NaN in an empty bin)"""
        return self.buf[:, 1] / self.buf[:, 0]

    def var(self):
        """(S, nbin) weighted variance of r inside the bin, sum w r^2 / sum w - mean^2"""
        m = self.mean()
        return self.buf[:, 2] / self.buf[:, 0] - m * m

    def err(self):
        """(S, nbin) standard error of ``mean()`` from the bin's own scatter: sqrt(var / (n - 1)), which is the error of a weighted
        mean whose weights are inverse variances up to one unknown scale; NaN where n < 2"""
        n = self.n
        return torch.sqrt(torch.clamp(self.var(), min=0.0) / torch.where(n > 1, n - 1, torch.full_like(n, float("nan"))))

    def _per_draw(self):
        return self.mean()

    def std_over_draws(self):
        """(nbin,) standard deviation of ``mean()`` over the S draws: the continuum posterior's error bar on the stack"""
        return self._draws("std_over_draws").std(0, unbiased=True)

    def _avg(self):
        """(4, nbin) float64 numpy: the sums averaged over the draws"""
        return self.buf.mean(0).cpu().numpy()

    @staticmethod
    def _box(x, half_width):
        """sums of x over [k - half_width, k + half_width], clipped at the ends"""
        hw, n = int(half_width), len(x)
        if hw < 0:
            raise QFAHipError(f"half_width = {half_width}, expected >= 0")
        c = np.concatenate([[0.0], np.cumsum(x)])
        k = np.arange(n)
        return c[np.minimum(k + hw + 1, n)] - c[np.maximum(k - hw, 0)]

    def calibration(self, half_width=10):
        """(nbin,) float64 numpy: the smooth calibration vector, sum w r over sum w, both summed over the bins [k - half_width,
        k + half_width]; NaN where that window holds no weight"""
        a = self._avg()
        sw, swr = self._box(a[0], half_width), self._box(a[1], half_width)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sw > 0.0, swr / np.where(sw > 0.0, sw, 1.0), np.nan)

    def chi2(self, about):
        """(nbin,) float64 numpy: the weighted scatter per pixel about ``about`` (a scalar or (nbin,)), (sum w r^2 - 2 a sum w r +
        a^2 sum w) / n; NaN in an empty bin"""
        s = self._avg()
        a = np.broadcast_to(np.asarray(about, dtype=np.float64), (self.nbin,))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(s[3] > 0.0, (s[2] - 2.0 * a * s[1] + a * a * s[0]) / np.where(s[3] > 0.0, s[3], 1.0), np.nan)

    def find_lines(self, min_count=50, chi2_ratio=3.0, max_dev=0.05, grow=1, half_width=10):
        """The bins to mask as float64 (n, 2) observed-frame intervals [lo, hi) in Angstrom -- what ``mask_absorbers(sky=...)`` and
        ``io.read_intervals`` take.  A bin is flagged when it holds at least ``min_count`` pixels (an eligible bin) and either its
        ``chi2`` about the smooth ``calibration(half_width)`` exceeds ``chi2_ratio`` times the median over the eligible bins, or its
        mean departs from the calibration by more than ``max_dev`` of it.  Flagged bins are grown by ``grow`` bins on both sides and
        merged.  The defaults suit a stack of some thousand spectra: 50 pixels make the scatter of a bin meaningful, a sky-line
        residual multiplies the scatter several times, and 5 % is beyond any calibration ripple."""
        s = self._avg()
        cal = self.calibration(half_width)
        chi = self.chi2(cal)
        ok = (s[3] >= float(min_count)) & np.isfinite(cal) & np.isfinite(chi)
        if not ok.any():
            return np.zeros((0, 2), dtype=np.float64)
        med = float(np.median(chi[ok]))
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = s[1] / s[0]
            flag = ok & ((chi > float(chi2_ratio) * med) | (np.abs(mean / cal - 1.0) > float(max_dev)))
        g = int(grow)
        if g < 0:
            raise QFAHipError(f"grow = {grow}, expected >= 0")
        grown = self._box(flag.astype(np.float64), g) > 0.0
        d = np.diff(np.concatenate([[0], grown.astype(np.int8), [0]]))
        lo, hi = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
        edges = self.wave_edges
        return np.stack([edges[lo], edges[hi]], axis=1).astype(np.float64).reshape(-1, 2)

    def table(self, half_width=10):
        """the calibration as ``calibrate`` and ``io.write_calibration`` take it: a dict u0, du, mode, cal"""
        return {"u0": self.u0, "du": self.du, "mode": self.mode, "cal": self.calibration(half_width)}

    def arrays(self):
        """what observed_stack.npz holds"""
        return self._export(wave_centers=self.wave_centers, wave_edges=self.wave_edges, mean=self.mean(), err=self.err(), n=self.n,
                            sums=self.buf, u0=self.u0, du=self.du, mode=self.mode)


def _table(t, half_width):
    if isinstance(t, ObservedStack):
        t = t.table(half_width)
    try:
        u0, du, mode, cal = float(t["u0"]), float(t["du"]), str(t["mode"]), np.ascontiguousarray(t["cal"], dtype=np.float64).reshape(-1)
    except (KeyError, TypeError, IndexError) as e:
        raise QFAHipError("calibrate: expected an ObservedStack or a table with u0, du, mode, cal") from e
    if len(cal) < 2:
        raise QFAHipError("calibrate: the calibration table needs at least two entries")
    _check_grid(u0, du, min(len(cal), MAX_BINS), mode)
    return u0, du, mode, cal


def calibrate(flux, error, zqso, wav_grid, table, *, half_width=10, c_min=0.1, out=None, device):
    """Divide N rest-frame spectra on ``wav_grid`` by a calibration vector (the rule: include/qfa_hip.h, ``qfa_calibrate_f32``).
    ``flux``, ``error`` (N, Npix) float32 with the -999 sentinels, ``zqso`` (N): host arrays or device tensors.  ``table``: an
    ``ObservedStack`` (its ``calibration(half_width)``) or a dict u0, du, mode, cal (``io.read_calibration``); the vector is
    interpolated linearly between the bin centres.  A valid pixel outside the table, or where the vector is not finite or below
    ``c_min``, is left as it is and counted.  ``out`` = (flux, error): two (N, Npix) float32 device tensors to fill, which may be the
    inputs themselves.  Returns ``(flux, error, n_uncal)``, ``n_uncal`` (N,) int32 on the device.  ``norm`` and ``snr`` of a
    preprocessed set are unchanged by a common factor and are not formed again."""
    from .preprocess import _dev
    device = torch.device(device)
    if device.type != "cuda":
        raise QFAHipError("calibrate needs a HIP device (torch device 'cuda'); qfa_amd has no CPU fallback")
    u0, du, mode, cal = _table(table, half_width)
    if not (float(c_min) > 0.0 and np.isfinite(float(c_min))):
        raise QFAHipError(f"c_min = {c_min}, must be positive and finite")
    f_d, e_d = _dev(flux, f32, device, "flux"), _dev(error, f32, device, "error")
    pix_u, spec_u = coordinates(wav_grid, zqso.detach().cpu().numpy() if isinstance(zqso, torch.Tensor) else zqso, mode)
    npix = len(pix_u)
    if f_d.ndim != 2 or f_d.shape[1] != npix or tuple(e_d.shape) != tuple(f_d.shape) or len(spec_u) != f_d.shape[0]:
        raise QFAHipError("flux / error must be (N, len(wav_grid)) and zqso (N,)")
    n = int(f_d.shape[0])
    if out is not None:
        fo, eo = out
        for t, name in ((fo, "out[0]"), (eo, "out[1]")):
            _lib.require_device_tensor(t, f32, name)
            if tuple(t.shape) != (n, npix) or t.device != f_d.device:
                raise QFAHipError(f"{name} must be ({n}, {npix}) on {f_d.device}")
    else:
        fo, eo = torch.empty_like(f_d), torch.empty_like(e_d)
    nu = torch.zeros((n,), dtype=torch.int32, device=device)
    dev_of = lambda x: torch.as_tensor(x, device=device)
    pu, su, cd = dev_of(pix_u), dev_of(spec_u), dev_of(cal)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().qfa_calibrate_f32(_ptr(f_d), _ptr(e_d), _ptr(pu), _ptr(su), n, npix, _ptr(cd), len(cal), u0, du,
                                                _lib.OBS_MODES[mode], float(c_min), _ptr(fo), _ptr(eo), _ptr(nu),
                                                _lib.current_stream(device)), "qfa_calibrate_f32")
    if out is not None:
        for t in out:                                          # written through raw pointers: tell torch
            torch.autograd.graph.increment_version(t)
    return fo, eo, nu


class ObservedFrame(object):
    """``observed_residuals`` / ``observed_stack``: a plain base class of ``qfa_amd.model.QFA`` that uses the model's plumbing as any
    other method of it does."""

    def observed_residuals(self, flux=None, error=None, mask=None, *, zqso, wav_grid, lam_min=None, nbin=None, dloglam=None, dlam=None,
                           rest_range=None, h=None, hmean=None, hcov=None, n_samples=0, seed=0, offset=0, unc=None, cont_min=0.0,
                           unit_weights=False, stack=None, zabs=None, zfac=None, batch=None):
        """One call of qfa_obs_stack_f32 on a batch: r = flux / continuum of every draw of the continuum, stacked in bins of
        observed wavelength (the contract is in include/qfa_hip.h).  ``zqso`` (B,) in batch order and ``wav_grid`` (Npix,) give the
        coordinate in float64.  The bins: ``stack`` -- an ``ObservedStack`` to ADD to -- or ``lam_min``, ``nbin`` and ``dloglam``
        (bins of log10 lambda) or ``dlam`` (bins of lambda).  ``rest_range`` = (lo, hi) in Angstrom restricts the stacked pixels
        to lo <= wav_grid < hi (the red side: (1216, inf)); default all.  The latent (``QFA._resolve_latent``): ``h`` |
        ``hmean`` | ``hmean`` + ``hcov`` + ``n_samples``, else ``predict`` runs on the inputs first and its ``unc`` enters the
        weights when S = 1.  Every input form of a batch: the tensors (``zabs`` or ``zfac`` only serve that ``predict``), or
        ``batch`` = a ``ResidentBatch``.  Returns the ``ObservedStack``."""
        if self.mu is None:
            raise QFAHipError("observed_residuals needs model.mu (load_from_npz or train first)")
        dev = self.device
        self._params_struct()
        if stack is not None:
            if not isinstance(stack, ObservedStack):
                raise QFAHipError("observed_residuals(stack=...): expected an ObservedStack")
            u0, du, nb, mode = stack.bins
            if lam_min is not None and obs_grid(lam_min, nb if nbin is None else nbin, dloglam, dlam) != stack.bins:
                raise QFAHipError("observed_residuals(stack=...): the stack's bins differ from the ones asked for")
        else:
            if lam_min is None or nbin is None:
                raise QFAHipError("observed_residuals: give stack=, or lam_min, nbin and dloglam or dlam")
            u0, du, nb, mode = obs_grid(lam_min, nbin, dloglam, dlam)
        if batch is not None:
            B = batch.B
        else:
            if not isinstance(flux, torch.Tensor) or flux.dim() != 2:
                raise QFAHipError("observed_residuals: flux must be a (B, Npix) tensor")
            B = int(flux.shape[0])
            for t, name in ((flux, "flux"), (error, "error"), (mask if mask is not None else flux, "mask")):
                if tuple(t.shape) != (B, self.Npix):
                    raise QFAHipError(f"{name}: shape {tuple(t.shape)}, expected ({B}, {self.Npix})")
        h, S, unc = self._resolve_latent("observed_residuals", B, h=h, hmean=hmean, hcov=hcov, n_samples=n_samples, seed=seed,
                                         offset=offset, unc=unc,
                                         predict_inputs=dict(flux=flux, error=error, zabs=zabs, mask=mask, zfac=zfac, batch=batch))
        bs, keep = self._batch_struct_rows(batch, raw_flux=True) if batch is not None else self._flux_batch(flux, error, mask)
        bs.A_blue = bs.zabs = bs.zq1 = bs.pix_ratio = None      # (not read by the call)
        ph = _lib.require_device_tensor(h, f32, "h")
        pu = None
        if unc is not None:
            if tuple(unc.shape) != (B, self.Npix):
                raise QFAHipError(f"unc: shape {tuple(unc.shape)}, expected ({B}, {self.Npix})")
            pu = _lib.require_device_tensor(unc, f32, "unc")
        if stack is None:
            stack = ObservedStack.zeros(S, u0, du, nb, mode, dev)
        elif stack.S != S:
            raise QFAHipError(f"observed_residuals(stack=...): the stack has {stack.S} draws, the call {S}")
        _lib.require_device_tensor(stack.buf, torch.float64, "stack")
        zq = zqso.detach().cpu().numpy() if isinstance(zqso, torch.Tensor) else zqso
        pix_u, spec_u = coordinates(wav_grid, zq, mode)
        if len(pix_u) != self.Npix or len(spec_u) != B:
            raise QFAHipError(f"wav_grid ({len(pix_u)},) / zqso ({len(spec_u)},): expected ({self.Npix},) and ({B},)")
        grid = np.asarray(wav_grid, dtype=np.float64).reshape(-1)
        lo, hi = (-np.inf, np.inf) if rest_range is None else (float(rest_range[0]), float(rest_range[1]))
        ob = _lib.ObsBins(u0, du, nb, int(np.searchsorted(grid, lo, side="left")), int(np.searchsorted(grid, hi, side="left")),
                          _lib.OBS_MODES[mode])
        ob.p_hi = max(ob.p_lo, ob.p_hi)
        pix_d, spec_d = torch.as_tensor(pix_u, device=dev), torch.as_tensor(spec_u, device=dev)
        mu = self.mu.to(device=dev, dtype=f32).contiguous()
        need = _lib.lib().qfa_obs_stack_workspace_bytes(B, S, self.Npix, self.Nh, nb)
        if need == 0:
            raise QFAHipError(f"observed_residuals: unsupported shape B={B} S={S} Npix={self.Npix} Nh={self.Nh} nbin={nb}")
        ws = self._scratch("obs_ws", need)
        _lib.check(_lib.lib().qfa_obs_stack_f32(
            _lib.require_device_tensor(self.F, f32, "F"), _ptr(mu), C.byref(bs), ph, pu, _ptr(pix_d), _ptr(spec_d), B, S, self.Npix,
            self.Nh, C.byref(ob), float(cont_min), _lib.F_OBS_UNIT_W if unit_weights else 0, _ptr(stack.buf), _ptr(ws), ws.numel(),
            _lib.current_stream(dev)), "qfa_obs_stack_f32")
        del keep
        return stack

    def observed_stack(self, dataloader, lam_min, nbin, dloglam=None, dlam=None, rest_range=None, n_samples=0, seed=0, batch_size=4096,
                       cont_min=0.0, unit_weights=False):
        """The observed-frame residual stack of a whole dataloader: an ``ObservedStack`` of S = max(1, n_samples) draws.  It walks
        the loader the way ``mean_transmission`` does (the resident rows form when the loader has one) and takes the redshifts and
        the grid from the loader's ``zqso`` and ``wav_grid``.  Under data parallelism the sums are all-reduced over the model's
        group: every rank returns the global stack."""
        if not (hasattr(dataloader, "zqso") and hasattr(dataloader, "wav_grid")):
            raise QFAHipError("observed_stack: the dataloader must carry zqso and wav_grid (a DeviceDataloader)")
        u0, du, nb, mode = obs_grid(lam_min, nbin, dloglam, dlam)
        S = max(1, int(n_samples))
        stack = ObservedStack.zeros(S, u0, du, nb, mode, self.device)
        zq = np.asarray(dataloader.zqso, dtype=np.float64).reshape(-1)
        row0 = int(getattr(dataloader, "_row0", 0))
        for s, inputs, _ in self._loader_slices(dataloader, int(batch_size)):
            B = inputs["batch"].B if "batch" in inputs else int(inputs["flux"].shape[0])
            _, hmean, hcov, _, unc = self.predict(**inputs)
            self.observed_residuals(**inputs, zqso=zq[s:s + B], wav_grid=dataloader.wav_grid, hmean=hmean, hcov=hcov,
                                    n_samples=int(n_samples), seed=seed, offset=row0 + s, unc=unc if int(n_samples) == 0 else None,
                                    rest_range=rest_range, cont_min=cont_min, unit_weights=unit_weights, stack=stack)
        if self._dp:
            stack.all_reduce(self._dp_group)
        return stack
