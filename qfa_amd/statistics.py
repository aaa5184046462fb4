"""The forest statistics of ``QFA``: transmission and its redshift-binned stack (``forest`` / ``mean_transmission``), the 1D flux
power spectrum (``p1d`` / ``flux_power``), its band powers (``p1d_bands`` / ``band_power``), the line-of-sight correlation function
(``xi`` / ``flux_correlation``), the flux PDF (``flux_pdf_segments`` / ``flux_pdf``) and the variance function
(``variance_segments`` / ``variance_function``), and the sightline bootstrap of the segment statistics (``segment_codes``,
``segment_bootstrap`` / ``bootstrap``).  ``ForestStatistics`` is a plain
base class of ``qfa_amd.model.QFA`` and uses the model's plumbing (``_batch_struct*``, ``_scratch``, ``predict``, ``sample_latent``,
``_loader_slices``) as any other method of it does; every call goes through the C-ABI in ``include/qfa_hip.h``."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import types

import numpy as np
import torch

from . import _lib
from ._lib import QFAHipError, _ptr
from .stacks import BootstrapStack, ForestStack, P1DBandStack, P1DStack, PDFStack, VarianceStack, XiStack, _band_map, _check_segments, _edges, _mode_k, _window2

f32 = torch.float32

# what `_power_of_loader` needs to know of a statistic: zeros(S, z0, dz, nz, L, dv) makes its stack -- and with it checks the
# statistic's parameters, before the first slice --, ``call`` is its method of a slice with its own ``keywords``, ``needs_dv`` False: dv
# matters only where <T> is made in the loop's own `mean_transmission`
_LoaderStat = collections.namedtuple("_LoaderStat", "zeros call keywords needs_dv", defaults=(True,))

# what `bootstrap` needs to know of a statistic: its loader method, the (B, S, nseg, W) rows of its slice call's outputs, and
# (W, the stack class's map from bootstrap sums to the estimate) of its stack
_BOOT_STATS = {
    "p1d": ("flux_power", lambda o: torch.cat([o[1].unsqueeze(-1), o[0]], -1),
            lambda st: (1 + st.M, functools.partial(P1DStack.bootstrap_estimate, dv=st.dv))),
    "bands": ("band_power", lambda o: o[0], lambda st: (st.nband, P1DBandStack.bootstrap_estimate)),
    "xi": ("flux_correlation", lambda o: torch.cat([o[1].unsqueeze(-1), o[0].flatten(3)], -1),
           lambda st: (1 + 2 * st.nlag, functools.partial(XiStack.bootstrap_estimate, nlag=st.nlag))),
    "pdf": ("flux_pdf", lambda o: o[0], lambda st: (st.nt, functools.partial(PDFStack.bootstrap_estimate, dt=st.dt))),
    "variance": ("variance_function", lambda o: o[0].flatten(3),
                 lambda st: (5 * st.nv, functools.partial(VarianceStack.bootstrap_estimate, nv=st.nv))),
}


def _p1d_params(tbar_bins, St, p_lo, L, nseg, min_used, stack):
    """qfa_p1d_t of `p1d`, `p1d_bands`, `xi`, `flux_pdf_segments` and `variance_segments`: the bins of tbar, the segments and the z-bins of ``stack`` (None: one unused bin)"""
    pp = _lib.P1DParams()
    pp.zT0, pp.dzT, pp.nT = ForestStack._round_bins(tbar_bins[0], tbar_bins[1], tbar_bins[2])
    pp.St = St
    pp.p_lo, pp.seg_len, pp.nseg, pp.min_used = p_lo, L, nseg, int(min_used)
    pp.z0, pp.dz, pp.nz = stack.bins if stack is not None else (0.0, 1.0, 1)
    return pp


class ForestStatistics(object):

    # ------------------------------------------------------------------ forest transmission
    def forest(self, flux=None, error=None, zabs=None, mask=None, *, h=None, hmean=None, hcov=None, n_samples=0, seed=0, offset=0,
               unc=None, bins=None, cont_min=0.0, pixel_range=None, unit_weights=False, stack=None, zfac=None, batch=None,
               return_pixels=True):
        """Lyman-alpha forest transmission T = flux / continuum on the blue side and its redshift-binned stack, for every draw of
        the continuum, without writing a continuum (qfa_forest_f32; the contract is in include/qfa_hip.h).
        The latent: ``h`` (B, S, Nh) as it is; else ``hmean`` alone (or with ``hcov`` and ``n_samples`` = 0): the posterior-mean
        continuum, S = 1; else ``hmean`` + ``hcov`` + ``n_samples`` > 0 through ``sample_latent`` (``seed``, ``offset`` = the
        global row of spectrum 0); with none of them ``predict`` runs on the inputs first, and its ``unc`` -- the continuum's
        1 sigma, which enters ivar -- is passed on when S = 1.  ``bins`` = (z0, dz, nbin) asks for the stack; ``stack``: a
        ``ForestStack`` to ADD to (its bins are used).  ``pixel_range`` = (p_lo, p_hi) restricts the stacked blue pixels,
        ``unit_weights`` stacks with w = 1 instead of w = ivar, ``cont_min``: pixels whose continuum is not above it are unused.
        ``mask`` None: every pixel is used.  A zabs tensor is read as given (never swapped for derived factors: the bins are
        defined bit for bit by z).  Returns (trans, ivar, stack): (B, S, Nb) float32 each (None with ``return_pixels`` False) and
        the ``ForestStack`` (None when neither ``bins`` nor ``stack`` was given)."""
        if self.mu is None:
            raise QFAHipError("forest needs model.mu (load_from_npz or train first)")
        if int(n_samples) < 0:
            raise QFAHipError(f"forest: n_samples = {n_samples}, expected >= 0")
        if bins is None and stack is None and not return_pixels:
            raise QFAHipError("forest: nothing asked for (no bins, no stack, return_pixels = False)")
        dev = self.device
        self._params_struct()                                   # (F as a contiguous float32 device tensor)
        if batch is not None:
            B = batch.B
        else:
            if not isinstance(flux, torch.Tensor) or flux.dim() != 2:
                raise QFAHipError("forest: flux must be a (B, Npix) tensor")
            B = self._check_batch_shapes(flux, error, zabs, mask if mask is not None else flux)
        h, S, unc = self._resolve_latent("forest", B, h=h, hmean=hmean, hcov=hcov, n_samples=n_samples, seed=seed, offset=offset, unc=unc,
                                         predict_inputs=dict(flux=flux, error=error, zabs=zabs, mask=mask, zfac=zfac, batch=batch))
        if batch is not None:
            bs, keep = self._batch_struct_rows(batch, raw_flux=True)
        else:
            bs, keep = self._batch_struct(flux, error, zabs, mask, zfac, allow_no_mask=True, auto_factor=False)
        bs.A_blue = None                                        # (not read by the call)
        ph = _lib.require_device_tensor(h, f32, "h")
        pu = None
        if unc is not None:
            if tuple(unc.shape) != (B, self.Npix):
                raise QFAHipError(f"unc: shape {tuple(unc.shape)}, expected ({B}, {self.Npix})")
            pu = _lib.require_device_tensor(unc, f32, "unc")
        if stack is not None:
            if not isinstance(stack, ForestStack) or stack.S != S or (bins is not None and ForestStack._round_bins(*bins) != stack.bins):
                raise QFAHipError(f"forest(stack=...): expected a ForestStack of {S} draws on the same bins")
            _lib.require_device_tensor(stack.buf, torch.float64, "stack")
        elif bins is not None:
            stack = ForestStack.zeros(S, bins[0], bins[1], bins[2], dev)
        fb = _lib.ForestBins()
        fb.z0, fb.dz, fb.nbin = stack.bins if stack is not None else (0.0, 1.0, 1)
        p_lo, p_hi = (0, self.Nb) if pixel_range is None else (int(pixel_range[0]), int(pixel_range[1]))
        if not 0 <= p_lo <= p_hi <= self.Nb:
            raise QFAHipError(f"forest: pixel_range = {pixel_range}, expected 0 <= p_lo <= p_hi <= {self.Nb}")
        fb.p_lo, fb.p_hi = p_lo, p_hi
        trans = ivar = None
        if return_pixels:
            trans = torch.empty((B, S, self.Nb), dtype=f32, device=dev)
            ivar = torch.empty((B, S, self.Nb), dtype=f32, device=dev)
        mu = self.mu.to(device=dev, dtype=f32).contiguous()
        need = _lib.lib().qfa_forest_workspace_bytes(B, S, self.Npix, self.Nb, self.Nh, int(fb.nbin))
        if need == 0:
            raise QFAHipError(f"forest: unsupported shape B={B} S={S} Npix={self.Npix} Nb={self.Nb} Nh={self.Nh} nbin={fb.nbin}")
        ws = self._scratch("forest_ws", need)
        _lib.check(_lib.lib().qfa_forest_f32(
            _lib.require_device_tensor(self.F, f32, "F"), _ptr(mu), C.byref(bs), ph, pu, B, S, self.Npix, self.Nb, self.Nh,
            C.byref(fb), float(cont_min), _lib.F_FOREST_UNIT_W if unit_weights else 0, _ptr(trans), _ptr(ivar),
            _ptr(stack.buf) if stack is not None else None, _ptr(ws), ws.numel(), _lib.current_stream(dev)), "qfa_forest_f32")
        return trans, ivar, stack

    def mean_transmission(self, dataloader, z_min, z_max, n_bins, n_samples=0, seed=0, batch_size=4096, cont_min=0.0,
                          pixel_range=None, unit_weights=False):
        """The stacked forest transmission of a whole dataloader in ``n_bins`` bins of [z_min, z_max): a ``ForestStack`` of S =
        max(1, n_samples) draws.  ``n_samples`` = 0 stacks the posterior-mean continuum (``predict``'s unc enters the weights);
        ``n_samples`` > 0 repeats the stack over that many posterior draws of every continuum (``std_over_draws``: the
        continuum's error bar on the stack).  It walks the loader the way ``predict_to_npz`` does (the resident rows form when
        the loader has one); the global row of a spectrum is its dataloader index, so the result does not depend on
        ``batch_size`` beyond the rounding of float64 sums.  Under data parallelism the sums are all-reduced over the model's
        group: every rank returns the global stack."""
        n_bins, S = int(n_bins), max(1, int(n_samples))
        if n_bins < 1 or not float(z_max) > float(z_min):
            raise QFAHipError(f"mean_transmission: bins [{z_min}, {z_max}) / {n_bins}")
        stack = ForestStack.zeros(S, z_min, (float(z_max) - float(z_min)) / n_bins, n_bins, self.device)
        row0 = int(getattr(dataloader, "_row0", 0))              # (a data-parallel loader: the global index of its first row)
        for s, inputs, _ in self._loader_slices(dataloader, int(batch_size)):
            _, hmean, hcov, _, unc = self.predict(**inputs)
            self.forest(**inputs, hmean=hmean, hcov=hcov, n_samples=int(n_samples), seed=seed, offset=row0 + s,
                        unc=unc if int(n_samples) == 0 else None, cont_min=cont_min, pixel_range=pixel_range,
                        unit_weights=unit_weights, stack=stack, return_pixels=False)
        if self._dp:
            stack.all_reduce(self._dp_group)
        return stack

    # ------------------------------------------------------------------ 1D flux power spectrum
    P1D_PAIR_BYTES = 1 << 30    # flux_power: the most the (B, S_chunk, Nb) trans / ivar pair of a slice may take

    def _p1d_inputs(self, what, asked, trans, ivar, zabs, zfac, batch, tbar, tbar_bins):
        """the checks and conversions `p1d`, `p1d_bands`, `xi`, `flux_pdf_segments` and `variance_segments` share: (B, S, tbar (St, nT)
        float32, St, tbar_bins, qfa_batch_t, the tensors it points into); ``asked``: whether the call has an output at all"""
        dev = self.device
        if not asked:
            raise QFAHipError(what + ": nothing asked for (no bins, no stack, return_segments = False)")
        if not isinstance(trans, torch.Tensor) or trans.dim() != 3 or trans.shape[2] != self.Nb or tuple(ivar.shape) != tuple(trans.shape):
            raise QFAHipError(f"{what}: trans / ivar must be (B, S, {self.Nb}) tensors")
        B, S = int(trans.shape[0]), int(trans.shape[1])
        if isinstance(tbar, ForestStack):
            if tbar.S not in (1, S):
                raise QFAHipError(f"{what}: tbar has {tbar.S} draws, expected 1 or {S}")
            tbar_bins, tbar = tbar.bins, tbar.mean
        if tbar_bins is None:
            raise QFAHipError(what + ": a tbar tensor needs tbar_bins = (z0, dz, nT)")
        tbar = tbar.to(device=dev, dtype=f32).reshape(-1, int(tbar_bins[2])).contiguous()
        St = int(tbar.shape[0])
        if St not in (1, S):
            raise QFAHipError(f"{what}: tbar has {St} rows, expected 1 or {S}")
        if batch is not None:
            if batch.B != B:
                raise QFAHipError(f"{what}: resident batch of {batch.B} spectra, trans has {B}")
            bs, keep = self._batch_struct_rows(batch, need_src=False)
        else:
            if zabs is None and zfac is None:
                raise QFAHipError(what + ": pass zabs, zfac = (zq1, pix_ratio) or batch")
            bs, keep = _lib.Batch(), []
            bs.row_stride = 0
            # `_batch_struct`'s rule, so that p1d bins on the very z `forest` and `mean_transmission` binned on
            self._redshift_form(bs, keep, B, zabs, zfac)
        return B, S, tbar, St, tbar_bins, bs, keep

    def _segment_call(self, what, name, inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack, *, cls, same, zeros, expected,
                      own=None):
        """what `p1d`, `p1d_bands`, `xi`, `flux_pdf_segments` and `variance_segments` share behind ``inp`` = `_p1d_inputs`' result: ``stack`` is checked (a
        ``cls`` of S draws and segments of L pixels on the same bins for which ``same(stack)`` holds, else the error ends in
        ``expected``) or made by ``zeros()`` when ``bins`` asks for one; ``own(stack)`` -> (the statistic's own size, its note in the
        error of an unsupported shape, its parameter struct); qfa_p1d_t; the workspace of ``name``_workspace_bytes.  Returns
        (stack, call): call(flags, *outputs) runs ``name``_f32 with the outputs between the flags and the stack."""
        B, S, tbar, St, tbar_bins, bs, keep = inp
        dev = self.device
        if stack is not None:
            if not isinstance(stack, cls) or stack.S != S or stack.L != L or not same(stack) or \
                    (bins is not None and cls._round_bins(bins[0], bins[1], bins[2]) != stack.bins):
                raise QFAHipError(f"{what}(stack=...): expected a {cls.__name__} of {S} draws{expected}")
            _lib.require_device_tensor(stack.buf, torch.float64, "stack")
        elif bins is not None:
            stack = zeros()
        size, note, prm = own(stack) if own is not None else ((), "", None)
        pp = _p1d_params(tbar_bins, St, int(pixel_start), L, nseg, min_used, stack)
        h = _lib.lib()
        need = getattr(h, name + "_workspace_bytes")(B * S, S, self.Nb, L, nseg, int(pp.nz), *size) if L >= 1 and nseg >= 1 else 0
        if need == 0:
            raise QFAHipError(f"{what}: unsupported shape B={B} S={S} Nb={self.Nb} seg_len={L} n_segments={nseg} nz={pp.nz}{note}")
        ws = self._scratch("p1d_ws", need)                        # (one for the five calls: they own it only while they run)

        def call(flags, *outputs):
            _lib.check(getattr(h, name + "_f32")(
                _lib.require_device_tensor(trans, f32, "trans"), _lib.require_device_tensor(ivar, f32, "ivar"), C.byref(bs),
                _ptr(tbar), B, S, self.Nb, C.byref(pp), *(() if prm is None else (C.byref(prm),)), flags, *(_ptr(o) for o in outputs),
                _ptr(stack.buf) if stack is not None else None, _ptr(ws), ws.numel(), _lib.current_stream(dev)), name + "_f32")
        return stack, call

    def p1d(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments, pixel_start=0,
            min_used, bins=None, stack=None, return_segments=True, dv=1.0):
        """The 1D flux power spectrum of forest segments and its (k, z) stack (qfa_p1d_f32; the contract is in include/qfa_hip.h).
        ``trans``, ``ivar`` (B, S, Nb) as ``forest`` returns them; the redshift of the pixels from ``zabs`` (B, Nb), ``zfac`` =
        (zq1, pix_ratio) or a resident ``batch``.  ``tbar``: the mean transmission the contrast delta_F = T / tbar - 1 is formed
        with -- a ``ForestStack`` (its ``mean`` per draw: one row per draw when it has S draws, else its single row for every
        draw) or a (St, nT) / (nT,) tensor over ``tbar_bins`` = (z0, dz, nT).  Segment g holds the ``seg_len`` pixels from
        ``pixel_start`` + g ``seg_len`` on and is used when at least ``min_used`` of them are.  ``bins`` = (z0, dz, nz) asks for
        the stack (``dv``: the pixel width in km/s it reports k and P in); ``stack``: a ``P1DStack`` to ADD to.  Returns
        (power (B, S, n_segments, M), noise (B, S, n_segments), stack): float32 P_m = |delta~_m|^2 / L for m = 1 .. M = seg_len // 2
        and the noise level, both in pixel units (None with ``return_segments`` False), and the ``P1DStack`` (or None)."""
        inp = self._p1d_inputs("p1d", bins is not None or stack is not None or return_segments, trans, ivar, zabs, zfac, batch, tbar,
                               tbar_bins)
        B, S, L, nseg, dev = inp[0], inp[1], int(seg_len), int(n_segments), self.device
        stack, call = self._segment_call("p1d", "qfa_p1d", inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack, cls=P1DStack,
                                         same=lambda st: True, zeros=lambda: P1DStack.zeros(S, bins[0], bins[1], bins[2], L, dv, dev),
                                         expected=f" and segments of {L} pixels on the same bins")
        power = noise = None
        if return_segments:
            power = torch.empty((B, S, nseg, L // 2), dtype=f32, device=dev)
            noise = torch.empty((B, S, nseg), dtype=f32, device=dev)
        call(0, power, noise)
        return power, noise, stack

    def _p1d_band_tables(self, L, dv, k_edges, resolution_kms):
        """(band (M,) int32, weight (M,) float32) of qfa_p1d_band_t on the device, built once per (L, dv, k_edges, resolution):
        weight_m = dv / (n_a W^2(k_m)) with n_a the number of modes of the band of mode m and W^2 = ``P1DStack.window2`` (1 without
        a resolution), so that Q_a is the mean over the band's modes of the P1D in km/s"""
        key = (int(L), float(dv), _edges(k_edges), None if resolution_kms is None else float(resolution_kms))
        cache = self._p1d_band_cache
        if key not in cache:
            _check_segments("p1d_bands", L, dv)
            band, count = _band_map(L, dv, key[2])
            w = np.full(len(band), float(dv), np.float64) / np.maximum(count[np.maximum(band, 0)], 1)
            if resolution_kms is not None:
                w = w / _window2(_mode_k(L, dv), float(dv), resolution_kms)
            w = np.where(band >= 0, w, 0.0).astype(np.float32)
            if len(cache) >= 16:
                cache.clear()
            # (one entry more than the modes: a pointer to an empty tensor would be NULL at L = 1)
            cache[key] = (torch.tensor(np.append(band, np.int32(-1)), device=self.device),
                          torch.tensor(np.append(w, np.float32(0.0)), device=self.device))
        return cache[key]

    def p1d_bands(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments, pixel_start=0,
                  min_used, bins=None, dv=1.0, k_edges, resolution_kms=None, subtract_noise=True, stack=None,
                  return_segments=False):
        """Band powers of the forest's P1D and the stack their covariance matrix comes from (qfa_p1d_band_f32; the contract is in
        include/qfa_hip.h).  The inputs and keywords of ``p1d``; ``k_edges``: nband + 1 increasing band edges in s/km -- band a
        holds the modes with k_edges[a] <= 2 pi m / (seg_len dv) < k_edges[a + 1].  Q_a of a segment is the mean over the band's
        modes of (P_m - N) dv / W^2(k_m): ``subtract_noise`` False keeps the noise in, ``resolution_kms`` divides by
        ``P1DStack.window2``.  ``bins`` = (z0, dz, nz) asks for the stack, ``stack``: a ``P1DBandStack`` to ADD to.  Returns
        (bandpower (B, S, n_segments, nband) float64, or None without ``return_segments``; the ``P1DBandStack``, or None)."""
        inp = self._p1d_inputs("p1d_bands", bins is not None or stack is not None or return_segments, trans, ivar, zabs, zfac, batch, tbar,
                               tbar_bins)
        B, S, L, nseg, dev = inp[0], inp[1], int(seg_len), int(n_segments), self.device

        def own(st):
            nband, qq = len(_edges(k_edges)) - 1, _lib.P1DBandParams()
            band, weight = self._p1d_band_tables(L, dv if st is None else st.dv, k_edges, resolution_kms)
            qq.nband, qq.band, qq.weight, qq.subtract_noise = nband, band.data_ptr(), weight.data_ptr(), 1 if subtract_noise else 0
            return (nband,), f" nband={nband}", qq

        stack, call = self._segment_call("p1d_bands", "qfa_p1d_band", inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack,
                                         cls=P1DBandStack, same=lambda st: st._k_edges == _edges(k_edges),
                                         zeros=lambda: P1DBandStack.zeros(S, bins[0], bins[1], bins[2], L, dv, k_edges, dev),
                                         expected=f" and segments of {L} pixels on the same bins and bands", own=own)
        bandpower = torch.empty((B, S, nseg, len(_edges(k_edges)) - 1), dtype=torch.float64, device=dev) if return_segments else None
        call(0, bandpower)
        return bandpower, stack

    def xi(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments, pixel_start=0, min_used,
           n_lags, sigma2_lss=0.0, unit_weights=False, bins=None, stack=None, return_segments=True, dv=1.0):
        """The pair-weighted correlation function of forest segments along the line of sight and its (lag, z) stack (qfa_xi_f32; the
        contract is in include/qfa_hip.h).  The inputs and keywords of ``p1d``: the same pixels are used, the same segments valid and
        binned in z.  Per segment and lag l < ``n_lags`` (<= seg_len): W_l = sum_j w_j w_{j+l} and A_l = sum_j w_j w_{j+l} d_j d_{j+l}
        with d = T / tbar - 1 and w = 1 / (v + ``sigma2_lss``), v the pixel's noise variance of d (``unit_weights``: w = 1 on every
        used pixel); an unused pixel has w = 0 and drops out of both, so the ratio carries no window of the mask.  ``bins`` =
        (z0, dz, nz) asks for the stack (``dv``: the pixel width in km/s it reports the lags in); ``stack``: a ``XiStack`` to ADD
        to.  Returns (pairs (B, S, n_segments, 2, n_lags) float32 = [W_l | A_l], noise0 (B, S, n_segments) float32 = sum_j w_j^2 v_j,
        the noise in A_0 -- both None with ``return_segments`` False -- and the ``XiStack`` (or None))."""
        inp = self._p1d_inputs("xi", bins is not None or stack is not None or return_segments, trans, ivar, zabs, zfac, batch, tbar, tbar_bins)
        B, S, dev = inp[0], inp[1], self.device
        L, nseg, s2 = int(seg_len), int(n_segments), float(sigma2_lss)
        nlag = XiStack.lag_params(L, n_lags)
        if not (s2 >= 0.0 and np.isfinite(s2)):
            raise QFAHipError(f"xi: sigma2_lss = {sigma2_lss}")
        stack, call = self._segment_call("xi", "qfa_xi", inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack, cls=XiStack,
                                         same=lambda st: st.nlag == nlag,
                                         zeros=lambda: XiStack.zeros(S, bins[0], bins[1], bins[2], L, nlag, dv, dev),
                                         expected=f", segments of {L} pixels and {nlag} lags on the same bins",
                                         own=lambda st: ((nlag,), f" n_lags={nlag}", _lib.XiParams(nlag, s2)))
        pairs = noise0 = None
        if return_segments:
            pairs = torch.empty((B, S, nseg, 2, nlag), dtype=f32, device=dev)
            noise0 = torch.empty((B, S, nseg), dtype=f32, device=dev)
        call(_lib.F_XI_UNIT_W if unit_weights else 0, pairs, noise0)
        return pairs, noise0, stack

    @staticmethod
    def _flux_params(t_min, t_max, n_tbins, relative, clamp, ivar_min):
        """`PDFStack.flux_params` of ``n_tbins`` equal bins of [t_min, t_max): an empty or unbounded range has no valid step"""
        return PDFStack.flux_params(t_min, (float(t_max) - float(t_min)) / max(1, int(n_tbins)), n_tbins, relative, clamp, ivar_min)

    def flux_pdf_segments(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments,
                          pixel_start=0, min_used, t_min, t_max, n_tbins, relative=False, clamp=False, ivar_min=0.0, bins=None,
                          stack=None, return_segments=True):
        """The flux PDF of forest segments and the stack its covariance comes from (qfa_flux_pdf_f32; the contract is in
        include/qfa_hip.h).  The inputs and keywords of ``p1d``: the same pixels are used, the same segments valid and binned in z.
        Per segment h_a = the number of counted pixels (used, with ivar >= ``ivar_min``) whose x = T -- or, with ``relative``,
        x = T / tbar(z) -- falls in flux bin a of the ``n_tbins`` (<= 64) equal bins of [``t_min``, ``t_max``); an edge belongs to
        the bin above it.  ``clamp`` counts x below the range in the first bin and above it in the last (the convention of the
        published PDFs); without it such pixels are in no bin.  ``bins`` = (z0, dz, nz) asks for the stack, ``stack``: a
        ``PDFStack`` to ADD to.  Returns (hist (B, S, n_segments, n_tbins) int32, or None with ``return_segments`` False; the
        ``PDFStack``, or None).  The counts are integers: the stack is exact, whatever the order and the split of the calls."""
        inp = self._p1d_inputs("flux_pdf_segments", bins is not None or stack is not None or return_segments, trans, ivar, zabs, zfac,
                               batch, tbar, tbar_bins)
        B, S, dev = inp[0], inp[1], self.device
        L, nseg = int(seg_len), int(n_segments)
        want = self._flux_params(t_min, t_max, n_tbins, relative, clamp, ivar_min)
        t0, dt, nt, _, _, imin = want
        stack, call = self._segment_call(
            "flux_pdf_segments", "qfa_flux_pdf", inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack, cls=PDFStack,
            same=lambda st: st.flux_bins + (st.relative, st.clamp, st.ivar_min) == want,
            zeros=lambda: PDFStack.zeros(S, bins[0], bins[1], bins[2], L, *want, dev),
            expected=f" and segments of {L} pixels on the same z-bins, flux bins, flags and ivar_min",
            own=lambda st: ((nt,), f" n_tbins={nt}", _lib.PDFParams(t0, dt, nt, imin)))
        hist = torch.empty((B, S, nseg, nt), dtype=torch.int32, device=dev) if return_segments else None
        call((_lib.F_PDF_RELATIVE if relative else 0) | (_lib.F_PDF_CLAMP if clamp else 0), hist)
        return hist, stack

    def variance_segments(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments,
                          pixel_start=0, min_used, e_lo, n_oct, sub=1, d_max=None, bins=None, stack=None, return_segments=False):
        """The moments of delta_F of forest segments in bins of the pipeline's noise variance, and their (v-bin, z) stack
        (qfa_variance_f32; the contract is in include/qfa_hip.h).  The inputs and keywords of ``p1d``: the same pixels are used, the
        same segments valid and binned in z.  The nv = ``n_oct`` << ``sub`` (<= 64) bins of v = 1 / (ivar tbar^2) are defined on the
        bits of the float32 v: 2^sub bins per octave from 2^``e_lo`` on (``VarianceStack.v_edges``).  A used pixel of a valid segment
        is counted when its v falls in a bin and |d| <= ``d_max`` (None: only non-finite d are cut).  ``bins`` = (z0, dz, nz) asks for
        the stack, ``stack``: a ``VarianceStack`` to ADD to.  Returns (moments (B, S, n_segments, 5, nv) float64 = [n_a | sum v |
        sum d | sum d^2 | sum d^4], or None without ``return_segments``; the ``VarianceStack``, or None)."""
        inp = self._p1d_inputs("variance_segments", bins is not None or stack is not None or return_segments, trans, ivar, zabs, zfac,
                               batch, tbar, tbar_bins)
        B, S, dev = inp[0], inp[1], self.device
        L, nseg = int(seg_len), int(n_segments)
        want = VarianceStack.var_params(e_lo, n_oct, sub, d_max)
        nv = want[1] << want[2]
        stack, call = self._segment_call(
            "variance_segments", "qfa_variance", inp, trans, ivar, L, nseg, pixel_start, min_used, bins, stack, cls=VarianceStack,
            same=lambda st: st.var_bins == want,
            zeros=lambda: VarianceStack.zeros(S, bins[0], bins[1], bins[2], L, *want, dev),
            expected=f" and segments of {L} pixels on the same z-bins, variance bins and d_max",
            own=lambda st: ((nv,), f" nv={nv}", _lib.VarParams(*want)))
        moments = torch.empty((B, S, nseg, 5, nv), dtype=torch.float64, device=dev) if return_segments else None
        call(0, moments)
        return moments, stack

    # ------------------------------------------------------------------ sightline bootstrap
    def segment_codes(self, trans, ivar, *, zabs=None, zfac=None, batch=None, tbar, tbar_bins=None, seg_len, n_segments, pixel_start=0,
                      min_used, bins):
        """The z-bin of every segment as ``p1d`` and the other segment statistics stack it (qfa_segment_codes_f32; the contract is in
        include/qfa_hip.h): the inputs and keywords of ``p1d``, ``bins`` = (z0, dz, nz).  Returns codes (B, S, n_segments) int32: the
        z-bin of a valid segment inside the bins, else -1."""
        inp = self._p1d_inputs("segment_codes", True, trans, ivar, zabs, zfac, batch, tbar, tbar_bins)
        B, S, tb, St, tbar_bins, bs, keep = inp
        L, nseg = int(seg_len), int(n_segments)
        pp = _p1d_params(tbar_bins, St, int(pixel_start), L, nseg, min_used, types.SimpleNamespace(bins=ForestStack._round_bins(*bins)))
        codes = torch.empty((B, S, max(nseg, 0)), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().qfa_segment_codes_f32(
            _lib.require_device_tensor(trans, f32, "trans"), _lib.require_device_tensor(ivar, f32, "ivar"), C.byref(bs), _ptr(tb), B, S,
            self.Nb, C.byref(pp), _ptr(codes), _lib.current_stream(self.device)), "qfa_segment_codes_f32")
        return codes

    def segment_bootstrap(self, rows, codes, *, n_boot, seed=0, offset=0, nz, stack=None, bins=None, estimate=None):
        """The Poisson bootstrap over sightlines of per-segment rows (qfa_bootstrap_f64; the contract is in include/qfa_hip.h).
        ``rows`` (B, S, n_segments, ...) float32, float64 or int32 as a segment statistic returns them (``power``, ``pairs``,
        ``hist``, ``bandpower``, ``moments``; the axes behind the third are one row of W values), ``codes`` (B, S, n_segments) int32
        of ``segment_codes``.  Replicate r weights spectrum b by w(``seed``, ``offset`` + b, r) ~ Poisson(1) -- ``offset``: the global
        row of spectrum 0, so that a data set cut into calls gets the weights of one call.  ``stack``: a ``BootstrapStack`` of S
        draws, ``n_boot`` replicates, ``nz`` bins and W columns to ADD to (its seed is used); else a new one (``bins``, ``estimate``:
        what it should carry).  Returns the ``BootstrapStack``."""
        if not isinstance(rows, torch.Tensor) or rows.dim() < 3 or str(rows.dtype).replace("torch.", "") not in _lib.ROW_TYPES:
            raise QFAHipError("segment_bootstrap: rows must be a (B, S, n_segments, ...) float32, float64 or int32 tensor")
        B, S, nseg = (int(x) for x in rows.shape[:3])
        W = int(np.prod(rows.shape[3:], dtype=np.int64))
        if tuple(codes.shape) != (B, S, nseg):
            raise QFAHipError(f"segment_bootstrap: codes {tuple(codes.shape)}, expected ({B}, {S}, {nseg})")
        R, nz, dev = int(n_boot), int(nz), self.device
        h = _lib.lib()
        need = h.qfa_bootstrap_workspace_bytes(B, S, nseg, W, nz, R)
        if need == 0:
            raise QFAHipError(f"segment_bootstrap: unsupported shape B={B} S={S} n_segments={nseg} W={W} nz={nz} n_boot={R}")
        if stack is None:
            stack = BootstrapStack.zeros(S, R, nz, W, seed, bins, estimate, dev)
        elif not isinstance(stack, BootstrapStack) or (stack.S, stack.R, stack.nz, stack.W) != (S, R, nz, W):
            raise QFAHipError(f"segment_bootstrap(stack=...): expected a BootstrapStack of {S} draws, {R} replicates, {nz} z-bins and "
                              f"{W} columns")
        ws = self._scratch("boot_ws", need)
        _lib.check(h.qfa_bootstrap_f64(
            _lib.require_device_tensor(rows, rows.dtype, "rows"), _lib.ROW_TYPES[str(rows.dtype).replace("torch.", "")],
            _lib.require_device_tensor(codes, torch.int32, "codes"), B, S, nseg, W, nz, R, stack.seed, int(offset), 0,
            _lib.require_device_tensor(stack.buf, torch.float64, "stack"), _ptr(ws), ws.numel(), _lib.current_stream(dev)),
            "qfa_bootstrap_f64")
        return stack

    def bootstrap(self, dataloader, statistic, z_min, z_max, n_zbins, n_boot, *, boot_seed=0, **keywords):
        """A segment statistic of a whole dataloader with its sightline bootstrap: ``statistic`` is "p1d", "bands", "xi", "pdf" or
        "variance", ``keywords`` those of its loader call (``flux_power``, ``band_power``, ``flux_correlation``, ``flux_pdf``,
        ``variance_function``).  That call's loop runs with the per-segment rows kept, and every slice adds its ``n_boot`` Poisson
        replicates (``boot_seed``) to a ``BootstrapStack`` whose ``estimate`` is the statistic's own formula.  The weight of a
        spectrum depends on its dataloader index alone and every sum is one chain in segment order, so the result does not depend
        on ``batch_size``; under data parallelism the sums are all-reduced over the model's group.  Returns (stack, boot): the
        statistic's stack, bit-equal to the plain loader call's, and the ``BootstrapStack``."""
        if statistic not in _BOOT_STATS:
            raise QFAHipError(f"bootstrap: statistic = {statistic!r}, expected one of {sorted(_BOOT_STATS)}")
        if int(n_boot) < 1:
            raise QFAHipError(f"bootstrap: n_boot = {n_boot}")
        method, rows, spec = _BOOT_STATS[statistic]
        self._boot_request = req = {"n_boot": int(n_boot), "seed": int(boot_seed), "rows": rows, "spec": spec, "boot": None}
        try:
            stack = getattr(self, method)(dataloader, z_min, z_max, n_zbins, **keywords)
        finally:
            self._boot_request = None
        return stack, req["boot"]

    def flux_power(self, dataloader, z_min, z_max, n_zbins, *, n_segments=3, seg_len=None, min_used_frac=0.75, tbar=None,
                   tbar_nbins=64, n_samples=0, seed=0, batch_size=4096, cont_min=0.0, dv=None):
        """The 1D flux power spectrum of a whole dataloader: a ``P1DStack`` of S = max(1, n_samples) draws over ``n_zbins`` bins of
        [z_min, z_max) in the redshift of a segment's central pixel.  The blue side is cut into ``n_segments`` segments of
        ``seg_len`` pixels (default Nb // n_segments); a segment is used when ``min_used_frac`` of its pixels are.  ``tbar``: the
        ``ForestStack`` the contrast is formed with; None runs ``mean_transmission`` first, with the same ``n_samples`` / ``seed``
        and ``tbar_nbins`` bins that cover every pixel of a stacked segment, so that draw s of <T> is the same continuum draw as
        draw s of T.  Per slice of the loader: ``predict``, ``forest`` and ``p1d``, the draws in chunks that keep the
        (B, S_chunk, Nb) trans / ivar pair under ``P1D_PAIR_BYTES`` (1 GiB).  ``dv``: the pixel width in km/s, default
        c ln(lambda_1 / lambda_0) of the loader's ``wav_grid``.  The global row of a spectrum is its dataloader index and the
        reducer adds segments in order, so the result does not depend on ``batch_size`` beyond the rounding of float64 sums.
        Under data parallelism the sums are all-reduced over the model's group: every rank returns the global stack."""
        return self._power_of_loader("flux_power", dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar,
                                     tbar_nbins, n_samples, seed, batch_size, cont_min, dv,
                                     _LoaderStat(lambda *a: P1DStack.zeros(*a, self.device), self.p1d, {}))

    def band_power(self, dataloader, z_min, z_max, n_zbins, k_edges, *, n_segments=3, seg_len=None, min_used_frac=0.75, tbar=None,
                   tbar_nbins=64, n_samples=0, seed=0, batch_size=4096, cont_min=0.0, dv=None, resolution_kms=None,
                   subtract_noise=True):
        """The band powers of a whole dataloader and their covariance: a ``P1DBandStack`` of S = max(1, n_samples) draws over
        ``n_zbins`` bins of [z_min, z_max) and the bands ``k_edges`` (nband + 1 edges in s/km).  Everything else is
        ``flux_power``'s: the same segments, mean transmission, draws and loop over the loader, with ``p1d_bands`` in the place of
        ``p1d``.  The sums of a slice are formed in chunks of a fixed number of segments, so the result depends on ``batch_size``
        only through the rounding of float64 sums.  Under data parallelism the sums are all-reduced over the model's group."""
        return self._power_of_loader("band_power", dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar,
                                     tbar_nbins, n_samples, seed, batch_size, cont_min, dv,
                                     _LoaderStat(lambda *a: P1DBandStack.zeros(*a, k_edges, self.device), self.p1d_bands,
                                                 {"k_edges": k_edges, "resolution_kms": resolution_kms, "subtract_noise": subtract_noise}))

    def flux_correlation(self, dataloader, z_min, z_max, n_zbins, n_lags, *, n_segments=3, seg_len=None, min_used_frac=0.75, tbar=None,
                         tbar_nbins=64, n_samples=0, seed=0, batch_size=4096, cont_min=0.0, dv=None, sigma2_lss=0.0,
                         unit_weights=False):
        """The line-of-sight correlation function of a whole dataloader: a ``XiStack`` of S = max(1, n_samples) draws over
        ``n_zbins`` bins of [z_min, z_max) and the lags 0 .. ``n_lags`` - 1 (in pixels; ``XiStack.lags_kms``).  Everything else is
        ``flux_power``'s: the same segments, mean transmission, draws and loop over the loader, with ``xi`` in the place of ``p1d``
        (``sigma2_lss``, ``unit_weights``: its weights).  The sums of a slice are formed in chunks of a fixed number of segments, so
        the result depends on ``batch_size`` only through the rounding of float64 sums.  Under data parallelism the sums are
        all-reduced over the model's group."""
        return self._power_of_loader("flux_correlation", dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar,
                                     tbar_nbins, n_samples, seed, batch_size, cont_min, dv,
                                     _LoaderStat(lambda S, z0, dz, nz, L, dv: XiStack.zeros(S, z0, dz, nz, L, n_lags, dv, self.device), self.xi,
                                                 {"n_lags": int(n_lags), "sigma2_lss": float(sigma2_lss), "unit_weights": bool(unit_weights)}))

    def flux_pdf(self, dataloader, z_min, z_max, n_zbins, n_tbins=20, *, t_min=0.0, t_max=1.0, relative=False, clamp=True,
                 ivar_min=0.0, n_segments=3, seg_len=None, min_used_frac=0.75, tbar=None, tbar_nbins=64, n_samples=0, seed=0,
                 batch_size=4096, cont_min=0.0):
        """The flux PDF of a whole dataloader and its covariance: a ``PDFStack`` of S = max(1, n_samples) draws over ``n_zbins`` bins
        of [z_min, z_max) and ``n_tbins`` flux bins of [t_min, t_max) (``relative``, ``clamp``, ``ivar_min``: see
        ``flux_pdf_segments``).  Everything else is ``flux_power``'s: the same segments, mean transmission, draws and loop over the
        loader, with ``flux_pdf_segments`` in the place of ``p1d``.  The PDF rides on segments, not on the per-pixel z-bins of
        ``mean_transmission``, because the segment is the unit its covariance is estimated from.  The sums are integers: the
        result does not depend on ``batch_size`` at all.  Under data parallelism the sums are all-reduced over the model's group."""
        pdf = {"t_min": float(t_min), "t_max": float(t_max), "n_tbins": int(n_tbins), "relative": bool(relative), "clamp": bool(clamp),
               "ivar_min": float(ivar_min)}
        want = self._flux_params(**pdf)
        zeros = lambda S, z0, dz, nz, L, dv: PDFStack.zeros(S, z0, dz, nz, L, *want, self.device)
        # (dv None: the PDF needs it for the range of its own <T> alone)
        return self._power_of_loader("flux_pdf", dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar,
                                     tbar_nbins, n_samples, seed, batch_size, cont_min, None,
                                     _LoaderStat(zeros, self.flux_pdf_segments, pdf, needs_dv=False))

    def variance_function(self, dataloader, z_min, z_max, n_zbins, *, e_lo=-12, n_oct=14, sub=1, d_max=None, n_segments=3, seg_len=None,
                          min_used_frac=0.75, tbar=None, tbar_nbins=64, n_samples=0, seed=0, batch_size=4096, cont_min=0.0):
        """The variance function of a whole dataloader: a ``VarianceStack`` of S = max(1, n_samples) draws over ``n_zbins`` bins of
        [z_min, z_max) and ``n_oct`` << ``sub`` bins of the pipeline's noise variance from 2^``e_lo`` on (``d_max``: see
        ``variance_segments``).  Everything else is ``flux_power``'s: the same segments, mean transmission, draws and loop over the
        loader, with ``variance_segments`` in the place of ``p1d``.  ``VarianceStack.fit()`` then gives eta(z), the correction to
        the pipeline's noise, and sigma2_lss(z), the intrinsic variance of the forest: ``fit().sigma2_lss`` is the number
        ``flux_correlation(sigma2_lss=...)`` and ``xi`` take -- as ONE scalar per call (of the z-bin of interest, or a mean over
        the bins); ``std_over_draws`` is the continuum's error bar on both.  The sums of a slice are formed in chunks of a fixed
        number of segments, so the result depends on ``batch_size`` only through the rounding of float64 sums.  Under data
        parallelism the sums are all-reduced over the model's group."""
        var = {"e_lo": int(e_lo), "n_oct": int(n_oct), "sub": int(sub), "d_max": d_max}
        VarianceStack.var_params(**var)
        zeros = lambda S, z0, dz, nz, L, dv: VarianceStack.zeros(S, z0, dz, nz, L, device=self.device, **var)
        # (dv None: the variance function needs it for the range of its own <T> alone)
        return self._power_of_loader("variance_function", dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar,
                                     tbar_nbins, n_samples, seed, batch_size, cont_min, None,
                                     _LoaderStat(zeros, self.variance_segments, var, needs_dv=False))

    def _power_of_loader(self, what, dataloader, z_min, z_max, n_zbins, n_segments, seg_len, min_used_frac, tbar, tbar_nbins,
                         n_samples, seed, batch_size, cont_min, dv, stat):
        """the loop `flux_power`, `band_power`, `flux_correlation`, `flux_pdf` and `variance_function` share; ``stat``: the statistic's `_LoaderStat`"""
        nseg, nz, S = int(n_segments), int(n_zbins), max(1, int(n_samples))
        L = int(seg_len) if seg_len is not None else (self.Nb // nseg if nseg > 0 else 0)
        if nseg < 1 or L < 1 or nseg * L > self.Nb or nz < 1 or not float(z_max) > float(z_min) or not 0.0 < float(min_used_frac) <= 1.0:
            raise QFAHipError(f"{what}: {nseg} segments of {L} pixels on Nb = {self.Nb}, bins [{z_min}, {z_max}) / {nz}, "
                              f"min_used_frac = {min_used_frac}")
        if dv is None and (stat.needs_dv or tbar is None):
            wav = getattr(dataloader, "wav_grid", None)
            if wav is None or len(wav) < 2:
                raise QFAHipError(what + ": the dataloader has no wav_grid: pass dv (km/s per pixel)")
            dv = 299792.458 * float(np.log(float(wav[1]) / float(wav[0])))
        stack = stat.zeros(S, z_min, (float(z_max) - float(z_min)) / nz, nz, L, dv)
        min_used = max(1, int(np.ceil(float(min_used_frac) * L)))
        if tbar is None:
            half = float(np.exp(0.5 * (L + 1) * float(dv) / 299792.458))          # (1 + z) over half a segment
            tbar = self.mean_transmission(dataloader, (1.0 + float(z_min)) / half - 1.0, (1.0 + float(z_max)) * half - 1.0,
                                          int(tbar_nbins), n_samples=int(n_samples), seed=seed, batch_size=batch_size,
                                          cont_min=cont_min)
        if not isinstance(tbar, ForestStack) or tbar.S not in (1, S):
            raise QFAHipError(f"{what}: tbar must be a ForestStack of 1 or {S} draws")
        tmean = tbar.mean.to(f32)
        row0 = int(getattr(dataloader, "_row0", 0))              # (a data-parallel loader: the global index of its first row)
        req, self._boot_request = getattr(self, "_boot_request", None), None      # (`bootstrap` asks: the rows are kept and resampled)
        if req is not None:
            W, estimate = req["spec"](stack)
            req["boot"] = BootstrapStack.zeros(S, req["n_boot"], nz, W, req["seed"], stack.bins, estimate, self.device)
        for s, inputs, _ in self._loader_slices(dataloader, int(batch_size)):
            _, hmean, hcov, _, unc = self.predict(**inputs)
            B = int(hmean.shape[0])
            if int(n_samples) > 0:
                h, unc = self.sample_latent(hmean, hcov, S, seed=seed, offset=row0 + s), None
            else:
                h = hmean.reshape(B, 1, self.Nh)
            Sc = max(1, min(S, self.P1D_PAIR_BYTES // max(1, B * self.Nb * 8)))
            zin = {"batch": inputs["batch"]} if "batch" in inputs else {"zabs": inputs["zabs"]}
            for s0 in range(0, S, Sc):
                s1 = min(S, s0 + Sc)
                hs = h if (s0 == 0 and s1 == S) else h[:, s0:s1].contiguous()
                tr, iv, _ = self.forest(**inputs, h=hs, unc=unc, cont_min=cont_min)
                kw = dict(tbar=tmean if tbar.S == 1 else tmean[s0:s1], tbar_bins=tbar.bins, seg_len=L, n_segments=nseg,
                          min_used=min_used, stack=stack.draws(s0, s1), return_segments=req is not None)
                out = stat.call(tr, iv, **zin, **kw, **stat.keywords)
                if req is not None:
                    seg = {k: kw[k] for k in ("tbar", "tbar_bins", "seg_len", "n_segments", "min_used")}
                    codes = self.segment_codes(tr, iv, **zin, **seg, bins=stack.bins)
                    self.segment_bootstrap(req["rows"](out), codes, n_boot=req["n_boot"], offset=row0 + s, nz=nz,
                                           stack=req["boot"].draws(s0, s1))
        if self._dp:
            stack.all_reduce(self._dp_group)
            if req is not None:
                req["boot"].all_reduce(self._dp_group)
        return stack
