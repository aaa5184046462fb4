"""QFA model with the reference's Python surface (reference QFA/model.py:24-316) on HIP kernels.

Same constructor, attributes, method names, argument order and return shapes as the reference
class ``QFA``; ``QFAModel`` / ``fit`` / ``predict`` are the aliases BASELINE.json's north_star
names.  Every method that computes something calls the C-ABI in ``include/qfa_hip.h``; nothing
here falls back to torch arithmetic when the library or the GPU is missing.

Additions over the reference (none changes a reference call's result):
  * ``predict`` -- batched ``prediction_for_single_spectra``;
  * ``sample_latent`` / ``continua_from_latent`` / ``sample_continua`` -- posterior draws on the device (include/qfa_hip.h);
  * ``sample_spectra`` / ``posterior_predictive`` -- mock spectra and posterior-predictive replicates drawn from the model;
  * the forest statistics, methods of the base class ``ForestStatistics`` (statistics.py) with their result classes in stacks.py:
    ``forest`` / ``mean_transmission`` / ``ForestStack`` -- Lyman-alpha forest transmission flux / continuum and its
    redshift-binned stack, per posterior draw, without writing a continuum (include/qfa_hip.h, qfa_forest_f32);
    ``p1d`` / ``flux_power`` / ``P1DStack`` -- the 1D flux power spectrum of forest segments and its (k, z) stack, per posterior
    draw (include/qfa_hip.h, qfa_p1d_f32);
    ``p1d_bands`` / ``band_power`` / ``P1DBandStack`` -- its band powers and the covariance matrix between the bands per draw and
    z-bin (include/qfa_hip.h, qfa_p1d_band_f32);
    ``xi`` / ``flux_correlation`` / ``XiStack`` -- the pair-weighted correlation function of the same segments along the line of
    sight and its (lag, z) stack, which carries no window of the mask (include/qfa_hip.h, qfa_xi_f32);
    ``flux_pdf_segments`` / ``flux_pdf`` / ``PDFStack`` -- the probability distribution of the transmitted flux of the same segments
    and the covariance matrix between its flux bins per draw and z-bin (include/qfa_hip.h, qfa_flux_pdf_f32);
    ``variance_segments`` / ``variance_function`` / ``VarianceStack`` -- the variance of delta_F of the same segments in bins of the
    pipeline's noise variance and of z, and the fit of eta and sigma2_lss on it (include/qfa_hip.h, qfa_variance_f32);
  * ``observed_residuals`` / ``observed_stack`` / ``ObservedStack`` -- the observed-frame residual stack, methods of the base class
    ``ObservedFrame`` (calibration.py): the calibration vector and the sky-line mask from the data themselves (include/qfa_hip.h,
    qfa_obs_stack_f32, qfa_calibrate_f32);
  * ``bal_scan`` / ``bal_catalog`` / ``BALScan`` -- the BAL finder, methods of the base class ``BALFinder`` (bal.py): BI, AI and the
    trough velocities per spectrum and posterior draw (include/qfa_hip.h, ``qfa_bal_scan_f32``, ``qfa_bal_mask_f32``);
  * ``dla_profiles`` / ``template_scan`` / ``dla_scan`` / ``DLAScan`` -- the DLA finder, methods of the base class ``DLAFinder``
    (dla.py): a likelihood-ratio scan of every spectrum over a grid of absorber redshift and column density (include/qfa_hip.h,
    qfa_template_scan_f32), whose catalogue ``mask_absorbers`` takes;
  * ``redshift_scan`` / ``redshift_catalog`` / ``RedshiftScan`` -- the quasar-redshift finder, methods of the base class
    ``RedshiftFinder`` (redshift.py): the likelihood of every spectrum at integer pixel shifts between data and model
    (include/qfa_hip.h, qfa_redshift_scan_f32), whose ``z()`` a second ``preprocess`` takes;
  * ``step`` -- forward + Adam + clip without a host sync (what ``train`` and bench.py run);
  * data parallelism: ``enable_data_parallel()`` all-reduces the packed sum/count buffer over
    RCCL once per step before the normalisation;
  * ``load_from_npz(path, reference_c0_quirk=True)``: the reference loader sets c0 <- beta
    (model.py:295); that stays the default because the shipped known answers need it.
"""
from __future__ import annotations

import ctypes as C
import os
import time
import weakref
from functools import partial
from typing import Callable, Dict

import numpy as np
import torch

from . import _lib
from . import utils as _utils
from .stacks import BootstrapStack, EMStats, ForestStack, P1DBandStack, P1DStack, PDFStack, VarianceStack, XiStack    # (re-exported)
from .dla import DLAFinder, DLAScan    # (re-exported)
from .calibration import ObservedFrame, ObservedStack    # (re-exported)
from .bal import BALFinder, BALScan    # (re-exported)
from .redshift import RedshiftFinder, RedshiftScan    # (re-exported)
from .statistics import ForestStatistics

f32 = torch.float32
log2pi = 1.8378770664093453
default_tau = partial(_utils.tau, which="becker")

PARAM_KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")
# default of QFA.auto_factor_zabs (tests/conftest.py turns it off: zabs tensors there are meant to exercise the zabs kernels;
# tests/test_auto_factor_default.py runs the default) and the relative tolerance of the structure test: three float32 roundings of
# 1 + z (zabs itself, zq1, pix_ratio).  The factors never serve a call made during a graph capture, a call in deterministic mode
# or an inference tensor (QFA._auto_zfac).
AUTO_FACTOR_ZABS = True
AUTO_FACTOR_TOL = 4e-7
AUTO_FACTOR_RECHECK = 64


def _resolve_tau(tau):
    """Map the reference's ``tau`` argument (a callable, model.py:26) onto a kernel tau model.
    Returns (TauModel or None, callable or None): built-ins run in-kernel, anything else is
    evaluated by calling it on zabs and handing exp(-tau) to the kernels as A_blue."""
    if isinstance(tau, str):
        return _lib.tau_model(tau, 1), None
    if isinstance(tau, partial) and tau.func is _utils.tau and not tau.args:
        kw = dict(tau.keywords or {})
        return _lib.tau_model(kw.get("which", "becker"), kw.get("series", 1)), None
    if tau is _utils.tau:
        return _lib.tau_model("becker", 1), None
    if callable(tau):
        return _lib.tau_model("becker", 1), tau
    raise TypeError("tau must be a name, qfa_amd.utils.tau (partial) or a callable")


class QFA(ForestStatistics, DLAFinder, ObservedFrame, BALFinder, RedshiftFinder):

    def __init__(self, Nb: int, Nr: int, Nh: int, device: torch.device,
                 tau: Callable[[torch.Tensor], torch.Tensor] = default_tau,
                 model_params: Dict[str, np.ndarray] = None) -> None:
        self.Nb = int(Nb)
        self.Nr = int(Nr)
        self.Nh = int(Nh)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.QFAHipError(f"QFA(device={device}): qfa_amd needs a HIP device (torch device 'cuda'); "
                                   "there is no CPU path")
        _lib.lib()
        self.Npix = self.Nb + self.Nr
        self.Nparams = self.Npix * self.Nh + self.Npix + self.Nb + 3
        self.tau = tau
        self._tau_model, self._tau_callable = _resolve_tau(tau)
        self.min_value = 1e-3
        self.max_value = 2.
        if model_params is not None:
            for k in PARAM_KEYS:
                setattr(self, k, torch.tensor(np.asarray(model_params[k]), dtype=f32).to(self.device).contiguous())
        else:
            self.random_init_func()
        self.mu = None
        self._ws = {}
        self._p1d_band_cache = {}                       # (_p1d_band_tables)
        self._dp_group = None
        self._dp = False
        self._dp_checked = False
        self._ar_events = None                          # optional (start, end) torch.cuda.Event pair recorded around the all-reduce
        # deterministic=True: per-block slab + fixed-order reducer instead of float32 atomics in pass 2
        # (qfa_nll_grad_det_f32): bit-identical sums from run to run, at the price of a (B/64) x accum-sized slab
        # (8..64 rows where pass 2 is pixel-resident -- large batches; there the default has no atomics either)
        self.deterministic = False
        # exact_gradients=True: the gradient of the loss the step reports, mean NLL over the batch (QFA_F_EXACT_GRAD), instead of
        # the reference's formulas (QFA/model.py:137-144: an extra diag(A) in the F term, 1 - tau0 (1+z)^beta - c0 and an extra zd
        # in the tau0 / c0 / beta terms, every element divided by its own count, 0/0 = NaN).  The packed buffer records the mode
        # (scalar slot 6), so forward / step / update_from_accum / train follow it with no other switch.  Not saved in checkpoints.
        self.exact_gradients = False
        # kernel-form switches of the *_ex_f32 entry points (_lib.F_*; 0 = defaults): A/B timing, cross-checks in tests/
        self.flags = 0
        # use the factored-z input form when a batch carries it (DeviceDataloader batches, or zfac=...): same results to
        # float32 rounding, 4 Nb bytes per spectrum and pass less HBM traffic, three transcendentals per blue element less
        self.use_factored_z = True
        # A plain zabs tensor (the reference's forward signature, no zfac attached) that comes back a SECOND time -- the same live
        # tensor object, unchanged (torch's version counter) -- is tested once for the structure the reference's loader gives it,
        # 1 + zabs[s][i] = (1 + z_qso[s]) wav_i / 1215.67 (QFA/dataloader.py:102; qfa_zabs_factor_f32, one pass over it and one
        # host synchronisation), and from then on the factored-z kernels run for it.  A loader that hands out fresh tensors every
        # step never pays anything; zabs that does not factor within AUTO_FACTOR_TOL keeps the zabs kernels.  Three kinds of call
        # always read zabs: a call inside a graph capture (the replays read whatever the static tensor then holds, while cached
        # factors would be the capture-time batch's), a call with deterministic = True (the first call on a tensor and the later
        # ones must run the same arithmetic) and a zabs made under torch.inference_mode() (no version counter to notice writes).
        # An explicit zfac, or the one a DeviceDataloader batch carries, is used in all three.
        self.auto_factor_zabs = AUTO_FACTOR_ZABS
        self._zf_seen = {}
        # running statistics of train(f_update="em") (an EMStats, or None); saved by save_checkpoint when present
        self.em_running = None

    # ------------------------------------------------------------------ parameters
    def random_init_func(self) -> None:
        """reference QFA/model.py:57-72"""
        self.F = (torch.rand((self.Npix, self.Nh), dtype=f32) - 0.5).to(self.device)
        self.Psi = torch.ones((self.Npix,), dtype=f32, device=self.device)
        self.omega = torch.ones((self.Nb,), dtype=f32, device=self.device)
        self.tau0 = torch.tensor(0.02, dtype=f32, device=self.device)
        self.c0 = torch.tensor(0.3, dtype=f32, device=self.device)
        self.beta = torch.tensor(2., dtype=f32, device=self.device)
        if getattr(self, "_dp", False):                 # every process drew its own F: rank 0's wins
            self.sync_replicas()

    @property
    def parameters(self):
        return {k: getattr(self, k) for k in PARAM_KEYS}

    @parameters.setter
    def parameters(self, params_dict):
        for k in PARAM_KEYS:
            setattr(self, k, params_dict[k])
        self.clip()

    def _clip_table(self):
        return {"omega": (self.min_value, self.max_value), "Psi": (self.min_value, self.max_value),
                "tau0": (0., 1.), "beta": (0.1, 5.), "c0": (-5., 5.)}

    def clip(self):
        """reference QFA/model.py:233-241"""
        h = _lib.lib()
        st = _lib.current_stream(self.device)
        for k, (lo, hi) in self._clip_table().items():
            x = getattr(self, k).to(f32).contiguous()
            if x.numel() == 0:                          # omega of a model without blue pixels
                continue
            y = torch.empty_like(x)
            _lib.check(h.qfa_clip_f32(_lib.require_device_tensor(x, f32, k), C.c_void_p(y.data_ptr()), x.numel(),
                                      lo, hi, st), "qfa_clip_f32")
            setattr(self, k, y)

    def smooth(self):
        """reference QFA/model.py:243-252: 15-px windows on omega/Psi, 31-px on F along pixels."""
        h = _lib.lib()
        st = _lib.current_stream(self.device)
        for k, half in (("omega", 7), ("Psi", 7), ("F", 15)):
            x = getattr(self, k).to(f32).contiguous()
            if x.numel() == 0:
                continue
            y = torch.empty_like(x)
            n = x.shape[0]
            cols = x.numel() // max(n, 1)
            _lib.check(h.qfa_smooth_f32(_lib.require_device_tensor(x, f32, k), C.c_void_p(y.data_ptr()), n, cols,
                                        half, st), "qfa_smooth_f32")
            setattr(self, k, y)

    # ------------------------------------------------------------------ plumbing
    def _params_struct(self):
        ps = _lib.Params()
        self._keep = []
        for k in PARAM_KEYS:
            t = getattr(self, k)
            if t.dtype != f32 or not t.is_contiguous() or t.device != self.device:
                t = t.to(device=self.device, dtype=f32).contiguous()
                setattr(self, k, t)
            setattr(ps, k, _lib.require_device_tensor(t, f32, k).value)
        return ps

    def _redshift_form(self, bs, keep, B, zabs, zfac=None, auto_factor=False, also_zabs=False):
        """The one rule for the redshift of the blue pixels of a qfa_batch_t: fills ``bs.zabs`` / ``bs.zq1`` / ``bs.pix_ratio`` for ``B``
        spectra, appends the float32 contiguous tensors they point into to ``keep`` and returns the converted zabs (or None).
        ``zfac`` = (zq1 (B,), pix_ratio (Nb,)): the factored-z input form of include/qfa_hip.h (1 + zabs[s][i] = zq1[s] pix_ratio[i],
        reference QFA/dataloader.py:102); default: the ``zfac`` attribute a DeviceDataloader attaches to the zabs tensors it builds.
        The pair is used when the model reads factored z at all (``use_factored_z``, no custom tau callable); else, or without one, the
        kernels read zabs.  ``auto_factor``: a plain zabs may be swapped for factors derived from it (`_auto_zfac`) -- off for the
        forest statistics, whose bins are defined bit for bit by z.  ``also_zabs``: zabs is passed on next to the pair (the training
        and prediction calls; the statistics pass one form only)."""
        if zfac is None:
            zfac = getattr(zabs, "zfac", None)
        usable = self.Nb > 0 and self._tau_callable is None and self.use_factored_z
        if zfac is None and zabs is not None and auto_factor and self.auto_factor_zabs and usable:
            zfac = self._auto_zfac(zabs)
        if not usable:
            zfac = None
        bs.zabs = bs.zq1 = bs.pix_ratio = None
        if zabs is not None and (zfac is None or also_zabs):
            if zfac is None and tuple(zabs.shape) != (B, self.Nb):
                raise _lib.QFAHipError(f"zabs: shape {tuple(zabs.shape)}, expected ({B}, {self.Nb})")
            zabs = zabs if (zabs.dtype == f32 and zabs.is_contiguous()) else zabs.to(f32).contiguous()
            keep.append(zabs)
            if self.Nb > 0:
                bs.zabs = _lib.require_device_tensor(zabs, f32, "zabs").value
        if zfac is not None:
            zq1, ratio = zfac
            if tuple(zq1.shape) != (B,) or tuple(ratio.shape) != (self.Nb,):
                raise _lib.QFAHipError(f"zfac shapes {tuple(zq1.shape)}, {tuple(ratio.shape)}: expected ({B},), ({self.Nb},)")
            zq1 = zq1 if (zq1.dtype == f32 and zq1.is_contiguous()) else zq1.to(f32).contiguous()
            ratio = ratio if (ratio.dtype == f32 and ratio.is_contiguous()) else ratio.to(f32).contiguous()
            keep += [zq1, ratio]
            bs.zq1 = _lib.require_device_tensor(zq1, f32, "zq1").value
            bs.pix_ratio = _lib.require_device_tensor(ratio, f32, "pix_ratio").value
        elif zabs is None and self.Nb > 0:
            raise _lib.QFAHipError("zabs is None and no usable zfac = (zq1, pix_ratio) was given")
        return zabs

    def _batch_struct(self, delta, error, zabs, mask, zfac=None, allow_no_mask=False, auto_factor=True):
        """qfa_batch_t of the 4-tensor form and the tensors it points into; the redshift by `_redshift_form`"""
        if mask is None and not allow_no_mask:
            raise _lib.QFAHipError("mask is None: expected a torch.bool tensor (reference model.py:124)")
        if mask is not None and mask.dtype != torch.bool:            # (None: sample_spectra only -- every pixel is used)
            raise _lib.QFAHipError(f"mask: dtype {mask.dtype}, expected torch.bool (reference model.py:124)")
        bs = _lib.Batch()
        delta = delta if (delta.dtype == f32 and delta.is_contiguous()) else delta.to(f32).contiguous()
        error = error if (error.dtype == f32 and error.is_contiguous()) else error.to(f32).contiguous()
        if mask is not None:
            mask = mask if mask.is_contiguous() else mask.contiguous()
        keep = [delta, error, mask]
        bs.delta = _lib.require_device_tensor(delta, f32, "delta").value
        bs.error = _lib.require_device_tensor(error, f32, "error").value
        bs.mask = _lib.require_device_tensor(mask, torch.bool, "mask").value if mask is not None else None
        bs.A_blue = None
        zabs = self._redshift_form(bs, keep, delta.shape[0], zabs, zfac, auto_factor=auto_factor, also_zabs=True)
        if self._tau_callable is not None and self.Nb > 0:
            a = torch.exp(-1. * self._tau_callable(zabs)).to(f32).contiguous()   # user code (model.py:125)
            keep.append(a)
            bs.A_blue = _lib.require_device_tensor(a, f32, "A_blue").value
        return bs, keep

    def _auto_zfac(self, zabs):
        """(zq1, pix_ratio) derived from a zabs tensor that was seen before and factors (see __init__), else None"""
        if zabs.dtype != f32 or not zabs.is_contiguous() or zabs.dim() != 2 or zabs.shape[1] != self.Nb or zabs.shape[0] < 1 \
                or zabs.device != self.device:
            return None
        # (the entry is left as it is: the eager calls around a capture keep their cached pair)
        if self.deterministic or zabs.is_inference() or torch.cuda.is_current_stream_capturing():
            return None
        sig = (zabs.data_ptr(), tuple(zabs.shape), zabs._version)
        ent = self._zf_seen.get(id(zabs))
        if ent is None or ent[0]() is not zabs or ent[1] != sig:
            if len(self._zf_seen) >= 64:                                  # (dead or stale entries)
                self._zf_seen = {k: e for k, e in self._zf_seen.items() if e[0]() is not None and e[0]()._version == e[1][2]}
                if len(self._zf_seen) >= 64:
                    self._zf_seen.clear()
            self._zf_seen[id(zabs)] = (weakref.ref(zabs), sig, "seen", 0)
            return None
        # A tensor written behind torch's back (raw pointers: another library, a captured graph's input buffer filled by a kernel)
        # keeps its version counter: the factors are re-derived and re-tested every AUTO_FACTOR_RECHECK uses, which bounds how long a
        # stale pair could serve (qfa_amd's own writers bump the counter: DeviceDataloader.next_batch(out=...)).
        uses = ent[3] + 1 if len(ent) > 3 else 1
        recheck = isinstance(ent[2], tuple) and uses % AUTO_FACTOR_RECHECK == 0
        if ent[2] == "seen" or recheck:
            B = int(zabs.shape[0])
            zq1 = torch.empty(B, dtype=f32, device=self.device)
            ratio = torch.empty(self.Nb, dtype=f32, device=self.device)
            nbad = torch.empty(1, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().qfa_zabs_factor_f32(C.c_void_p(zabs.data_ptr()), B, self.Nb, AUTO_FACTOR_TOL, C.c_void_p(zq1.data_ptr()),
                                                      C.c_void_p(ratio.data_ptr()), C.c_void_p(nbad.data_ptr()),
                                                      _lib.current_stream(self.device)), "qfa_zabs_factor_f32")
            ok = int(nbad.item()) == 0                                    # (the one host synchronisation per repeated tensor)
            if ok and recheck:                                            # same tensors (a captured graph may hold their addresses)
                ent[2][0].copy_(zq1)
                ent[2][1].copy_(ratio)
                ent = (ent[0], sig, ent[2], uses)
            else:
                ent = (ent[0], sig, (zq1, ratio) if ok else None, uses)
        else:
            ent = (ent[0], ent[1], ent[2], uses)
        self._zf_seen[id(zabs)] = ent
        return ent[2]

    def _batch_struct_rows(self, rb, raw_flux=False, need_src=True):
        """qfa_batch_t of a ``ResidentBatch`` (qfa_amd/resident.py; ABI v3 rows / row_stride): pointers to the WHOLE resident
        arrays plus the device array of row numbers -- no gather, no copy.  ``raw_flux``: the predict call (delta = raw flux)."""
        if self._tau_callable is not None:
            raise _lib.QFAHipError("a custom tau callable is evaluated on materialised zabs: use the 4-tensor form")
        if rb.Npix != self.Npix or rb.Nb != self.Nb:
            raise _lib.QFAHipError(f"resident batch of shape (.., {rb.Npix}), Nb = {rb.Nb}; the model has ({self.Npix}, {self.Nb})")
        src = rb.flux if raw_flux else rb.delta
        if not need_src:                                        # (sample_spectra: the call reads neither flux nor delta)
            src = rb.error
        if src is None:
            raise _lib.QFAHipError("resident batch without " + ("flux" if raw_flux else "delta"))
        N, stride = int(rb.error.shape[0]), int(rb.stride)
        for t, name, dt in ((src, "delta", f32), (rb.error, "error", f32), (rb.mask, "mask", torch.bool)):
            if tuple(t.shape) != (N, stride) or stride < self.Npix:
                raise _lib.QFAHipError(f"resident {name}: shape {tuple(t.shape)}, expected ({N}, {stride} >= {self.Npix})")
        if rb.rows.dtype != torch.int32:
            raise _lib.QFAHipError(f"rows: dtype {rb.rows.dtype}, expected torch.int32")
        bs = _lib.Batch()
        bs.delta = _lib.require_device_tensor(src, f32, "delta").value
        bs.error = _lib.require_device_tensor(rb.error, f32, "error").value
        bs.mask = _lib.require_device_tensor(rb.mask, torch.bool, "mask").value
        bs.rows = _lib.require_device_tensor(rb.rows, torch.int32, "rows").value
        bs.row_stride = stride
        bs.A_blue = None
        bs.zabs = bs.zq1 = bs.pix_ratio = None
        if self.Nb > 0:
            if rb.zq1 is not None and self.use_factored_z:
                if tuple(rb.zq1.shape) != (N,) or tuple(rb.pix_ratio.shape) != (self.Nb,):
                    raise _lib.QFAHipError(f"resident zq1 / pix_ratio: shapes {tuple(rb.zq1.shape)}, {tuple(rb.pix_ratio.shape)}")
                bs.zq1 = _lib.require_device_tensor(rb.zq1, f32, "zq1").value
                bs.pix_ratio = _lib.require_device_tensor(rb.pix_ratio, f32, "pix_ratio").value
            elif rb.zabs is not None:
                if tuple(rb.zabs.shape) != (N, self.Nb):
                    raise _lib.QFAHipError(f"resident zabs: shape {tuple(rb.zabs.shape)}, expected ({N}, {self.Nb})")
                bs.zabs = _lib.require_device_tensor(rb.zabs, f32, "zabs").value
            else:
                raise _lib.QFAHipError("resident batch carries neither zabs nor usable (zq1, pix_ratio)")
        return bs, [rb]

    def _workspace(self, B):
        need = _lib.lib().qfa_workspace_bytes(int(B), self.Npix, self.Nh)
        if need == 0:
            raise _lib.QFAHipError(f"unsupported shape B={B} Npix={self.Npix} Nh={self.Nh}")
        ws = self._ws.get("ws")
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws["ws"] = ws
        return ws

    def _accum(self, zero=True):
        n = _lib.lib().qfa_accum_floats(self.Npix, self.Nb, self.Nh)
        acc = self._ws.get("accum")
        if acc is None or acc.numel() != n:
            acc = torch.empty(n, dtype=f32, device=self.device)
            self._ws["accum"] = acc
        if zero:
            acc.zero_()
        return acc

    def _scratch(self, key, nbytes):
        """the uint8 workspace ``self._ws[key]``, grown to hold ``nbytes``"""
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return buf

    def _check_batch_shapes(self, delta, error, zabs, mask):
        B = delta.shape[0]
        if zabs is None:
            zabs = delta.new_empty((B, self.Nb))            # (factored-z form: shape check of the rest only)
        if tuple(delta.shape) != (B, self.Npix) or tuple(error.shape) != (B, self.Npix) \
                or tuple(mask.shape) != (B, self.Npix) or tuple(zabs.shape) != (B, self.Nb):
            raise _lib.QFAHipError(
                f"batch shapes {tuple(delta.shape)}, {tuple(error.shape)}, {tuple(zabs.shape)}, {tuple(mask.shape)} "
                f"do not match (B,{self.Npix}), (B,{self.Npix}), (B,{self.Nb}), (B,{self.Npix})")
        return B

    def _resolve_latent(self, what, B, *, h, hmean, hcov, n_samples, seed, offset, unc, predict_inputs):
        """The latent of a call on posterior draws (``forest``, ``observed_residuals``, ``bal_scan``): ``h`` (B, S, Nh) as it is; else
        ``hmean`` alone (or with ``hcov`` and ``n_samples`` = 0), S = 1; else ``hmean`` + ``hcov`` + ``n_samples`` > 0 through
        ``sample_latent``; with none of them ``predict(**predict_inputs)`` runs first, and its unc is handed back when S = 1 and
        none was passed.  Returns ``(h, S, unc)``; ``what`` names the caller in the messages."""
        if hcov is not None and hmean is None:
            raise _lib.QFAHipError(f"{what}: hcov without hmean")
        if h is not None and hmean is not None:
            raise _lib.QFAHipError(f"{what}: pass h or hmean / hcov, not both")
        S = int(n_samples)
        if S < 0 or (S > 0 and h is None and hmean is not None and hcov is None):
            raise _lib.QFAHipError(f"{what}: n_samples > 0 needs hcov next to hmean")
        if h is None and hmean is None:
            _, hmean, hcov, _, punc = self.predict(**predict_inputs)
            if S == 0 and unc is None:
                unc = punc
        if h is not None:
            if h.dim() != 3 or h.shape[0] != B or h.shape[2] != self.Nh or h.shape[1] < 1 or (S > 0 and h.shape[1] != S):
                raise _lib.QFAHipError(f"h: shape {tuple(h.shape)}, expected ({B}, {S if S > 0 else 'S'}, {self.Nh})")
            return h, int(h.shape[1]), unc
        if tuple(hmean.shape) != (B, self.Nh):
            raise _lib.QFAHipError(f"hmean: shape {tuple(hmean.shape)}, expected ({B}, {self.Nh})")
        if S > 0:
            return self.sample_latent(hmean, hcov, S, seed=seed, offset=offset), S, unc
        return hmean.reshape(B, 1, self.Nh), 1, unc

    def _flux_batch(self, flux, error, mask):
        """qfa_batch_t of flux / error / mask alone and the tensors it points into: the tensor form of a call that reads no
        redshift (``observed_residuals``, ``bal_scan``).  The callers check the shapes: their messages differ."""
        if mask is not None and mask.dtype != torch.bool:
            raise _lib.QFAHipError(f"mask: dtype {mask.dtype}, expected torch.bool")
        bs = _lib.Batch()
        flux = flux if (flux.dtype == f32 and flux.is_contiguous()) else flux.to(f32).contiguous()
        error = error if (error.dtype == f32 and error.is_contiguous()) else error.to(f32).contiguous()
        mask = mask if mask is None or mask.is_contiguous() else mask.contiguous()
        bs.delta = _lib.require_device_tensor(flux, f32, "flux").value
        bs.error = _lib.require_device_tensor(error, f32, "error").value
        bs.mask = _lib.require_device_tensor(mask, torch.bool, "mask").value if mask is not None else None
        bs.rows, bs.row_stride = None, 0
        return bs, [flux, error, mask]

    # ------------------------------------------------------------------ data parallel
    def enable_data_parallel(self, group=None, optimizer=None, sync=True):
        """Shard spectra across ranks: every rank calls forward/step on its own shard; the packed
        [sums | counts | sum NLL | B] buffer is all-reduced (RCCL) before sum/count.
        Parameters (and the Adam state of ``optimizer``) are replicated: ``sync`` broadcasts rank 0's copy, because
        gF = F_local * sumA_global - accF_global silently trains garbage once the replicas differ (each process
        draws its own random F, or resumes from its own file)."""
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialised")
        self._dp = True
        self._dp_group = group
        self._dp_checked = False
        if sync:
            self.sync_replicas(optimizer)

    def _replica_tensors(self, optimizer=None):
        ts = [getattr(self, k) for k in PARAM_KEYS]
        if self.mu is not None:
            ts.append(self.mu)
        if optimizer is not None:
            ts += [optimizer.m[k] for k in PARAM_KEYS] + [optimizer.v[k] for k in PARAM_KEYS]
        return ts

    def sync_replicas(self, optimizer=None, src=0):
        """Broadcast parameters, mu and (optionally) the Adam moments and epoch index from rank ``src``."""
        from .distributed import agree_on_layout, broadcast_
        self._params_struct()                           # contiguous float32 tensors on the device
        ts = self._replica_tensors(optimizer)
        agree_on_layout(ts, self._dp_group)             # every rank issues the same broadcasts, or every rank raises
        for t in ts:
            if t.numel():
                broadcast_(t, src, self._dp_group)
        if optimizer is not None:
            i = torch.tensor([int(optimizer.i)], dtype=torch.int64, device=self.device)
            broadcast_(i, src, self._dp_group)
            optimizer.i = int(i.item())
        self._dp_checked = False

    def check_replicas(self, optimizer=None):
        """Raise unless every rank holds bit-identical parameters (and Adam state) and the same ``exact_gradients``: a
        collective, call it on all ranks."""
        from .distributed import agree_on_layout, replicas_in_sync
        agree_on_layout(self._replica_tensors(optimizer), self._dp_group)
        ts = [t for t in self._replica_tensors(optimizer) if t.numel()]
        # the gradient mode too: ranks that disagree would add both kinds of sums into one buffer (finalize: NaN)
        ts.append(torch.tensor([1.0 if self.exact_gradients else 0.0], dtype=torch.float64, device=self.device))
        if not replicas_in_sync(ts, self._dp_group):
            raise _lib.QFAHipError("data-parallel replicas differ (parameters / mu / Adam state / exact_gradients): call "
                                   "sync_replicas(optimizer) after random_init_func / load_* on every rank, and set "
                                   "exact_gradients alike")
        self._dp_checked = True

    def accumulate(self, delta=None, error=None, zabs=None, mask=None, accum=None, nll=None, events=None, zfac=None,
                   batch=None):
        """Raw sums of one (shard of a) batch into the packed buffer; no normalisation.
        ``events``: optional list of 5 recorded torch.cuda.Event(enable_timing=True) that the library
        re-records at {start, parameter images, pass 1, solve, pass 2} on the current stream (bench.py).
        ``batch``: a ``ResidentBatch`` in the place of the four tensors (the resident, indexed input form)."""
        ps = self._params_struct()
        if batch is not None:
            B = batch.B
            bs, keep = self._batch_struct_rows(batch)
        else:
            B = self._check_batch_shapes(delta, error, zabs, mask)
            bs, keep = self._batch_struct(delta, error, zabs, mask, zfac)
        ws = self._workspace(B)
        # (the model's own buffer is zeroed by the library's first kernel, QFA_F_ZERO_ACCUM: one launch less per step)
        acc = self._accum(zero=False) if accum is None else accum
        zero_flag = _lib.F_ZERO_ACCUM if accum is None else 0
        evs = None
        if events is not None:
            evs = (C.c_void_p * 5)(*[C.c_void_p(e.cuda_event) for e in events])
        slab, slab_bytes = None, 0
        if self.deterministic:
            slab_bytes = _lib.lib().qfa_det_slab_bytes(B, self.Npix, self.Nb, self.Nh)
            sl = self._ws.get("slab")
            if sl is None or sl.numel() < slab_bytes:
                sl = torch.empty(slab_bytes, dtype=torch.uint8, device=self.device)
                self._ws["slab"] = sl
            slab = C.c_void_p(sl.data_ptr())
        _lib.check(_lib.lib().qfa_nll_grad_ex_f32(
            C.byref(ps), C.byref(bs), C.byref(self._tau_model), B, self.Npix, self.Nb, self.Nh,
            C.c_void_p(nll.data_ptr()) if nll is not None else None, C.c_void_p(acc.data_ptr()),
            C.c_void_p(ws.data_ptr()), ws.numel(), slab, slab_bytes,
            int(self.flags) | zero_flag | (_lib.F_EXACT_GRAD if self.exact_gradients else 0),
            _lib.current_stream(self.device), evs), "qfa_nll_grad_ex_f32")
        return acc

    def _finalize(self, acc, normalize=True):
        g = {"F": torch.empty((self.Npix, self.Nh), dtype=f32, device=self.device),
             "Psi": torch.empty((self.Npix,), dtype=f32, device=self.device),
             "omega": torch.empty((self.Nb,), dtype=f32, device=self.device),
             "tau0": torch.empty((), dtype=f32, device=self.device),
             "c0": torch.empty((), dtype=f32, device=self.device),
             "beta": torch.empty((), dtype=f32, device=self.device)}
        loss = torch.empty((1, 1), dtype=f32, device=self.device)
        _lib.check(_lib.lib().qfa_finalize_grads_f32(
            C.c_void_p(acc.data_ptr()), C.c_void_p(self.F.data_ptr()), self.Npix, self.Nb, self.Nh,
            1 if normalize else 0, C.c_void_p(g["F"].data_ptr()), C.c_void_p(g["Psi"].data_ptr()),
            C.c_void_p(g["omega"].data_ptr()) if self.Nb > 0 else None, C.c_void_p(g["tau0"].data_ptr()),
            C.c_void_p(g["c0"].data_ptr()), C.c_void_p(g["beta"].data_ptr()), C.c_void_p(loss.data_ptr()),
            _lib.current_stream(self.device)), "qfa_finalize_grads_f32")
        return loss, g

    # ------------------------------------------------------------------ reference surface
    def forward(self, delta: torch.Tensor = None, error: torch.Tensor = None, zabs: torch.Tensor = None,
                mask: torch.Tensor = None, events=None, zfac=None, batch=None):
        """Batch loss (1,1) and count-normalised gradient dict (reference QFA/model.py:74-105).
        ``batch``: a ``ResidentBatch`` in the place of the four tensors."""
        return self._finalize(self._global_sums(delta, error, zabs, mask, events, zfac, batch), True)

    def _global_sums(self, delta, error, zabs, mask, events=None, zfac=None, batch=None):
        """the packed sum / count buffer of the (global) batch: this rank's raw sums, all-reduced under data parallelism"""
        if (batch.B if batch is not None else delta.shape[0]) == 0:
            if not self._dp:
                raise _lib.QFAHipError("forward: empty batch")
            acc = self._accum()                         # an exhausted rank adds zeros to the global sums and counts
        else:
            acc = self.accumulate(delta, error, zabs, mask, events=events, zfac=zfac, batch=batch)
        if self._dp:
            from .distributed import all_reduce_accum
            ev = self._ar_events                    # (bench.py: a pair of recorded events around the collective)
            if ev is not None:
                ev[0].record()
            all_reduce_accum(acc, self._dp_group)
            if ev is not None:
                ev[1].record()
        return acc

    def loglikelihood_and_gradient_for_single_spectra(self, delta, error, zabs, mask):
        """One spectrum: NLL (1,1) and the six un-normalised gradients, zeros at masked pixels
        (reference QFA/model.py:107-158)."""
        acc = self.accumulate(delta[None, :], error[None, :], zabs[None, :], mask[None, :])
        return self._finalize(acc, False)

    def predict(self, flux: torch.Tensor = None, error: torch.Tensor = None, zabs: torch.Tensor = None,
                mask: torch.Tensor = None, events=None, out=None, zfac=None, batch=None):
        """Batched posterior prediction: ll (B,), hmean (B,Nh), hcov (B,Nh,Nh), cont (B,Npix),
        unc (B,Npix) (reference QFA/model.py:160-180 applied to every row).  ``events``: optional list of 4 recorded
        torch.cuda.Event(enable_timing=True), re-recorded at {start, images + pass 1, solve, continuum writer};
        ``out``: the five output tensors to write into (bench.py re-uses them)."""
        if self.mu is None:
            raise _lib.QFAHipError("predict needs model.mu (load_from_npz or train first)")
        ps = self._params_struct()
        if batch is not None:                                   # a ResidentBatch: rows of the resident flux / error / mask
            B = batch.B
            bs, keep = self._batch_struct_rows(batch, raw_flux=True)
        else:
            B = self._check_batch_shapes(flux, error, zabs, mask)
            bs, keep = self._batch_struct(flux, error, zabs, mask, zfac)
        mu = self.mu.to(device=self.device, dtype=f32).contiguous()
        ws = self._workspace(B)
        dev = self.device
        if out is not None:
            ll, hmean, hcov, cont, unc = out
            for t, shp in ((ll, (B,)), (hmean, (B, self.Nh)), (hcov, (B, self.Nh, self.Nh)), (cont, (B, self.Npix)),
                           (unc, (B, self.Npix))):
                if tuple(t.shape) != shp:
                    raise _lib.QFAHipError(f"predict(out=...): expected shape {shp}, got {tuple(t.shape)}")
                _lib.require_device_tensor(t, f32, "out")
        else:
            ll = torch.empty((B,), dtype=f32, device=dev)
            hmean = torch.empty((B, self.Nh), dtype=f32, device=dev)
            hcov = torch.empty((B, self.Nh, self.Nh), dtype=f32, device=dev)
            cont = torch.empty((B, self.Npix), dtype=f32, device=dev)
            unc = torch.empty((B, self.Npix), dtype=f32, device=dev)
        evs = None
        if events is not None:
            evs = (C.c_void_p * 4)(*[C.c_void_p(e.cuda_event) for e in events])
        _lib.check(_lib.lib().qfa_predict_ex_f32(
            C.byref(ps), C.c_void_p(mu.data_ptr()), C.byref(bs), C.byref(self._tau_model), B, self.Npix, self.Nb,
            self.Nh, C.c_void_p(ll.data_ptr()), C.c_void_p(hmean.data_ptr()), C.c_void_p(hcov.data_ptr()),
            C.c_void_p(cont.data_ptr()), C.c_void_p(unc.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
            int(self.flags), _lib.current_stream(dev), evs), "qfa_predict_ex_f32")
        return ll, hmean, hcov, cont, unc

    # ------------------------------------------------------------------ posterior draws
    def sample_latent(self, hmean, hcov, n_samples, seed=0, offset=0, out=None):
        """``n_samples`` draws h ~ N(hmean[b], hcov[b]) of every spectrum: (B, S, Nh) float32 (qfa_sample_latent_f32; the
        draw contract is in include/qfa_hip.h).  ``offset`` is the global row of spectrum 0, so that the draws of a spectrum
        depend only on (seed, its global row), not on how a data set is cut into calls.  ``out``: a (B, S, Nh) tensor to fill."""
        S = int(n_samples)
        if S < 1:
            raise _lib.QFAHipError(f"sample_latent: n_samples = {n_samples}, expected >= 1")
        if int(offset) < 0:
            raise _lib.QFAHipError(f"sample_latent: offset = {offset}, expected >= 0")
        if not 0 <= int(seed) < 2 ** 64:
            raise _lib.QFAHipError(f"sample_latent: seed = {seed}, expected a uint64")
        if hmean.dim() != 2 or hmean.shape[1] != self.Nh:
            raise _lib.QFAHipError(f"hmean: shape {tuple(hmean.shape)}, expected (B, {self.Nh})")
        B = hmean.shape[0]
        if tuple(hcov.shape) != (B, self.Nh, self.Nh):
            raise _lib.QFAHipError(f"hcov: shape {tuple(hcov.shape)}, expected ({B}, {self.Nh}, {self.Nh})")
        pm = _lib.require_device_tensor(hmean, f32, "hmean")
        pc = _lib.require_device_tensor(hcov, f32, "hcov")
        if out is None:
            out = torch.empty((B, S, self.Nh), dtype=f32, device=hmean.device)
        elif tuple(out.shape) != (B, S, self.Nh):
            raise _lib.QFAHipError(f"sample_latent(out=...): expected shape {(B, S, self.Nh)}, got {tuple(out.shape)}")
        po = _lib.require_device_tensor(out, f32, "out")
        _lib.check(_lib.lib().qfa_sample_latent_f32(pm, pc, B, self.Nh, S, C.c_uint64(int(seed)), int(offset), po,
                                                    _lib.current_stream(hmean.device)), "qfa_sample_latent_f32")
        return out

    def continua_from_latent(self, h, out=None):
        """mu + F h for latent vectors h (..., Nh): (..., Npix) float32 (qfa_continua_f32) -- the mock-continuum notebook's
        ``F@h+mu`` for any number of vectors at once."""
        if self.mu is None:
            raise _lib.QFAHipError("continua_from_latent needs model.mu (load_from_npz or train first)")
        if h.dim() < 1 or h.shape[-1] != self.Nh:
            raise _lib.QFAHipError(f"h: shape {tuple(h.shape)}, expected (..., {self.Nh})")
        ph = _lib.require_device_tensor(h, f32, "h")
        R = h.numel() // self.Nh
        shape = tuple(h.shape[:-1]) + (self.Npix,)
        if out is None:
            out = torch.empty(shape, dtype=f32, device=h.device)
        elif tuple(out.shape) != shape:
            raise _lib.QFAHipError(f"continua_from_latent(out=...): expected shape {shape}, got {tuple(out.shape)}")
        po = _lib.require_device_tensor(out, f32, "out")
        mu = self.mu.to(device=self.device, dtype=f32).contiguous()
        ws = self._scratch("cont_ws", _lib.lib().qfa_continua_workspace_bytes(self.Npix, self.Nh))
        _lib.check(_lib.lib().qfa_continua_f32(
            _lib.require_device_tensor(self.F, f32, "F"), C.c_void_p(mu.data_ptr()), ph, R, self.Npix, self.Nh, po,
            C.c_void_p(ws.data_ptr()), ws.numel(), _lib.current_stream(h.device)), "qfa_continua_f32")
        return out

    def sample_continua(self, flux=None, error=None, zabs=None, mask=None, n_samples=1, seed=0, offset=0, hmean=None,
                        hcov=None, batch=None, zfac=None, out=None, return_latent=False):
        """``n_samples`` continua per spectrum drawn from the posterior: (B, S, Npix) float32 (and h (B, S, Nh) with
        ``return_latent``).  With ``hmean`` / ``hcov`` it only draws and writes; otherwise ``predict`` runs on the inputs first
        (the four tensors, ``zfac`` or a resident ``batch``).  Bit-identical to sample_latent + continua_from_latent."""
        if self.mu is None:
            raise _lib.QFAHipError("sample_continua needs model.mu (load_from_npz or train first)")
        if int(n_samples) < 1:
            raise _lib.QFAHipError(f"sample_continua: n_samples = {n_samples}, expected >= 1")
        if (hmean is None) != (hcov is None):
            raise _lib.QFAHipError("sample_continua: pass hmean and hcov together")
        if hmean is None:
            _, hmean, hcov, _, _ = self.predict(flux, error, zabs, mask, zfac=zfac, batch=batch)
        h = self.sample_latent(hmean, hcov, n_samples, seed=seed, offset=offset)
        cont = self.continua_from_latent(h, out=out)
        return (cont, h) if return_latent else cont

    # ------------------------------------------------------------------ mock spectra
    def sample_spectra(self, error=None, zabs=None, mask=None, *, n_samples=1, seed=0, offset=0, h=None, hmean=None, hcov=None,
                       zfac=None, batch=None, out=None, return_delta=False, return_latent=False):
        """``n_samples`` spectra per row drawn from the model, flux = A (mu + F h) + sqrt(D) e under the row's own ``error`` and
        ``mask``: (B, S, Npix) float32, masked pixels -999 (qfa_mock_spectra_f32; the draw contract is in include/qfa_hip.h).
        The latent: ``h`` (B, S, Nh) as it is (``n_samples`` may then stay at its default); else ``hmean`` / ``hcov`` through ``sample_latent`` (a posterior-predictive
        replicate when they come from ``predict``); else the prior (zeros / identity through ``sample_latent``): mock data.
        ``offset`` is the global row of spectrum 0: a spectrum's draws depend only on (seed, its global row).  ``mask`` None:
        every pixel is used.  ``batch``: a ``ResidentBatch`` in the place of error / zabs / mask.  ``out``: the (B, S, Npix)
        tensor to fill.  ``return_delta`` adds delta = flux - mu A, ``return_latent`` adds h, in that order behind the flux.
        Bit-identical to calling ``sample_latent`` and the C entry point by hand."""
        if self.mu is None:
            raise _lib.QFAHipError("sample_spectra needs model.mu (load_from_npz or train first)")
        S = int(n_samples)
        if S < 1:
            raise _lib.QFAHipError(f"sample_spectra: n_samples = {n_samples}, expected >= 1")
        if int(offset) < 0:
            raise _lib.QFAHipError(f"sample_spectra: offset = {offset}, expected >= 0")
        if not 0 <= int(seed) < 2 ** 64:
            raise _lib.QFAHipError(f"sample_spectra: seed = {seed}, expected a uint64")
        if (hmean is None) != (hcov is None):
            raise _lib.QFAHipError("sample_spectra: pass hmean and hcov together")
        if h is not None and hmean is not None:
            raise _lib.QFAHipError("sample_spectra: pass h or hmean / hcov, not both")
        ps = self._params_struct()
        if batch is not None:
            B = batch.B
            bs, keep = self._batch_struct_rows(batch, need_src=False)
        else:
            if not isinstance(error, torch.Tensor) or error.dim() != 2:
                raise _lib.QFAHipError("sample_spectra: error must be a (B, Npix) tensor")
            B = self._check_batch_shapes(error, error, zabs, mask if mask is not None else error)
            bs, keep = self._batch_struct(error, error, zabs, mask, zfac, allow_no_mask=True)
        bs.delta = None                                         # (not read by the call)
        dev = self.device
        if h is None:
            if hmean is None:
                hmean = torch.zeros((B, self.Nh), dtype=f32, device=dev)
                hcov = torch.eye(self.Nh, dtype=f32, device=dev).repeat(B, 1, 1)
            elif hmean.dim() != 2 or hmean.shape[0] != B:
                raise _lib.QFAHipError(f"hmean: shape {tuple(hmean.shape)}, expected ({B}, {self.Nh})")
            h = self.sample_latent(hmean, hcov, S, seed=seed, offset=offset)
        else:
            if h.dim() == 3 and S == 1:                         # (n_samples left at its default: h says how many)
                S = int(h.shape[1])
            if tuple(h.shape) != (B, S, self.Nh) or S < 1:
                raise _lib.QFAHipError(f"h: shape {tuple(h.shape)}, expected {(B, S, self.Nh)}")
        ph = _lib.require_device_tensor(h, f32, "h")
        if out is None:
            out = torch.empty((B, S, self.Npix), dtype=f32, device=dev)
        elif tuple(out.shape) != (B, S, self.Npix):
            raise _lib.QFAHipError(f"sample_spectra(out=...): expected shape {(B, S, self.Npix)}, got {tuple(out.shape)}")
        po = _lib.require_device_tensor(out, f32, "out")
        delta = torch.empty((B, S, self.Npix), dtype=f32, device=dev) if return_delta else None
        mu = self.mu.to(device=dev, dtype=f32).contiguous()
        ws = self._scratch("mock_ws", _lib.lib().qfa_mock_workspace_bytes(self.Npix, self.Nh))
        _lib.check(_lib.lib().qfa_mock_spectra_f32(
            C.byref(ps), C.c_void_p(mu.data_ptr()), C.byref(bs), C.byref(self._tau_model), ph, B, S, self.Npix, self.Nb, self.Nh,
            C.c_uint64(int(seed)), int(offset), po, _lib._ptr(delta), _lib._ptr(ws), ws.numel(), _lib.current_stream(dev)),
            "qfa_mock_spectra_f32")
        res = (out,) + ((delta,) if return_delta else ()) + ((h,) if return_latent else ())
        return res if len(res) > 1 else out

    def posterior_predictive(self, flux=None, error=None, zabs=None, mask=None, n_samples=1, seed=0, offset=0, *, zfac=None,
                             batch=None):
        """``n_samples`` replicates of every observed spectrum under its own posterior, noise and mask: (B, S, Npix) float32.
        ``predict`` on the inputs, then ``sample_spectra`` with the posterior's hmean / hcov and the observed error and mask --
        what a posterior-predictive check compares with the data."""
        _, hmean, hcov, _, _ = self.predict(flux, error, zabs, mask, zfac=zfac, batch=batch)
        return self.sample_spectra(error, zabs, mask, n_samples=n_samples, seed=seed, offset=offset, hmean=hmean, hcov=hcov,
                                   zfac=zfac, batch=batch)

    def _loader_slices(self, dataloader, batch_size):
        """the slices predict_to_npz and the forest statistics walk: (first dataloader index, keyword inputs of predict / forest,
        paths)"""
        n = len(dataloader)
        for s in range(0, n, batch_size):
            # rows of the resident arrays, no copy (the resident form carries the factors, never zabs: with use_factored_z off or
            # a custom tau the loader materialises the four tensors)
            if hasattr(dataloader, "rows_batch") and self._tau_callable is None and (self.use_factored_z or self.Nb == 0):
                rb, paths = dataloader.rows_batch(s, min(s + batch_size, n))
                yield s, {"batch": rb}, paths
            elif hasattr(dataloader, "get_rows"):                # one launch for the whole slice
                f, e, z, m, paths = dataloader.get_rows(s, min(s + batch_size, n))
                yield s, {"flux": f, "error": e, "zabs": z, "mask": m}, paths
            else:                                                # the reference's per-spectrum contract
                items = [dataloader[i] for i in range(s, min(s + batch_size, n))]
                f, e, z, m = (torch.stack([it[j] for it in items]) for j in range(4))
                yield s, {"flux": f, "error": e, "zabs": z, "mask": m}, [it[4] for it in items]

    def predict_to_npz(self, dataloader, output_dir, batch_size=4096, n_samples=0, seed=0, n_replicates=0, forest=False):
        """The predict mode of the reference's main.py:87-98 for a whole dataloader: one
        ``<basename>`` .npz per spectrum with keys ll, hmean, hcov, cont, uncertainty and the
        reference's shapes ((1,1), (Nh,1), (Nh,Nh), (Npix,), (Npix,)); the posterior runs batched.
        ``n_samples`` > 0 adds ``cont_samples`` (S, Npix): continua drawn from the posterior with ``seed``, the global row of a
        spectrum being its dataloader index (so the files do not depend on ``batch_size``).  ``n_replicates`` > 0 adds
        ``flux_replicates`` (K, Npix): posterior-predictive replicates of the spectrum under its own error and mask
        (``sample_spectra``), same ``seed`` and global row.  ``forest`` adds ``transmission`` and ``transmission_ivar`` (Nb,):
        flux over the posterior-mean continuum on the blue side and its inverse variance (``QFA.forest`` with this
        prediction's hmean and unc)."""
        os.makedirs(output_dir, exist_ok=True)
        written = []
        for s, inputs, paths in self._loader_slices(dataloader, batch_size):
            res = self.predict(**inputs)
            samples = None
            if n_samples > 0:
                samples = self.sample_continua(n_samples=n_samples, seed=seed, offset=s, hmean=res[1], hcov=res[2]).cpu().numpy()
            replicates = None
            if n_replicates > 0:
                replicates = self.sample_spectra(n_samples=n_replicates, seed=seed, offset=s, hmean=res[1], hcov=res[2],
                                                 **{k: v for k, v in inputs.items() if k != "flux"}).cpu().numpy()
            trans = tivar = None
            if forest:
                trans, tivar, _ = self.forest(**inputs, hmean=res[1], unc=res[4])
                trans, tivar = trans[:, 0].cpu().numpy(), tivar[:, 0].cpu().numpy()
            ll, hmean, hcov, cont, unc = (x.cpu().numpy() for x in res)
            for r, path in enumerate(paths):
                name = os.path.basename(str(path))
                if not name.endswith(".npz"):
                    name += ".npz"
                extra = {} if samples is None else {"cont_samples": samples[r]}
                if replicates is not None:
                    extra["flux_replicates"] = replicates[r]
                if trans is not None:
                    extra["transmission"], extra["transmission_ivar"] = trans[r], tivar[r]
                np.savez(os.path.join(output_dir, name), ll=ll[r].reshape(1, 1), hmean=hmean[r].reshape(self.Nh, 1),
                         hcov=hcov[r], cont=cont[r], uncertainty=unc[r], **extra)
                written.append(name)
        return written

    def save_checkpoint(self, path, optimizer=None):
        """Parameters + mu in the reference's .npz layout (model.py:254-280) plus, optionally, the Adam
        state (i, m_*, v_*) the reference never saves -- so that a resumed run continues exactly."""
        arrs = {k: getattr(self, k).detach().cpu().numpy() for k in PARAM_KEYS}
        if self.mu is not None:
            arrs["mu"] = self.mu.detach().cpu().numpy()
        if optimizer is not None:
            arrs["adam_i"] = np.asarray(optimizer.i)
            for k in PARAM_KEYS:
                arrs["adam_m_" + k] = optimizer.m[k].detach().cpu().numpy()
                arrs["adam_v_" + k] = optimizer.v[k].detach().cpu().numpy()
        if self.em_running is not None:
            arrs["em_stats"] = self.em_running.buf.detach().cpu().numpy()
        np.savez(path, **arrs)

    def load_checkpoint(self, path, optimizer=None):
        """Inverse of save_checkpoint (c0 is read from c0: this is not the reference loader)."""
        f = np.load(path)
        def T(x):
            return torch.tensor(np.asarray(x), dtype=f32, device=self.device).contiguous()
        for k in PARAM_KEYS:
            setattr(self, k, T(f[k]))
        if "mu" in f.files:
            self.mu = T(f["mu"])
        if optimizer is not None and "adam_i" in f.files:
            optimizer.load_state_dict({"i": int(f["adam_i"]), "m": {k: T(f["adam_m_" + k]) for k in PARAM_KEYS},
                                       "v": {k: T(f["adam_v_" + k]) for k in PARAM_KEYS}})
        if "em_stats" in f.files:
            self.em_running = EMStats(T(f["em_stats"]), self.Npix, self.Nh)
        if self._dp:
            self.sync_replicas(optimizer)

    def prediction_for_single_spectra(self, flux, error, zabs, mask):
        """reference QFA/model.py:160-180: ll (1,1), hmean (Nh,1), hcov (Nh,Nh), cont (Npix,), unc (Npix,)."""
        ll, hmean, hcov, cont, unc = self.predict(flux[None, :], error[None, :], zabs[None, :], mask[None, :])
        return ll.reshape(1, 1), hmean.reshape(self.Nh, 1), hcov[0], cont[0], unc[0]

    def step(self, optimizer, delta=None, error=None, zabs=None, mask=None, events=None, zfac=None, batch=None, inplace=False):
        """forward -> Adam.update -> clip, all on device, no host sync (model.py:212-214, 316).
        Returns the (1,1) loss tensor.  ``batch``: a ``ResidentBatch`` in the place of the four tensors."""
        if hasattr(optimizer, "update_from_accum"):
            # sum / count and Adam + clip in one launch: the step never looks at the gradients (bit-identical to the two calls)
            acc = self._global_sums(delta, error, zabs, mask, events, zfac, batch)
            loss, new = optimizer.update_from_accum(self, acc, clip=self._clip_table(), inplace=inplace)
        else:
            loss, grads = self.forward(delta, error, zabs, mask, events=events, zfac=zfac, batch=batch)
            new = optimizer.update(self.parameters, grads, clip=self._clip_table(), inplace=inplace)
        if not inplace:
            for k in PARAM_KEYS:
                setattr(self, k, new[k])
        return loss

    # ------------------------------------------------------------------ closed-form EM update of F
    def em_statistics(self, delta=None, error=None, zabs=None, mask=None, *, zfac=None, batch=None, stats=None, nll=None):
        """Sufficient statistics of the closed-form update of F for one (shard of a) batch at the current parameters
        (qfa_em_stats_f32): S2_i = sum_s wD A^2 (C_s^-1 + y_s y_s^T), S1_i = sum_s wD A delta y_s, cnt_i, sum NLL, B.
        Returns an ``EMStats``; ``stats`` given: the sums are ADDED to it.  ``nll``: optional (B,) tensor for the per-spectrum
        NLL.  Input forms, ``auto_factor_zabs`` and graph capture as ``accumulate``; no float atomics in any mode."""
        ps = self._params_struct()
        if batch is not None:
            B = batch.B
            bs, keep = self._batch_struct_rows(batch)
        else:
            B = self._check_batch_shapes(delta, error, zabs, mask)
            bs, keep = self._batch_struct(delta, error, zabs, mask, zfac)
        h = _lib.lib()
        need = h.qfa_em_workspace_bytes(int(B), self.Npix, self.Nh)
        if need == 0:
            raise _lib.QFAHipError(f"unsupported shape B={B} Npix={self.Npix} Nh={self.Nh}")
        ws = self._scratch("em_ws", need)
        flags = 0
        if stats is None:
            stats = EMStats(torch.empty(h.qfa_em_floats(self.Npix, self.Nh), dtype=f32, device=self.device), self.Npix, self.Nh)
            flags = _lib.F_ZERO_ACCUM
        elif stats.Npix != self.Npix or stats.Nh != self.Nh:
            raise _lib.QFAHipError(f"stats of shape ({stats.Npix}, {stats.Nh}); the model has ({self.Npix}, {self.Nh})")
        if nll is not None and (nll.dtype != f32 or nll.numel() != B or not nll.is_contiguous()):
            raise _lib.QFAHipError(f"nll: expected a contiguous float32 tensor of {B} elements")
        _lib.check(h.qfa_em_stats_f32(
            C.byref(ps), C.byref(bs), C.byref(self._tau_model), int(B), self.Npix, self.Nb, self.Nh,
            _lib.require_device_tensor(stats.buf, f32, "stats"), C.c_void_p(nll.data_ptr()) if nll is not None else None,
            C.c_void_p(ws.data_ptr()), ws.numel(), flags | (int(self.flags) & _lib.F_SYNC),
            _lib.current_stream(self.device)), "qfa_em_stats_f32")
        return stats

    def _em_update(self, stats, ridge=0.0, damping=1.0):
        """F <- F + damping ((S2 + ridge I)^-1 S1 - F) in place (qfa_em_update_f_f32); the device counter of skipped rows"""
        self._params_struct()
        if stats.Npix != self.Npix or stats.Nh != self.Nh:
            raise _lib.QFAHipError(f"stats of shape ({stats.Npix}, {stats.Nh}); the model has ({self.Npix}, {self.Nh})")
        nsk = self._ws.get("em_skipped")
        if nsk is None:
            nsk = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ws["em_skipped"] = nsk
        fp = _lib.require_device_tensor(self.F, f32, "F")
        _lib.check(_lib.lib().qfa_em_update_f_f32(
            _lib.require_device_tensor(stats.buf, f32, "stats"), fp, self.Npix, self.Nh, float(ridge), float(damping), fp,
            C.c_void_p(nsk.data_ptr()), _lib.current_stream(self.device)), "qfa_em_update_f_f32")
        return nsk

    def em_update_F(self, stats, ridge=0.0, damping=1.0):
        """The closed-form M-step of F from ``stats`` (an ``EMStats``), in place on ``self.F``.  Rows no spectrum observes
        (cnt = 0) and rows whose system is not positive definite stay as they are; returns their number (one host
        synchronisation; during a graph capture the device counter is returned instead)."""
        nsk = self._em_update(stats, ridge, damping)
        if torch.cuda.is_current_stream_capturing():
            return nsk
        return int(nsk.item())

    def _em_global(self, delta, error, zabs, mask, zfac=None, batch=None):
        """statistics of the (global) batch: this rank's sums, all-reduced under data parallelism"""
        if (batch.B if batch is not None else delta.shape[0]) == 0:
            if not self._dp:
                raise _lib.QFAHipError("em_step: empty batch")
            st = EMStats(torch.zeros(_lib.lib().qfa_em_floats(self.Npix, self.Nh), dtype=f32, device=self.device),
                         self.Npix, self.Nh)
        else:
            st = self.em_statistics(delta, error, zabs, mask, zfac=zfac, batch=batch)
        if self._dp:
            from .distributed import all_reduce_accum
            all_reduce_accum(st.buf, self._dp_group)
        return st

    def em_step(self, delta=None, error=None, zabs=None, mask=None, *, zfac=None, batch=None, ridge=0.0, damping=1.0):
        """One EM step of F on a batch: statistics (all-reduced under ``enable_data_parallel``) and the closed-form update, all
        on the device, no host sync.  Returns the (1, 1) mean NLL at the parameters the statistics were taken with, as
        ``step`` reports it.  The other parameters stay as they are."""
        st = self._em_global(delta, error, zabs, mask, zfac, batch)
        self._em_update(st, ridge, damping)
        return st.loss

    def _train_step_em(self, optimizer, batch_args, em_rho, em_ridge):
        """``train(f_update="em")``: Adam + clip for Psi, omega, tau0, beta, c0 (F left out of the tensor list), then, at the
        parameters after that update, the statistics of the same batch blended into the running ones and the update of F"""
        loss, grads = self.forward(**batch_args)
        rest = [k for k in PARAM_KEYS if k != "F"]
        new = optimizer.update({k: getattr(self, k) for k in rest}, {k: grads[k] for k in rest}, clip=self._clip_table())
        for k in rest:
            setattr(self, k, new[k])
        st = self._em_global(batch_args.get("delta"), batch_args.get("error"), batch_args.get("zabs"), batch_args.get("mask"),
                             batch=batch_args.get("batch"))
        if self.em_running is None:
            self.em_running = st
        else:
            self.em_running.blend_(st, em_rho)
        self._em_update(self.em_running, em_ridge, 1.0)
        return loss

    def step_graph(self, optimizer, batch_size, resident=None):
        """A captured hipGraph of one training step for batches of ``batch_size`` spectra (StepGraph)."""
        return StepGraph(self, optimizer, batch_size, resident=resident)

    def train(self, optimizer, dataloader, n_epochs, output_dir="./result", save_interval=5, smooth_interval=5,
              quiet=False, logger=None, use_graph=False, graph_steps=8, f_update="adam", em_rho=1.0, em_ridge=0.0):
        """Training loop with the reference's control flow (reference QFA/model.py:183-231):
        Niter = data_size // batch_size (quirk Q5), optimizer.step() once per epoch (Q4), early
        stop the first time the epoch-mean NLL is negative (Q6), smooth / save cadence.
        ``use_graph``: replay a captured hipGraph of the step for the full-size batches (small batches are
        launch-bound: ~15 launches of a few microseconds each); same arithmetic, parameters updated in place.
        ``graph_steps``: consecutive steps per replay with a resident loader (StepGraph; the tail of an epoch runs eagerly).
        ``f_update``: "adam" (default: the reference's loop) or "em": Adam moves Psi, omega, tau0, beta, c0 and F gets its
        closed-form update from the statistics of the same batch, taken after the Adam update and blended into the running
        statistics ``self.em_running`` with ``em_rho`` (1.0 = replace), ridge ``em_ridge``; the step runs eagerly (no graph)."""
        if f_update not in ("adam", "em"):
            raise ValueError(f"f_update = {f_update!r}: expected 'adam' or 'em'")
        em = f_update == "em"
        os.makedirs(output_dir, exist_ok=True)
        output_dir = os.path.join(output_dir, "checkpoints")
        os.makedirs(output_dir, exist_ok=True)
        self.mu = torch.tensor(np.asarray(dataloader.mu), dtype=f32).to(self.device)
        Niter = dataloader.data_size // dataloader.batch_size
        if self._dp:
            # replicated state must be identical before the first update (and the loader must be the sharded kind:
            # same number of steps on every rank, or the all-reduce deadlocks on an uneven tail)
            import torch.distributed as dist
            if getattr(dataloader, "world", 1) != dist.get_world_size(self._dp_group):
                raise _lib.QFAHipError("data-parallel train() needs a dataloader sharded over the same ranks "
                                       "(DeviceDataloader(rank=, world=))")
            self.check_replicas(optimizer)
        # the captured step graph is a single-process tool (launch-bound small batches); under data parallelism the
        # per-rank batch is large (c4: 125 000 spectra) and the collective stays an eager RCCL call
        # A loader that keeps the data set resident (DeviceDataloader.next_batch_rows) hands over row numbers instead of a
        # materialised copy of every batch (the reference rebuilds delta per batch on the host, dataloader.py:124-138, although
        # it depends on mu and tau only); a custom tau callable needs the materialised zabs
        resident = hasattr(dataloader, "next_batch_rows") and self._tau_callable is None and (self.use_factored_z or self.Nb == 0)
        sg = None
        if use_graph and not self._dp and not em:
            sg = StepGraph(self, optimizer, dataloader.batch_size, resident=dataloader if resident else None,
                           steps=graph_steps if resident else 1)
        # Side effects under data parallelism: the replicas are identical, so ONE rank prints, logs and writes the
        # checkpoints (concurrent np.savez of the same path from every rank can interleave into a corrupt zip); the
        # others wait at a barrier so that nobody reads a half-written file.
        lead = True
        if self._dp:
            import torch.distributed as dist
            lead = dist.get_rank(self._dp_group) == 0

        def save(name):
            if lead:
                self.save_to_npz(output_dir, name)
            if self._dp:
                import torch.distributed as dist
                dist.barrier(group=self._dp_group)

        for epoch in range(n_epochs):
            dataloader.rewind()
            total = torch.zeros((), dtype=torch.float64, device=self.device)
            t0 = time.time()
            while dataloader.have_next_batch():
                if em and resident:
                    loss = self._train_step_em(optimizer, {"batch": dataloader.next_batch_rows()}, em_rho, em_ridge)
                elif em:
                    d, e, z, m = dataloader.next_batch()
                    loss = self._train_step_em(optimizer, {"delta": d, "error": e, "zabs": z, "mask": m}, em_rho, em_ridge)
                elif sg is not None and sg.fits(dataloader):
                    loss = sg.run_next(dataloader)
                elif resident:
                    loss = self.step(optimizer, batch=dataloader.next_batch_rows())
                else:
                    d, e, z, m = dataloader.next_batch()
                    loss = self.step(optimizer, d, e, z, m)
                total += loss.reshape(()).double()
            optimizer.step()
            # every step of the epoch is queued, none may have run yet: draw and upload the next epoch's shuffle now, beside
            # the GPU's work, not between two epochs (at 4 x 10^5 resident rows the host shuffle is 5 ms = 1.4 steps at c3)
            if epoch + 1 < n_epochs and hasattr(dataloader, "prefetch_epoch"):
                dataloader.prefetch_epoch()
            total_loss = total.item() / Niter          # one host sync per epoch; ZeroDivisionError if Niter == 0
            msg = "epoch: {:03d}/{:03d}  ;  loss:  {:.2f}  ;  time:  {:.2f} s ".format(
                epoch, n_epochs, total_loss, time.time() - t0)
            if not quiet and lead:
                print(msg)
            if logger is not None and lead:
                logger.info(msg)
            if total_loss < 0.:
                self.smooth()
                save("model_parameters_epoch_%02i.npz" % (epoch + 1))
                break
            if (epoch + 1) % smooth_interval == 0:
                self.smooth()
            if (epoch + 1) % save_interval == 0:
                save("model_parameters_epoch_%02i.npz" % (epoch + 1))

    fit = train

    # ------------------------------------------------------------------ checkpoints
    def save_to_npz(self, output_dir: str, file_name: str):
        """reference QFA/model.py:254-280: keys mu, F, Psi, omega, tau0, c0, beta."""
        os.makedirs(output_dir, exist_ok=True)
        arrs = {k: getattr(self, k).detach().cpu().numpy() for k in PARAM_KEYS}
        arrs["mu"] = self.mu.detach().cpu().numpy()
        final = os.path.join(output_dir, file_name)
        tmp = final + f".tmp{os.getpid()}.npz"          # complete file under a private name, then an atomic rename
        np.savez(tmp, **arrs)
        os.replace(tmp, final)

    def load_from_npz(self, path: str, reference_c0_quirk: bool = True):
        """reference QFA/model.py:282-295.  With ``reference_c0_quirk`` (default) c0 is read from
        the file's ``beta`` entry exactly as the reference does (model.py:295, quirk Q1)."""
        f = np.load(path)
        def T(x):
            return torch.tensor(np.asarray(x), dtype=f32, device=self.device).contiguous()
        self.mu = T(f["mu"])
        self.F = T(f["F"])
        self.omega = T(f["omega"])
        self.Psi = T(f["Psi"])
        self.tau0 = T(f["tau0"])
        self.beta = T(f["beta"])
        if reference_c0_quirk and "c0" in f.files and float(np.asarray(f["c0"])) != float(np.asarray(f["beta"])):
            import warnings
            warnings.warn(f"{path}: c0 is read from the file's 'beta' entry ({float(np.asarray(f['beta'])):g}) as the "
                          f"reference does (QFA/model.py:295); the file's own c0 is {float(np.asarray(f['c0'])):g}. "
                          "Pass reference_c0_quirk=False (config MODEL.REFERENCE_C0_QUIRK) to read c0.", stacklevel=2)
        self.c0 = T(f["beta"] if reference_c0_quirk else f["c0"])
        if self._dp:
            self.sync_replicas()


class StepGraph(object):
    """One training step (forward -> sum/count -> Adam + clip, model.py:212-214) captured as a hipGraph.

    The step of a small batch is launch-bound; the graph replays its ~15 kernels with one submission.  Inputs
    live in fixed buffers (a DeviceDataloader builds its batches straight into them, other loaders are copied),
    parameters and Adam moments are updated in place.  The learning rate and the bias-correction index are
    kernel arguments by value, so the graph is re-captured when they (or a parameter tensor) change -- once per
    epoch in ``QFA.train``.  The first step after such a change runs eagerly (it also warms the workspace up)."""

    def __init__(self, model, optimizer, batch_size, resident=None, steps=1):
        """``resident``: a loader with the resident form (``next_rows_into`` / ``rows_view``): the graph then reads the
        loader's resident arrays through ONE fixed buffer of row numbers, refilled per replay by a device-side copy of
        4 B bytes per step, instead of four batch-sized input buffers.  ``steps`` (resident form only): consecutive training
        steps per replay -- the step of the reference's default batch (500 spectra) is 80 us of kernels, and one graph launch
        plus the refill per step costs half of that again; ``steps`` = 8 replays eight steps (eight consecutive batches of the
        epoch's order, parameters and Adam moments updated in place between them) with one launch and one refill.  ``run``
        then returns the SUM of the steps' losses."""
        self.model, self.opt, self.B = model, optimizer, int(batch_size)
        dev = model.device
        self.resident = resident
        self.steps = int(steps) if resident is not None else 1
        if self.steps < 1:
            raise ValueError("steps >= 1")
        if resident is not None:
            self.rows = torch.zeros((self.steps * self.B,), dtype=torch.int32, device=dev)
            self.buf = None
        else:
            self.buf = (torch.empty((self.B, model.Npix), dtype=f32, device=dev),
                        torch.empty((self.B, model.Npix), dtype=f32, device=dev),
                        torch.empty((self.B, model.Nb), dtype=f32, device=dev),
                        torch.empty((self.B, model.Npix), dtype=torch.bool, device=dev))
        self.graph, self.key, self.loss = None, None, None
        self.replays = 0

    @property
    def rb(self):
        """the loader's resident arrays (as they are NOW: set_tau rebuilds them) seen through the fixed buffer of row numbers"""
        return self.resident.rows_view(self.rows)

    def _rb_step(self, k):
        return self.resident.rows_view(self.rows[k * self.B:(k + 1) * self.B])

    def _key(self):
        # everything the captured launches bake in: scalars passed by value and every buffer address
        m, o = self.model, self.opt
        return ((o.i, float(o.scheduled_lr), float(o.b1), float(o.b2), float(o.eps), float(o.weight_decay),
                 bool(m.exact_gradients))
                + tuple(getattr(m, k).data_ptr() for k in PARAM_KEYS)
                + tuple(o.m[k].data_ptr() for k in PARAM_KEYS) + tuple(o.v[k].data_ptr() for k in PARAM_KEYS)
                + (tuple(t.data_ptr() for t in (self.rb.delta, self.rb.error, self.rb.mask, self.rb.zq1))
                   if self.resident is not None else ()))

    def _body(self):
        m = self.model
        if self.resident is None:
            return m.step(self.opt, *self.buf, inplace=True)
        total = None
        for k in range(self.steps):                              # consecutive steps: each sees the previous one's update
            loss = m.step(self.opt, batch=self._rb_step(k), inplace=True)
            total = loss if total is None else total + loss
        return total

    def fits(self, dataloader):
        if self.resident is not None and self.steps > 1:
            return dataloader is self.resident and dataloader.full_batches_left() >= self.steps
        n = dataloader.next_batch_size() if hasattr(dataloader, "next_batch_size") else None
        return n is None or n == self.B

    def _fill(self, dataloader):
        if self.resident is not None:
            if dataloader is not self.resident:
                raise _lib.QFAHipError("StepGraph(resident=loader) replays batches of that loader only")
            dataloader.next_rows_into(self.rows)
            return True
        if hasattr(dataloader, "next_batch_size"):
            dataloader.next_batch(out=self.buf)
            return True
        batch = dataloader.next_batch()
        if batch[0].shape[0] != self.B:
            return batch
        for dst, src in zip(self.buf, batch):
            dst.copy_(src)
        return True

    def run_next(self, dataloader):
        filled = self._fill(dataloader)
        if filled is not True:                                   # a short last batch of a foreign loader
            return self.model.step(self.opt, *filled)
        return self.run()

    def run(self):
        """one step on the batch in ``self.buf``"""
        m = self.model
        for k in PARAM_KEYS:                                     # in-place updates need plain float32 storage
            p = getattr(m, k)
            if p.dtype != f32 or not p.is_contiguous():
                setattr(m, k, p.to(f32).contiguous())
        key = self._key()
        if key != self.key:
            self.graph, self.key = None, key
            return self._body()                                  # eager: first step with these scalars
        if self.graph is None:
            torch.cuda.synchronize(m.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.loss = self._body()
            self.graph = g
        self.graph.replay()
        self.replays += 1
        return self.loss


QFAModel = QFA
