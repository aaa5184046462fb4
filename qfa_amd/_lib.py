"""ctypes binding of libqfa_hip.so (C-ABI declared in include/qfa_hip.h).

There is deliberately no fallback: if the shared library is missing, cannot be loaded, or a
tensor is not a contiguous float32/bool tensor on a HIP device, a ``QFAHipError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (no environment switch: tools/with_lib.py sets this attribute before the first lib() call for A/B timing of library variants)
LIB_PATH = os.path.join(_HERE, "libqfa_hip.so")

EXPORTS = (
    "qfa_abi_version", "qfa_tau_model", "qfa_workspace_bytes", "qfa_accum_floats",
    "qfa_nll_grad_f32", "qfa_nll_grad_events_f32", "qfa_nll_grad_det_f32", "qfa_nll_grad_ex_f32", "qfa_predict_ex_f32", "qfa_det_slab_bytes", "qfa_pixres_plan", "qfa_finalize_grads_f32", "qfa_predict_f32", "qfa_predict_events_f32",
    "qfa_adam_clip_f32",
    "qfa_adam_clip_multi_f32", "qfa_clip_f32", "qfa_smooth_f32", "qfa_tau_f32", "qfa_tauhi_f32", "qfa_omega_func_f32", "qfa_woodbury_f32", "qfa_build_batch_f32", "qfa_mu_estimate_f64",
    "qfa_mu_sums_f64", "qfa_mu_finish_f64", "qfa_build_resident_f32", "qfa_finalize_adam_clip_f32", "qfa_zabs_factor_f32",
    "qfa_sample_latent_f32", "qfa_continua_workspace_bytes", "qfa_continua_f32",
    "qfa_mock_workspace_bytes", "qfa_mock_spectra_f32",
    "qfa_em_floats", "qfa_em_workspace_bytes", "qfa_em_stats_f32", "qfa_em_update_f_f32",
    "qfa_forest_stack_doubles", "qfa_forest_workspace_bytes", "qfa_forest_f32",
    "qfa_p1d_stack_doubles", "qfa_p1d_workspace_bytes", "qfa_p1d_f32",
    "qfa_p1d_band_stack_doubles", "qfa_p1d_band_workspace_bytes", "qfa_p1d_band_chunk_segments", "qfa_p1d_band_f32",
    "qfa_xi_stack_doubles", "qfa_xi_workspace_bytes", "qfa_xi_f32",
    "qfa_flux_pdf_stack_doubles", "qfa_flux_pdf_workspace_bytes", "qfa_flux_pdf_f32",
    "qfa_variance_stack_doubles", "qfa_variance_workspace_bytes", "qfa_variance_f32",
    "qfa_preprocess_workspace_bytes", "qfa_preprocess_f32",
    "qfa_absorber_workspace_bytes", "qfa_absorber_mask_f32",
    "qfa_dla_profiles_f32", "qfa_template_scan_workspace_bytes", "qfa_template_scan_f32",
    "qfa_segment_codes_f32", "qfa_bootstrap_workspace_bytes", "qfa_bootstrap_f64",
    "qfa_obs_stack_doubles", "qfa_obs_stack_workspace_bytes", "qfa_obs_stack_f32", "qfa_calibrate_f32",
    "qfa_bal_scan_f32", "qfa_bal_mask_f32",
    "qfa_zscan_workspace_bytes", "qfa_redshift_scan_f32",
)

TAU_IDS = {"becker": 0, "fg": 1, "kamble": 2, "mock": 3}
ABI_VERSION = 4
# `flags` of qfa_nll_grad_ex_f32 / qfa_predict_ex_f32 (include/qfa_hip.h QFA_F_*)
F_PASS2_F32, F_PASS2_XDL, F_S3_FAST, F_PREDICT_F32, F_SYNC = 0x1, 0x2, 0x4, 0x8, 0x20
F_PASS2_PIXRES = 0x40
F_ZERO_ACCUM = 0x80
F_FOREST_UNIT_W = 0x200    # qfa_forest_f32: stack with w = 1 instead of w = ivar
F_XI_UNIT_W = 0x400        # qfa_xi_f32: w = 1 on a used pixel instead of 1 / (v + sigma2_lss)
F_PDF_RELATIVE = 0x800     # qfa_flux_pdf_f32: bin x = T / tbar(z) instead of x = T
F_PDF_CLAMP = 0x1000       # qfa_flux_pdf_f32: x outside the range counts in the first / last bin
F_OBS_UNIT_W = 0x2000      # qfa_obs_stack_f32: stack with w = 1 instead of w = ivar
OBS_MODES = {"log": 0, "linear": 1}    # qfa_obs_bins_t.mode (QFA_OBS_*)
ROW_TYPES = {"float32": 0, "float64": 1, "int32": 2}    # qfa_bootstrap_f64: QFA_ROW_* by the name of the rows' dtype
ABS_LYB, ABS_CORRECT = 0x1, 0x2    # qfa_absorber_t.flags (QFA_ABS_*)
F_EXACT_GRAD = 0x100       # exact gradients of mean NLL (opt-in; QFA.exact_gradients); the buffer carries the mode in slot 6


class QFAHipError(RuntimeError):
    pass


class TauModel(C.Structure):
    _fields_ = [("amp", C.c_float), ("scale", C.c_float), ("expo", C.c_float), ("offset", C.c_float)]


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("F", "Psi", "omega", "tau0", "c0", "beta")]


ADAM_MAX = 8


class AdamMulti(C.Structure):       # qfa_adam_multi_t
    _fields_ = [("p", C.c_void_p * ADAM_MAX), ("g", C.c_void_p * ADAM_MAX), ("m", C.c_void_p * ADAM_MAX),
                ("v", C.c_void_p * ADAM_MAX), ("p_out", C.c_void_p * ADAM_MAX), ("n", C.c_size_t * ADAM_MAX),
                ("lo", C.c_float * ADAM_MAX), ("hi", C.c_float * ADAM_MAX), ("count", C.c_int)]


class Batch(C.Structure):
    # qfa_batch_t (ABI v3: rows / row_stride = the resident, indexed input form)
    _fields_ = [(n, C.c_void_p) for n in ("delta", "error", "zabs", "mask", "A_blue", "zq1", "pix_ratio", "rows")] + \
               [("row_stride", C.c_int64)]


class ForestBins(C.Structure):      # qfa_forest_bins_t
    _fields_ = [("z0", C.c_float), ("dz", C.c_float), ("nbin", C.c_int), ("p_lo", C.c_int), ("p_hi", C.c_int)]


class P1DParams(C.Structure):       # qfa_p1d_t
    _fields_ = [("zT0", C.c_float), ("dzT", C.c_float), ("nT", C.c_int), ("St", C.c_int), ("p_lo", C.c_int), ("seg_len", C.c_int),
                ("nseg", C.c_int), ("min_used", C.c_int), ("z0", C.c_float), ("dz", C.c_float), ("nz", C.c_int)]


class P1DBandParams(C.Structure):   # qfa_p1d_band_t
    _fields_ = [("nband", C.c_int), ("band", C.c_void_p), ("weight", C.c_void_p), ("subtract_noise", C.c_int)]


class XiParams(C.Structure):        # qfa_xi_t
    _fields_ = [("nlag", C.c_int), ("sigma2_lss", C.c_float)]


class PDFParams(C.Structure):       # qfa_pdf_t
    _fields_ = [("t0", C.c_float), ("dt", C.c_float), ("nt", C.c_int), ("ivar_min", C.c_float)]


class VarParams(C.Structure):       # qfa_var_t
    _fields_ = [("e_lo", C.c_int), ("n_oct", C.c_int), ("sub", C.c_int), ("d_max", C.c_float)]


class PreprocessParams(C.Structure):   # qfa_preprocess_t
    _fields_ = [("min_coverage", C.c_double), ("norm_lo", C.c_double), ("norm_hi", C.c_double), ("snr_lo", C.c_double),
                ("snr_hi", C.c_double), ("norm_min_pixels", C.c_int)]


class AbsorberParams(C.Structure):     # qfa_absorber_t
    _fields_ = [("t_min", C.c_double), ("b_kms", C.c_double), ("snr_lo", C.c_double), ("snr_hi", C.c_double), ("flags", C.c_uint)]


class ObsBins(C.Structure):            # qfa_obs_bins_t
    _fields_ = [("u0", C.c_double), ("du", C.c_double), ("nbin", C.c_int), ("p_lo", C.c_int), ("p_hi", C.c_int), ("mode", C.c_uint)]


BAL_MAX_LINES, BAL_MAX_INDICES, BAL_MAX_TROUGHS, BAL_MAX_WIN = 4, 4, 8, 2048    # QFA_BAL_MAX_*
BAL_MODES = {"whole": 0, "after": 1}   # qfa_bal_index_t.mode (QFA_BAL_*)


class BalIndex(C.Structure):           # qfa_bal_index_t
    _fields_ = [("v_lo", C.c_double), ("v_hi", C.c_double), ("w_min", C.c_double), ("mode", C.c_uint)]


class BalParams(C.Structure):          # qfa_bal_t
    _fields_ = [("n_lines", C.c_int), ("n_indices", C.c_int), ("p_lo", C.c_int * BAL_MAX_LINES), ("p_hi", C.c_int * BAL_MAX_LINES),
                ("vedge", C.c_void_p * BAL_MAX_LINES), ("index", BalIndex * BAL_MAX_INDICES), ("thr", C.c_double),
                ("smooth", C.c_int), ("max_gap", C.c_int), ("trough_index", C.c_int)]


_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises QFAHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QFAHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C qfa_amd/csrc` (hipcc --offload-arch=gfx950). qfa_amd has no CPU fallback.")
    try:
        h = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise QFAHipError(f"cannot load {LIB_PATH}: {e}") from e
    p, i, f, d, sz, i64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int64
    sigs = {
        "qfa_abi_version": (i, []),
        "qfa_tau_model": (i, [i, i, C.POINTER(TauModel)]),
        "qfa_workspace_bytes": (sz, [i, i, i]),
        "qfa_accum_floats": (sz, [i, i, i]),
        "qfa_nll_grad_f32": (i, [C.POINTER(Params), C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i, p, p, p, sz, p]),
        "qfa_nll_grad_events_f32": (i, [C.POINTER(Params), C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i, p, p, p, sz,
                                        p, C.POINTER(C.c_void_p)]),
        "qfa_nll_grad_det_f32": (i, [C.POINTER(Params), C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i, p, p, p, sz,
                                     p, sz, p, C.POINTER(C.c_void_p)]),
        "qfa_nll_grad_ex_f32": (i, [C.POINTER(Params), C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i, p, p, p, sz,
                                    p, sz, C.c_uint, p, C.POINTER(C.c_void_p)]),
        "qfa_predict_ex_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i,
                                   p, p, p, p, p, p, sz, C.c_uint, p, C.POINTER(C.c_void_p)]),
        "qfa_det_slab_bytes": (sz, [i, i, i, i]),
        "qfa_finalize_grads_f32": (i, [p, p, i, i, i, i, p, p, p, p, p, p, p, p]),
        "qfa_predict_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i,
                                p, p, p, p, p, p, sz, p]),
        "qfa_predict_events_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i,
                                       p, p, p, p, p, p, sz, p, C.POINTER(C.c_void_p)]),
        "qfa_adam_clip_f32": (i, [p, p, p, p, p, sz, d, d, d, d, d, i, f, f, p]),
        "qfa_adam_clip_multi_f32": (i, [C.POINTER(AdamMulti), d, d, d, d, d, i, p]),
        "qfa_finalize_adam_clip_f32": (i, [p, i, i, i, C.POINTER(AdamMulti), d, d, d, d, d, i, p, p]),
        "qfa_clip_f32": (i, [p, p, sz, f, f, p]),
        "qfa_smooth_f32": (i, [p, p, i, i, i, p]),
        "qfa_tau_f32": (i, [p, p, sz, C.POINTER(TauModel), p]),
        "qfa_tauhi_f32": (i, [p, p, p, p, sz, p]),
        "qfa_omega_func_f32": (i, [p, p, p, p, p, sz, p]),
        "qfa_woodbury_f32": (i, [p, p, i, i, p, p, p, sz, p]),
        "qfa_build_batch_f32": (i, [p, p, p, p, p, d, p, i, i, i, i, i64, p, p, p, p, p]),
        "qfa_build_resident_f32": (i, [p, p, p, p, d, p, i, i64, i, i, i64, p, p, p, p]),
        "qfa_mu_estimate_f64": (i, [p, p, p, p, d, i, i, i, i, i64, i, p, p, p, p]),
        "qfa_mu_sums_f64": (i, [p, p, p, p, d, i, i, i, i, i64, p, p]),
        "qfa_mu_finish_f64": (i, [p, i, i, p, p, p]),
        "qfa_zabs_factor_f32": (i, [p, i, i, f, p, p, p, p]),
        "qfa_sample_latent_f32": (i, [p, p, i, i, i, C.c_uint64, i64, p, p]),
        "qfa_continua_workspace_bytes": (sz, [i, i]),
        "qfa_continua_f32": (i, [p, p, p, i64, i, i, p, p, sz, p]),
        "qfa_mock_workspace_bytes": (sz, [i, i]),
        "qfa_mock_spectra_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), p, i, i, i, i, i, C.c_uint64, i64,
                                     p, p, p, sz, p]),
        "qfa_em_floats": (sz, [i, i]),
        "qfa_em_workspace_bytes": (sz, [i, i, i]),
        "qfa_em_stats_f32": (i, [C.POINTER(Params), C.POINTER(Batch), C.POINTER(TauModel), i, i, i, i, p, p, p, sz, C.c_uint, p]),
        "qfa_em_update_f_f32": (i, [p, p, i, i, d, d, p, p, p]),
        "qfa_forest_stack_doubles": (sz, [i, i]),
        "qfa_forest_workspace_bytes": (sz, [i, i, i, i, i, i]),
        "qfa_forest_f32": (i, [p, p, C.POINTER(Batch), p, p, i, i, i, i, i, C.POINTER(ForestBins), f, C.c_uint, p, p, p, p, sz, p]),
        "qfa_p1d_stack_doubles": (sz, [i, i, i]),
        "qfa_p1d_workspace_bytes": (sz, [i, i, i, i, i, i]),
        "qfa_p1d_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), C.c_uint, p, p, p, p, sz, p]),
        "qfa_p1d_band_stack_doubles": (sz, [i, i, i]),
        "qfa_p1d_band_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        "qfa_p1d_band_chunk_segments": (i, []),
        "qfa_p1d_band_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), C.POINTER(P1DBandParams), C.c_uint, p, p,
                                 p, sz, p]),
        "qfa_xi_stack_doubles": (sz, [i, i, i]),
        "qfa_xi_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        "qfa_xi_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), C.POINTER(XiParams), C.c_uint, p, p, p, p, sz, p]),
        "qfa_flux_pdf_stack_doubles": (sz, [i, i, i]),
        "qfa_flux_pdf_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        "qfa_flux_pdf_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), C.POINTER(PDFParams), C.c_uint, p, p, p, sz, p]),
        "qfa_variance_stack_doubles": (sz, [i, i, i]),
        "qfa_variance_workspace_bytes": (sz, [i, i, i, i, i, i, i]),
        "qfa_variance_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), C.POINTER(VarParams), C.c_uint, p, p, p, sz, p]),
        "qfa_preprocess_workspace_bytes": (sz, [i, i, i]),
        "qfa_preprocess_f32": (i, [p, p, p, p, p, p, i, i, p, p, i, C.POINTER(PreprocessParams), p, p, p, p, p, sz, p]),
        "qfa_absorber_workspace_bytes": (sz, [i, i]),
        "qfa_absorber_mask_f32": (i, [p, p, p, p, i, i, p, p, p, p, i, p, p, C.POINTER(AbsorberParams), p, p, p, p, p, p, sz, p]),
        "qfa_dla_profiles_f32": (i, [p, i, d, d, i, d, d, i, d, i, p, p]),
        "qfa_template_scan_workspace_bytes": (sz, [i, i, i, i]),
        "qfa_template_scan_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), p, i, i, i, i, i, p, p, p, p, p, sz,
                                      C.c_uint, p]),
        "qfa_zscan_workspace_bytes": (sz, [i, i, i, i]),
        "qfa_redshift_scan_f32": (i, [C.POINTER(Params), p, C.POINTER(Batch), C.POINTER(TauModel), p, i, i, i, i, i, p, p, p, p, p, p, p, sz,
                                      C.c_uint, p]),
        "qfa_segment_codes_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, C.POINTER(P1DParams), p, p]),
        "qfa_bootstrap_workspace_bytes": (sz, [i, i, i, i, i, i]),
        "qfa_bootstrap_f64": (i, [p, i, p, i, i, i, i, i, i, C.c_uint64, i64, C.c_uint, p, p, sz, p]),
        "qfa_pixres_plan": (i, [i, i, i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "qfa_obs_stack_doubles": (sz, [i, i]),
        "qfa_obs_stack_workspace_bytes": (sz, [i, i, i, i, i]),
        "qfa_obs_stack_f32": (i, [p, p, C.POINTER(Batch), p, p, p, p, i, i, i, i, C.POINTER(ObsBins), f, C.c_uint, p, p, sz, p]),
        "qfa_calibrate_f32": (i, [p, p, p, p, i, i, p, i, d, d, C.c_uint, d, p, p, p, p]),
        "qfa_bal_scan_f32": (i, [p, p, C.POINTER(Batch), p, i, i, i, i, i, C.POINTER(BalParams), f, C.c_uint, p, p, p, p, p, p]),
        "qfa_bal_mask_f32": (i, [p, p, p, i, i, i, i, i, C.POINTER(d), i, d, p, p, p]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(h, name, None)
        if fn is None:
            raise QFAHipError(f"{LIB_PATH} does not export {name} (include/qfa_hip.h): rebuild it")
        fn.restype = res
        fn.argtypes = args
    if h.qfa_abi_version() != ABI_VERSION:
        raise QFAHipError(f"libqfa_hip.so ABI version {h.qfa_abi_version()}, expected {ABI_VERSION}")
    _lib = h
    return h


def check(status, what):
    if status == 0:
        return
    if status < 0:
        names = {-1: "QFA_E_NULL", -2: "QFA_E_SIZE", -3: "QFA_E_WORKSPACE", -4: "QFA_E_TAU", -5: "QFA_E_FLAGS"}
        raise QFAHipError(f"{what}: invalid argument ({names.get(status, status)})")
    raise QFAHipError(f"{what}: hipError_t {status}")


def tau_model(which="becker", series=1):
    if which not in TAU_IDS:
        raise NotImplementedError("currently available mean optical depth function: ['becker', 'fg', 'kamble']")
    t = TauModel()
    check(lib().qfa_tau_model(TAU_IDS[which], int(series), C.byref(t)), "qfa_tau_model")
    return t


def require_device_tensor(t, dtype, name):
    """Raw pointer of a contiguous tensor on a HIP device, or a loud error."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise QFAHipError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if t.device.type != "cuda":
        raise QFAHipError(f"{name}: tensor is on {t.device}; qfa_amd runs on a HIP device only (no CPU fallback)")
    if t.dtype != dtype:
        raise QFAHipError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise QFAHipError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _ptr(t):
    """raw pointer of a tensor the caller has checked, NULL for None"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def current_stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
