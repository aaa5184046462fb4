"""Configuration with the reference's keys, without yacs.

Same tree, defaults, YAML merge (``BASE`` chaining), ``--opts KEY VALUE`` pairs and command-line overrides as
reference QFA/config.py:15-152 / main.py:16-44; the container is a plain attribute dict (``cfg.DATA.BATCH_SIZE``).
"""
from __future__ import annotations

import copy
import os

import yaml


class Node(dict):
    """dict with attribute access; ``dump()`` writes YAML like yacs' CfgNode.dump()"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def dump(self):
        def plain(n):
            return {k: plain(v) if isinstance(v, dict) else v for k, v in n.items()}
        return yaml.safe_dump(plain(self), default_flow_style=False)


def _node(d):
    return Node({k: _node(v) if isinstance(v, dict) else v for k, v in d.items()})


DEFAULTS = {                                        # reference QFA/config.py:15-63
    "BASE": [""], "TYPE": "train", "GPU": 0,
    "DATA": {"DATA_DIR": "", "VALIDATION_DIR": "", "OUTPUT_DIR": "", "CATALOG": "", "VALIDATION_CATALOG": "",
             "DATA_NUM": 10000, "VALIDATION_NUM": 1000, "BATCH_SIZE": 500, "SNR_MIN": 2, "SNR_MAX": 100, "Z_MIN": 2,
             "Z_MAX": 3.5, "NUM_MASK": 0, "LAMMIN": 1030.0, "LAMMAX": 1600.0, "LOGLAM_DELTA": 1e-4, "NPROCS": 24,
             "VALIDATION": False},
    "MODEL": {"NH": 8, "TAU": "becker", "RESUME": "",
              # not in the reference: its load_from_npz reads c0 from the file's 'beta' entry (QFA/model.py:295, quirk
              # Q1).  True keeps that (the reference's shipped models and stored answers need it); set it to False
              # for models trained and saved by this package, whose files hold the true c0.
              "REFERENCE_C0_QUIRK": True,
              # not in the reference: predict mode adds N_SAMPLES continua drawn from the posterior to every file
              # (cont_samples, (N_SAMPLES, Npix)); SAMPLE_SEED seeds the counter-based generator (include/qfa_hip.h)
              "N_SAMPLES": 0, "SAMPLE_SEED": 0,
              # not in the reference: predict mode adds N_REPLICATES posterior-predictive replicates of every spectrum under its
              # own noise and mask to every file (flux_replicates, (N_REPLICATES, Npix)); same SAMPLE_SEED
              "N_REPLICATES": 0,
              # not in the reference: train with the exact gradient of the mean NLL instead of the reference's formulas
              # (QFA.exact_gradients, include/qfa_hip.h QFA_F_EXACT_GRAD); off = the reference's update
              "EXACT_GRADIENTS": False,
              # not in the reference: predict mode adds the forest transmission flux / continuum of the blue side and its inverse
              # variance to every file (transmission, transmission_ivar, (Nb,)); FOREST_NBINS > 0 also writes
              # mean_transmission.npz, the stack in FOREST_NBINS bins of [FOREST_ZMIN, FOREST_ZMAX), repeated over N_SAMPLES
              # posterior draws when that is set (QFA.forest / mean_transmission)
              "FOREST": False, "FOREST_ZMIN": 0.0, "FOREST_ZMAX": 0.0, "FOREST_NBINS": 0,
              # not in the reference: predict mode with P1D_SEGMENTS > 0 (needs FOREST_NBINS > 0) also writes flux_power.npz, the
              # 1D flux power spectrum of P1D_SEGMENTS segments of the blue side stacked in P1D_NZBINS bins of [FOREST_ZMIN,
              # FOREST_ZMAX), per posterior draw when N_SAMPLES is set, the contrast formed with the stack of
              # mean_transmission.npz; a segment needs P1D_MIN_USED_FRAC of its pixels used (QFA.flux_power)
              "P1D_SEGMENTS": 0, "P1D_NZBINS": 4, "P1D_MIN_USED_FRAC": 0.75,
              # not in the reference: P1D_NBANDS > 0 (needs P1D_SEGMENTS > 0) also writes flux_power_bands.npz, the power in
              # P1D_NBANDS equal bands of k from the fundamental to Nyquist and the covariance matrix between the bands per z-bin,
              # from the scatter of the segments and, when N_SAMPLES is set, over the posterior draws (QFA.band_power)
              "P1D_NBANDS": 0,
              # not in the reference: XI_NLAGS > 0 (needs P1D_SEGMENTS > 0, at most the segment length) also writes
              # flux_correlation.npz, the pair-weighted correlation function of the same segments at the lags 0 .. XI_NLAGS - 1
              # pixels per z-bin, which carries no window of the mask; pixels are weighted by 1 / (noise variance + XI_SIGMA2_LSS)
              # (QFA.flux_correlation)
              "XI_NLAGS": 0, "XI_SIGMA2_LSS": 0.0,
              # not in the reference: PDF_NBINS > 0 (needs P1D_SEGMENTS > 0, at most 64) also writes flux_pdf.npz, the probability
              # distribution of the transmitted flux of the same segments in PDF_NBINS bins of [PDF_TMIN, PDF_TMAX) per z-bin with
              # the covariance matrix between the bins; PDF_CLAMP counts pixels outside the range in the first / last bin,
              # PDF_RELATIVE bins T / <T>(z), PDF_IVAR_MIN leaves out pixels of lower inverse variance (QFA.flux_pdf)
              "PDF_NBINS": 0, "PDF_TMIN": 0.0, "PDF_TMAX": 1.0, "PDF_CLAMP": True, "PDF_RELATIVE": False, "PDF_IVAR_MIN": 0.0,
              # not in the reference: VAR_NOCT > 0 (needs P1D_SEGMENTS > 0) also writes variance_function.npz, the variance of delta_F
              # of the same segments in VAR_NOCT octaves of the pipeline's noise variance from 2^VAR_ELO on, 2^VAR_SUB bins per octave
              # (at most 64 bins), per z-bin, and the fit var = eta v + sigma2_lss on the bins of at least VAR_MIN_COUNT pixels;
              # VAR_DMAX > 0 leaves out pixels with |delta_F| above it (QFA.variance_function)
              "VAR_NOCT": 0, "VAR_ELO": -12, "VAR_SUB": 1, "VAR_DMAX": 0.0, "VAR_MIN_COUNT": 100,
              # not in the reference: BOOT_N > 0 makes every segment statistic predict mode writes (flux_power, flux_power_bands,
              # flux_correlation, flux_pdf, variance_function) also write <its file stem>_bootstrap.npz: its estimate in BOOT_N Poisson
              # bootstrap replicates over quasars and their covariance matrix per z-bin; BOOT_SEED seeds the weights (QFA.bootstrap)
              "BOOT_N": 0, "BOOT_SEED": 0,
              # not in the reference: BAL = True makes predict mode also write bal_catalog.csv (one row per trough: file, line, v_min,
              # v_max, bi, ai; io.read_bal_csv, python -m qfa_amd.preprocess --bal_catalog) and bal_scan.npz: BI and AI of C IV and
              # Si IV under the posterior continuum, per posterior draw when N_SAMPLES is set (QFA.bal_catalog).  BAL_THR: the
              # normalised flux a trough lies below; BAL_SMOOTH: odd boxcar width 1 .. 15; BAL_MAX_GAP: masked pixels 0 .. 16 a trough
              # may bridge; BAL_NITER > 1 repeats predict -> find -> mask; BAL_MIN_AI: the AI in km/s above which a spectrum's troughs
              # are listed; BAL_PAD_KMS widens the troughs masked between iterations
              "BAL": False, "BAL_THR": 0.9, "BAL_SMOOTH": 1, "BAL_MAX_GAP": 0, "BAL_NITER": 1, "BAL_MIN_AI": 0.0, "BAL_PAD_KMS": 0.0,
              # not in the reference: ZSCAN = True makes predict mode also write redshift_catalog.csv (one row per spectrum: file,
              # z_cat, z, sigma_z, dv_kms, sigma_kms, best_s, offset, best_llr, at_edge; io.read_redshift_csv) and redshift_scan.npz:
              # the likelihood of every spectrum at the pixel shifts -ZSCAN_MAX_SHIFT .. ZSCAN_MAX_SHIFT between data and model
              # (QFA.redshift_catalog; the grid must be uniform in log wavelength)
              "ZSCAN": False, "ZSCAN_MAX_SHIFT": 20},
    "TRAIN": {"NEPOCHS": 500, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-1, "DECAY_ALPHA": 0.9, "DECAY_STEP": 10,
              "WINDOW_LENGTH_FOR_MU": 16,
              # not in the reference: "em" = F by its closed-form EM update, Adam for the other parameters (QFA.train
              # f_update / em_rho / em_ridge); "adam" = the reference's loop
              "F_UPDATE": "adam", "EM_RHO": 1.0, "EM_RIDGE": 0.0},
}

# command-line flag -> config key (reference QFA/config.py:92-139)
ARG_KEYS = {
    "gpu": "GPU", "n_epochs": "TRAIN.NEPOCHS", "learning_rate": "TRAIN.LEARNING_RATE",
    "weight_decay": "TRAIN.WEIGHT_DECAY", "decay_alpha": "TRAIN.DECAY_ALPHA", "decay_step": "TRAIN.DECAY_STEP",
    "data_dir": "DATA.DATA_DIR", "validation_dir": "DATA.VALIDATION_DIR", "output_dir": "DATA.OUTPUT_DIR",
    "catalog": "DATA.CATALOG", "validation_catalog": "DATA.VALIDATION_CATALOG", "data_num": "DATA.DATA_NUM",
    "validation_num": "DATA.VALIDATION_NUM", "batch_size": "DATA.BATCH_SIZE", "snr_min": "DATA.SNR_MIN",
    "snr_max": "DATA.SNR_MAX", "z_min": "DATA.Z_MIN", "z_max": "DATA.Z_MAX", "num_mask": "DATA.NUM_MASK",
    "nprocs": "DATA.NPROCS", "validation": "DATA.VALIDATION", "tau": "MODEL.TAU", "type": "TYPE",
}
# keys of DEFAULTS the reference does not have (tests/test_cli_config.py pins everything else against
# tests/golden/g12_config.json, extracted from the reference's config.py / main.py)
EXTRA_KEYS = ("MODEL.REFERENCE_C0_QUIRK", "MODEL.N_SAMPLES", "MODEL.SAMPLE_SEED", "MODEL.N_REPLICATES", "MODEL.EXACT_GRADIENTS",
              "MODEL.FOREST", "MODEL.FOREST_ZMIN", "MODEL.FOREST_ZMAX", "MODEL.FOREST_NBINS", "MODEL.P1D_SEGMENTS",
              "MODEL.P1D_NZBINS", "MODEL.P1D_MIN_USED_FRAC", "MODEL.P1D_NBANDS", "MODEL.XI_NLAGS", "MODEL.XI_SIGMA2_LSS", "MODEL.PDF_NBINS",
              "MODEL.PDF_TMIN", "MODEL.PDF_TMAX", "MODEL.PDF_CLAMP", "MODEL.PDF_RELATIVE", "MODEL.PDF_IVAR_MIN", "MODEL.VAR_NOCT", "MODEL.VAR_ELO",
              "MODEL.VAR_SUB", "MODEL.VAR_DMAX", "MODEL.VAR_MIN_COUNT", "MODEL.BOOT_N", "MODEL.BOOT_SEED", "MODEL.BAL",
              "MODEL.BAL_THR", "MODEL.BAL_SMOOTH", "MODEL.BAL_MAX_GAP", "MODEL.BAL_NITER", "MODEL.BAL_MIN_AI", "MODEL.BAL_PAD_KMS",
              "MODEL.ZSCAN", "MODEL.ZSCAN_MAX_SHIFT", "TRAIN.F_UPDATE", "TRAIN.EM_RHO", "TRAIN.EM_RIDGE")


def _set(cfg, dotted, value):
    node = cfg
    keys = dotted.split(".")
    for k in keys[:-1]:
        node = node[k]
    if keys[-1] not in node:
        raise KeyError(f"unknown config key {dotted}")
    old = node[keys[-1]]
    if isinstance(value, str) and not isinstance(old, str):          # KEY VALUE pairs arrive as text
        if isinstance(old, bool):
            value = value.strip().lower() in ("1", "true", "yes", "on")
        elif isinstance(old, int):
            value = int(value)
        elif isinstance(old, float):
            value = float(value)
        else:
            value = yaml.safe_load(value)
    if isinstance(old, float) and isinstance(value, int) and not isinstance(value, bool):
        value = float(value)
    node[keys[-1]] = value


def _merge(cfg, other, where):
    for k, v in other.items():
        if k not in cfg:
            raise KeyError(f"unknown config key {k} in {where}")
        if isinstance(v, dict):
            _merge(cfg[k], v, where)
        else:
            cfg[k] = v


def merge_from_file(cfg, path):
    """YAML file over the config, files named in its BASE list first (reference QFA/config.py:67-77)"""
    with open(path) as f:
        y = yaml.safe_load(f) or {}
    for base in y.get("BASE", [""]):
        if base:
            merge_from_file(cfg, os.path.join(os.path.dirname(path), base))
    _merge(cfg, y, path)


def get_config(args=None):
    """defaults <- --cfg file <- --opts pairs <- explicit flags (reference QFA/config.py:80-152)"""
    cfg = _node(copy.deepcopy(DEFAULTS))
    if args is None:
        return cfg
    if isinstance(getattr(args, "cfg", None), str):
        merge_from_file(cfg, args.cfg)
    opts = getattr(args, "opts", None)
    if opts:
        if len(opts) % 2:
            raise ValueError("--opts takes KEY VALUE pairs")
        for k, v in zip(opts[0::2], opts[1::2]):
            _set(cfg, k, v)
    for flag, key in ARG_KEYS.items():
        v = getattr(args, flag, None)
        if v:                                            # the reference ignores falsy values too
            _set(cfg, key, v)
    if getattr(args, "Nh", None):
        # the reference parses --Nh (main.py:25) and never applies it (QFA/config.py:92-139 has no such branch)
        import warnings
        warnings.warn("--Nh is accepted and ignored, as in the reference; use --opts MODEL.NH <n>", stacklevel=2)
    return cfg
