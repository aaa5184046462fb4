"""Command line of the reference's main.py on the MI355X path.

    python -m qfa_amd.cli --cfg config.yaml --type train  [--catalog ... --data_dir ... --output_dir ...]
    python -m qfa_amd.cli --cfg config.yaml --type predict

Same flags, config keys and outputs as reference main.py:16-101: ``config.yaml`` and ``log.txt`` in OUTPUT_DIR,
checkpoints every five epochs, ``predict/<name>.npz`` with ll, hmean, hcov, cont, uncertainty (and cont_samples, drawn
from the posterior, with ``--opts MODEL.N_SAMPLES <S> MODEL.SAMPLE_SEED <seed>``).  Spectra are read
on the host (qfa_amd.io), everything after that runs on the GPU; there is no CPU device.
"""
from __future__ import annotations

import argparse
import logging
import os
import time
from functools import partial


def build_parser():
    p = argparse.ArgumentParser(description="QFA training / prediction on MI355X")
    p.add_argument("--cfg", type=str)
    p.add_argument("--catalog", type=str)
    p.add_argument("--type", type=str, help="train or predict")
    p.add_argument("--data_num", type=int)
    p.add_argument("--validation_catalog", type=str)
    p.add_argument("--validation_num", type=int)
    p.add_argument("--batch_size", type=int)
    p.add_argument("--n_epochs", type=int)
    p.add_argument("--Nh", type=int)
    p.add_argument("--tau", type=str)
    p.add_argument("--learning_rate", type=float)
    p.add_argument("--gpu", type=int)
    p.add_argument("--snr_min", type=float)
    p.add_argument("--snr_max", type=float)
    p.add_argument("--z_min", type=float)
    p.add_argument("--z_max", type=float)
    p.add_argument("--num_mask", type=int)
    p.add_argument("--decay_alpha", type=float)
    p.add_argument("--decay_step", type=int)
    p.add_argument("--weight_decay", type=float)
    p.add_argument("--output_dir", type=str)
    p.add_argument("--data_dir", type=str)
    p.add_argument("--validation_dir", type=str)
    p.add_argument("--validation", type=bool)
    p.add_argument("--nprocs", type=int)
    p.add_argument("--opts", nargs="*", help="KEY VALUE pairs, e.g. MODEL.NH 16")
    return p


def load_data(cfg, device):
    """the reference Dataloader constructor (QFA/dataloader.py:58-112) on qfa_amd.io + DeviceDataloader"""
    import numpy as np
    from . import io
    from .dataloader import DeviceDataloader
    D = cfg.DATA
    wav = io.wavelength_grid(D.LAMMIN, D.LAMMAX, D.LOGLAM_DELTA)
    if cfg.TYPE == "train":
        parts = [io.load_from_catalog(D.CATALOG, D.DATA_DIR, D.DATA_NUM, D.SNR_MIN, D.SNR_MAX, D.Z_MIN, D.Z_MAX,
                                      D.NUM_MASK, D.NPROCS, D.OUTPUT_DIR, "train")]
        if D.VALIDATION and os.path.exists(D.VALIDATION_CATALOG) and os.path.exists(D.VALIDATION_DIR):
            parts.append(io.load_from_catalog(D.VALIDATION_CATALOG, D.VALIDATION_DIR, D.VALIDATION_NUM, D.SNR_MIN,
                                              D.SNR_MAX, D.Z_MIN, D.Z_MAX, D.NUM_MASK, D.NPROCS, D.OUTPUT_DIR,
                                              "validation"))
        flux, error, zqso, paths = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    elif cfg.TYPE == "predict":
        files = io.read_prediction_catalog(D.CATALOG)
        flux, error, zqso, paths = io.read_spectra([os.path.join(D.DATA_DIR, x) for x in files], D.NPROCS)
    else:
        raise NotImplementedError("TYPE should be in ['train', 'predict']!")
    return DeviceDataloader(flux, error, zqso, wav, D.BATCH_SIZE, device, tau=cfg.MODEL.TAU,
                            window_length_for_mu=cfg.TRAIN.WINDOW_LENGTH_FOR_MU, mode=cfg.TYPE, paths=paths)


def load_model_file(model, path, cfg, optimizer=None):
    """A file written by QFA.save_checkpoint (it carries adam_* keys and the true c0) goes through load_checkpoint;
    anything else through the reference's loader, with its c0 <- beta quirk unless MODEL.REFERENCE_C0_QUIRK is off.
    Returns True when the optimiser state was restored too."""
    import numpy as np
    with np.load(path) as f:
        full = "adam_i" in f.files
    if full:
        model.load_checkpoint(path, optimizer)
        return optimizer is not None
    model.load_from_npz(path, reference_c0_quirk=bool(cfg.MODEL.REFERENCE_C0_QUIRK))
    return False


def refuse(message, check, *args, **kw):
    """the command line's ValueError for what a stack's own parameter check (qfa_amd/stacks.py) refuses: the bounds are written there"""
    from ._lib import QFAHipError
    try:
        check(*args, **kw)
    except QFAHipError:
        raise ValueError(message) from None


def main(argv=None):
    from .config import get_config
    from .stacks import P1DBandStack, PDFStack, VarianceStack, XiStack, _edges
    args = build_parser().parse_args(argv)
    cfg = get_config(args)
    assert cfg.TYPE in ("train", "predict"), "TYPE must be in ['train', 'predict']!"
    if cfg.TYPE == "predict" and int(cfg.MODEL.P1D_SEGMENTS) > 0 and int(cfg.MODEL.FOREST_NBINS) <= 0:
        raise ValueError("MODEL.P1D_SEGMENTS > 0 needs MODEL.FOREST_NBINS > 0 (the mean transmission the contrast is formed with)")
    if cfg.TYPE == "predict" and int(cfg.MODEL.P1D_NBANDS) > 0 and int(cfg.MODEL.P1D_SEGMENTS) <= 0:
        raise ValueError("MODEL.P1D_NBANDS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose power is binned)")
    M = cfg.MODEL
    if cfg.TYPE == "predict" and int(M.P1D_NBANDS) != 0:
        refuse("MODEL.P1D_NBANDS must lie in 0 .. 64", _edges, range(int(M.P1D_NBANDS) + 1))
    if cfg.TYPE == "predict" and int(M.XI_NLAGS) != 0:
        if int(M.XI_NLAGS) < 0 or int(M.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.XI_NLAGS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixel pairs are summed)")
        import numpy as np
        from . import io
        wav = io.wavelength_grid(cfg.DATA.LAMMIN, cfg.DATA.LAMMAX, cfg.DATA.LOGLAM_DELTA)
        seg_len = int(np.sum(wav < 1215.67)) // int(M.P1D_SEGMENTS)                  # (the dataloader's Nb, flux_power's segments)
        refuse(f"MODEL.XI_NLAGS = {int(M.XI_NLAGS)} exceeds the segment length {seg_len}", XiStack.lag_params, seg_len, M.XI_NLAGS)
        if not float(M.XI_SIGMA2_LSS) >= 0.0 or float(M.XI_SIGMA2_LSS) == float("inf"):
            raise ValueError("MODEL.XI_SIGMA2_LSS must be finite and >= 0")
    if cfg.TYPE == "predict" and int(M.PDF_NBINS) != 0:
        refuse("MODEL.PDF_NBINS must lie in 0 .. 64", PDFStack.flux_params, 0.0, 1.0, M.PDF_NBINS)
        if int(M.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.PDF_NBINS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixels are counted)")
        refuse("MODEL.PDF_TMAX must be finite and above MODEL.PDF_TMIN", PDFStack.flux_params, M.PDF_TMIN,
               (float(M.PDF_TMAX) - float(M.PDF_TMIN)) / int(M.PDF_NBINS), M.PDF_NBINS)
        refuse("MODEL.PDF_IVAR_MIN must be finite and >= 0", PDFStack.flux_params, 0.0, 1.0, 1, ivar_min=M.PDF_IVAR_MIN)
    if cfg.TYPE == "predict" and int(M.VAR_NOCT) != 0:
        refuse("MODEL.VAR_SUB must lie in 0 .. 4", VarianceStack.var_params, 0, 1, M.VAR_SUB)
        refuse("MODEL.VAR_NOCT << MODEL.VAR_SUB must lie in 1 .. 64 (0 = off)", VarianceStack.var_params, 0, M.VAR_NOCT, M.VAR_SUB)
        if int(M.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.VAR_NOCT > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixels are binned)")
        refuse("MODEL.VAR_ELO must be >= -126 and MODEL.VAR_ELO + MODEL.VAR_NOCT <= 127", VarianceStack.var_params, M.VAR_ELO, M.VAR_NOCT,
               M.VAR_SUB)
        if not float(M.VAR_DMAX) >= 0.0 or float(M.VAR_DMAX) == float("inf"):
            raise ValueError("MODEL.VAR_DMAX must be finite and >= 0 (0 = no cut)")
        if int(M.VAR_MIN_COUNT) < 1:
            raise ValueError("MODEL.VAR_MIN_COUNT must be >= 1")
    if cfg.TYPE == "predict" and not 0 <= int(M.BOOT_N) <= 65536:
        raise ValueError("MODEL.BOOT_N must lie in 0 .. 65536 (0 = off)")
    if cfg.TYPE == "predict" and bool(M.BAL):
        from .bal import DEFAULT_LINES, check_scan_params
        refuse("MODEL.BAL_THR must be positive and finite, MODEL.BAL_SMOOTH odd in 1 .. 15, MODEL.BAL_MAX_GAP in 0 .. 16",
               check_scan_params, DEFAULT_LINES, M.BAL_THR, M.BAL_SMOOTH, M.BAL_MAX_GAP)
        if int(M.BAL_NITER) < 1 or not float(M.BAL_PAD_KMS) >= 0.0 or float(M.BAL_PAD_KMS) == float("inf"):
            raise ValueError("MODEL.BAL_NITER must be >= 1 and MODEL.BAL_PAD_KMS finite and >= 0")
    if cfg.TYPE == "predict" and bool(M.ZSCAN):
        from .redshift import MAX_SHIFT
        if not 0 <= int(M.ZSCAN_MAX_SHIFT) <= MAX_SHIFT:
            raise ValueError(f"MODEL.ZSCAN_MAX_SHIFT must lie in 0 .. {MAX_SHIFT}")
    os.makedirs(cfg.DATA.OUTPUT_DIR, exist_ok=True)
    with open(os.path.join(cfg.DATA.OUTPUT_DIR, "config.yaml"), "w") as f:
        f.write(cfg.dump())

    import torch
    from . import QFA, Adam, step_scheduler
    from .utils import tau as taufunc
    device = torch.device("cuda", int(cfg.GPU))
    torch.cuda.set_device(device)
    dataloader = load_data(cfg, device)
    model = QFA(dataloader.Nb, dataloader.Nr, cfg.MODEL.NH, device=device, tau=partial(taufunc, which=cfg.MODEL.TAU))
    model.exact_gradients = bool(cfg.MODEL.EXACT_GRADIENTS)
    if cfg.TYPE == "train":
        logger = logging.getLogger("qfa_amd")
        logger.setLevel(logging.INFO)
        handler = logging.FileHandler(os.path.join(cfg.DATA.OUTPUT_DIR, "log.txt"))
        handler.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s"))
        logger.addHandler(handler)
        scheduler = step_scheduler(cfg.TRAIN.DECAY_ALPHA, cfg.TRAIN.DECAY_STEP)
        optimizer = Adam(params=model.parameters, learning_rate=cfg.TRAIN.LEARNING_RATE, device=device,
                         scheduler=scheduler, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
        full_state = False
        if cfg.MODEL.RESUME and os.path.exists(cfg.MODEL.RESUME):
            print(f"=> Resume from {cfg.MODEL.RESUME}")
            full_state = load_model_file(model, cfg.MODEL.RESUME, cfg, optimizer)
        if not full_state:
            # as main.py:83: the reference re-randomises even after a resume (quirk Q8); a checkpoint of this
            # package that carries the Adam state (QFA.save_checkpoint) continues instead
            model.random_init_func()
        model.train(optimizer, dataloader, cfg.TRAIN.NEPOCHS, cfg.DATA.OUTPUT_DIR, logger=logger,
                    f_update=str(cfg.TRAIN.F_UPDATE), em_rho=float(cfg.TRAIN.EM_RHO), em_ridge=float(cfg.TRAIN.EM_RIDGE))
    else:
        print(f"try to predict {len(dataloader)} spectra...")
        print(f"=> Resume from {cfg.MODEL.RESUME}")
        load_model_file(model, cfg.MODEL.RESUME, cfg)         # parameters and mu of the trained model
        ts = time.time()
        model.predict_to_npz(dataloader, os.path.join(cfg.DATA.OUTPUT_DIR, "predict"),
                             n_samples=int(cfg.MODEL.N_SAMPLES), seed=int(cfg.MODEL.SAMPLE_SEED),
                             n_replicates=int(cfg.MODEL.N_REPLICATES), forest=bool(cfg.MODEL.FOREST))
        if int(M.FOREST_NBINS) > 0:
            import numpy as np
            save = lambda name, stack, **kw: np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, name), **stack.arrays(**kw))
            draws = dict(n_samples=int(M.N_SAMPLES), seed=int(M.SAMPLE_SEED))
            st = model.mean_transmission(dataloader, float(M.FOREST_ZMIN), float(M.FOREST_ZMAX), int(M.FOREST_NBINS), **draws)
            save("mean_transmission.npz", st)
        if int(M.P1D_SEGMENTS) > 0:
            # the contrast is formed with the very stack mean_transmission.npz holds: pixels outside [FOREST_ZMIN, FOREST_ZMAX) are
            # unused, and a segment that loses too many of them to the edges is left out (P1D_MIN_USED_FRAC)
            shared = dict(n_segments=int(M.P1D_SEGMENTS), min_used_frac=float(M.P1D_MIN_USED_FRAC), tbar=st, **draws)
            done = []                                           # (flux_power's stack first: the bands lie on its segments and dv)
            # (config switch, loader method, its name in QFA.bootstrap, its own keywords, arrays()'s keywords, file): one row per statistic
            for switch, method, boot, own, export, name in (
                    (M.P1D_SEGMENTS, model.flux_power, "p1d", dict, {}, "flux_power.npz"),
                    (M.P1D_NBANDS, model.band_power, "bands",
                     lambda: dict(k_edges=P1DBandStack.linear_k_edges(done[0].L, done[0].dv, int(M.P1D_NBANDS))), {}, "flux_power_bands.npz"),
                    (M.XI_NLAGS, model.flux_correlation, "xi", lambda: dict(n_lags=int(M.XI_NLAGS), sigma2_lss=float(M.XI_SIGMA2_LSS)), {},
                     "flux_correlation.npz"),
                    (M.PDF_NBINS, model.flux_pdf, "pdf",
                     lambda: dict(n_tbins=int(M.PDF_NBINS), t_min=float(M.PDF_TMIN), t_max=float(M.PDF_TMAX), relative=bool(M.PDF_RELATIVE),
                                  clamp=bool(M.PDF_CLAMP), ivar_min=float(M.PDF_IVAR_MIN)), {}, "flux_pdf.npz"),
                    (M.VAR_NOCT, model.variance_function, "variance",
                     lambda: dict(e_lo=int(M.VAR_ELO), n_oct=int(M.VAR_NOCT), sub=int(M.VAR_SUB),
                                  d_max=float(M.VAR_DMAX) if float(M.VAR_DMAX) > 0.0 else None),
                     dict(min_count=int(M.VAR_MIN_COUNT)), "variance_function.npz")):
                if int(switch) > 0 and int(M.BOOT_N) > 0:
                    stack, bt = model.bootstrap(dataloader, boot, float(M.FOREST_ZMIN), float(M.FOREST_ZMAX), int(M.P1D_NZBINS),
                                                int(M.BOOT_N), boot_seed=int(M.BOOT_SEED), **own(), **shared)
                    done.append(stack)
                    save(name, stack, **export)
                    save(name[:-4] + "_bootstrap.npz", bt)
                elif int(switch) > 0:
                    done.append(method(dataloader, float(M.FOREST_ZMIN), float(M.FOREST_ZMAX), int(M.P1D_NZBINS), **own(), **shared))
                    save(name, done[-1], **export)
        if bool(M.BAL):
            import numpy as np
            from . import io
            scan = model.bal_catalog(dataloader, thr=float(M.BAL_THR), smooth=int(M.BAL_SMOOTH), max_gap=int(M.BAL_MAX_GAP),
                                     n_samples=int(M.N_SAMPLES), seed=int(M.SAMPLE_SEED), n_iter=int(M.BAL_NITER),
                                     pad_kms=float(M.BAL_PAD_KMS))
            io.write_bal_csv(os.path.join(cfg.DATA.OUTPUT_DIR, "bal_catalog.csv"),
                             scan.to_table([os.path.basename(n) for n in scan.names], min_value=float(M.BAL_MIN_AI)))
            np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "bal_scan.npz"), **scan.arrays())
        if bool(M.ZSCAN):
            import numpy as np
            from . import io
            scan = model.redshift_catalog(dataloader, int(M.ZSCAN_MAX_SHIFT))
            io.write_redshift_csv(os.path.join(cfg.DATA.OUTPUT_DIR, "redshift_catalog.csv"),
                                  scan.to_table([os.path.basename(n) for n in scan.names]))
            np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "redshift_scan.npz"), **scan.arrays())
        print(f"Finish predicting {len(dataloader)} spectra in {time.time() - ts} seconds...")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
