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


def main(argv=None):
    from .config import get_config
    args = build_parser().parse_args(argv)
    cfg = get_config(args)
    assert cfg.TYPE in ("train", "predict"), "TYPE must be in ['train', 'predict']!"
    if cfg.TYPE == "predict" and int(cfg.MODEL.P1D_SEGMENTS) > 0 and int(cfg.MODEL.FOREST_NBINS) <= 0:
        raise ValueError("MODEL.P1D_SEGMENTS > 0 needs MODEL.FOREST_NBINS > 0 (the mean transmission the contrast is formed with)")
    if cfg.TYPE == "predict" and int(cfg.MODEL.P1D_NBANDS) > 0 and int(cfg.MODEL.P1D_SEGMENTS) <= 0:
        raise ValueError("MODEL.P1D_NBANDS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose power is binned)")
    if cfg.TYPE == "predict" and not 0 <= int(cfg.MODEL.P1D_NBANDS) <= 64:
        raise ValueError("MODEL.P1D_NBANDS must lie in 0 .. 64")
    if cfg.TYPE == "predict" and int(cfg.MODEL.XI_NLAGS) != 0:
        if int(cfg.MODEL.XI_NLAGS) < 0 or int(cfg.MODEL.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.XI_NLAGS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixel pairs are summed)")
        import numpy as np
        from . import io
        wav = io.wavelength_grid(cfg.DATA.LAMMIN, cfg.DATA.LAMMAX, cfg.DATA.LOGLAM_DELTA)
        seg_len = int(np.sum(wav < 1215.67)) // int(cfg.MODEL.P1D_SEGMENTS)          # (the dataloader's Nb, flux_power's segments)
        if int(cfg.MODEL.XI_NLAGS) > seg_len:
            raise ValueError(f"MODEL.XI_NLAGS = {int(cfg.MODEL.XI_NLAGS)} exceeds the segment length {seg_len}")
        if not float(cfg.MODEL.XI_SIGMA2_LSS) >= 0.0 or float(cfg.MODEL.XI_SIGMA2_LSS) == float("inf"):
            raise ValueError("MODEL.XI_SIGMA2_LSS must be finite and >= 0")
    if cfg.TYPE == "predict" and int(cfg.MODEL.PDF_NBINS) != 0:
        if not 1 <= int(cfg.MODEL.PDF_NBINS) <= 64:
            raise ValueError("MODEL.PDF_NBINS must lie in 0 .. 64")
        if int(cfg.MODEL.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.PDF_NBINS > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixels are counted)")
        if not float(cfg.MODEL.PDF_TMAX) > float(cfg.MODEL.PDF_TMIN) or abs(float(cfg.MODEL.PDF_TMAX)) == float("inf") or \
                abs(float(cfg.MODEL.PDF_TMIN)) == float("inf"):
            raise ValueError("MODEL.PDF_TMAX must be finite and above MODEL.PDF_TMIN")
        if not float(cfg.MODEL.PDF_IVAR_MIN) >= 0.0 or float(cfg.MODEL.PDF_IVAR_MIN) == float("inf"):
            raise ValueError("MODEL.PDF_IVAR_MIN must be finite and >= 0")
    if cfg.TYPE == "predict" and int(cfg.MODEL.VAR_NOCT) != 0:
        noct, elo, sub = int(cfg.MODEL.VAR_NOCT), int(cfg.MODEL.VAR_ELO), int(cfg.MODEL.VAR_SUB)
        if not 0 <= sub <= 4:
            raise ValueError("MODEL.VAR_SUB must lie in 0 .. 4")
        if not 1 <= noct << sub <= 64:
            raise ValueError("MODEL.VAR_NOCT << MODEL.VAR_SUB must lie in 1 .. 64 (0 = off)")
        if int(cfg.MODEL.P1D_SEGMENTS) <= 0:
            raise ValueError("MODEL.VAR_NOCT > 0 needs MODEL.P1D_SEGMENTS > 0 (the segments whose pixels are binned)")
        if elo < -126 or elo + noct > 127:
            raise ValueError("MODEL.VAR_ELO must be >= -126 and MODEL.VAR_ELO + MODEL.VAR_NOCT <= 127")
        if not float(cfg.MODEL.VAR_DMAX) >= 0.0 or float(cfg.MODEL.VAR_DMAX) == float("inf"):
            raise ValueError("MODEL.VAR_DMAX must be finite and >= 0 (0 = no cut)")
        if int(cfg.MODEL.VAR_MIN_COUNT) < 1:
            raise ValueError("MODEL.VAR_MIN_COUNT must be >= 1")
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
        if int(cfg.MODEL.FOREST_NBINS) > 0:
            import numpy as np
            st = model.mean_transmission(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX),
                                         int(cfg.MODEL.FOREST_NBINS), n_samples=int(cfg.MODEL.N_SAMPLES),
                                         seed=int(cfg.MODEL.SAMPLE_SEED))
            np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "mean_transmission.npz"), z_centers=st.z_centers.cpu().numpy(),
                     z_edges=st.z_edges.cpu().numpy(), mean=st.mean.cpu().numpy(), var=st.var.cpu().numpy(), n=st.n.cpu().numpy(),
                     tau_eff=st.tau_eff.cpu().numpy(), sums=st.buf.cpu().numpy())
        if int(cfg.MODEL.P1D_SEGMENTS) > 0:
            # the contrast is formed with the very stack mean_transmission.npz holds: pixels outside [FOREST_ZMIN, FOREST_ZMAX) are
            # unused, and a segment that loses too many of them to the edges is left out (P1D_MIN_USED_FRAC)
            ps = model.flux_power(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX), int(cfg.MODEL.P1D_NZBINS),
                                  n_segments=int(cfg.MODEL.P1D_SEGMENTS), min_used_frac=float(cfg.MODEL.P1D_MIN_USED_FRAC),
                                  tbar=st, n_samples=int(cfg.MODEL.N_SAMPLES), seed=int(cfg.MODEL.SAMPLE_SEED))
            np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "flux_power.npz"), k=ps.k.cpu().numpy(), z_centers=ps.z_centers.cpu().numpy(),
                     z_edges=ps.z_edges.cpu().numpy(), power=ps.power().cpu().numpy(), err=ps.err().cpu().numpy(),
                     power_raw=ps.power_raw.cpu().numpy(), noise=ps.noise.cpu().numpy(), n=ps.n.cpu().numpy(),
                     seg_len=ps.L, dv=ps.dv, sums=ps.buf.cpu().numpy())
            if int(cfg.MODEL.P1D_NBANDS) > 0:
                from .model import P1DBandStack
                bs = model.band_power(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX), int(cfg.MODEL.P1D_NZBINS),
                                      P1DBandStack.linear_k_edges(ps.L, ps.dv, int(cfg.MODEL.P1D_NBANDS)),
                                      n_segments=int(cfg.MODEL.P1D_SEGMENTS), min_used_frac=float(cfg.MODEL.P1D_MIN_USED_FRAC),
                                      tbar=st, n_samples=int(cfg.MODEL.N_SAMPLES), seed=int(cfg.MODEL.SAMPLE_SEED))
                out = dict(k_edges=bs.k_edges.cpu().numpy(), k_centers=bs.k_centers.cpu().numpy(), z_edges=bs.z_edges.cpu().numpy(),
                           n=bs.n.cpu().numpy(), mean=bs.mean.cpu().numpy(), cov=bs.cov.cpu().numpy())
                if bs.S > 1:
                    out["cov_over_draws"] = bs.cov_over_draws.cpu().numpy()
                np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "flux_power_bands.npz"), **out)
            if int(cfg.MODEL.XI_NLAGS) > 0:
                xs = model.flux_correlation(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX),
                                            int(cfg.MODEL.P1D_NZBINS), int(cfg.MODEL.XI_NLAGS), n_segments=int(cfg.MODEL.P1D_SEGMENTS),
                                            min_used_frac=float(cfg.MODEL.P1D_MIN_USED_FRAC), tbar=st, n_samples=int(cfg.MODEL.N_SAMPLES),
                                            seed=int(cfg.MODEL.SAMPLE_SEED), sigma2_lss=float(cfg.MODEL.XI_SIGMA2_LSS))
                np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "flux_correlation.npz"), lags_kms=xs.lags_kms.cpu().numpy(),
                         z_centers=xs.z_centers.cpu().numpy(), z_edges=xs.z_edges.cpu().numpy(), xi=xs.xi().cpu().numpy(),
                         xi_raw=xs.xi(subtract_noise=False).cpu().numpy(), err=xs.err().cpu().numpy(), n=xs.n.cpu().numpy(),
                         sum_w=xs.sum_w.cpu().numpy(), seg_len=xs.L, dv=xs.dv, sums=xs.buf.cpu().numpy())
            if int(cfg.MODEL.PDF_NBINS) > 0:
                fs = model.flux_pdf(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX), int(cfg.MODEL.P1D_NZBINS),
                                    int(cfg.MODEL.PDF_NBINS), t_min=float(cfg.MODEL.PDF_TMIN), t_max=float(cfg.MODEL.PDF_TMAX),
                                    relative=bool(cfg.MODEL.PDF_RELATIVE), clamp=bool(cfg.MODEL.PDF_CLAMP),
                                    ivar_min=float(cfg.MODEL.PDF_IVAR_MIN), n_segments=int(cfg.MODEL.P1D_SEGMENTS),
                                    min_used_frac=float(cfg.MODEL.P1D_MIN_USED_FRAC), tbar=st, n_samples=int(cfg.MODEL.N_SAMPLES),
                                    seed=int(cfg.MODEL.SAMPLE_SEED))
                out = dict(z=fs.z_centers.cpu().numpy(), t_edges=fs.t_edges.cpu().numpy(), pdf=fs.pdf().cpu().numpy(),
                           err=fs.err().cpu().numpy(), cov=fs.cov().cpu().numpy(), counts=fs.counts.cpu().numpy(),
                           n_segments=fs.n_segments.cpu().numpy(), out_of_range=fs.out_of_range().cpu().numpy())
                if fs.S > 1:
                    out["std_over_draws"] = fs.std_over_draws.cpu().numpy()
                    out["total_cov"] = fs.total_cov.cpu().numpy()
                np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "flux_pdf.npz"), **out)
            if int(cfg.MODEL.VAR_NOCT) > 0:
                vs = model.variance_function(dataloader, float(cfg.MODEL.FOREST_ZMIN), float(cfg.MODEL.FOREST_ZMAX), int(cfg.MODEL.P1D_NZBINS),
                                             e_lo=int(cfg.MODEL.VAR_ELO), n_oct=int(cfg.MODEL.VAR_NOCT), sub=int(cfg.MODEL.VAR_SUB),
                                             d_max=float(cfg.MODEL.VAR_DMAX) if float(cfg.MODEL.VAR_DMAX) > 0.0 else None,
                                             n_segments=int(cfg.MODEL.P1D_SEGMENTS), min_used_frac=float(cfg.MODEL.P1D_MIN_USED_FRAC),
                                             tbar=st, n_samples=int(cfg.MODEL.N_SAMPLES), seed=int(cfg.MODEL.SAMPLE_SEED))
                ft = vs.fit(min_count=int(cfg.MODEL.VAR_MIN_COUNT))
                out = dict(z=vs.z_centers.cpu().numpy(), z_edges=vs.z_edges.cpu().numpy(), v_edges=vs.v_edges.cpu().numpy(),
                           v_mean=vs.v_mean.cpu().numpy(), var_delta=vs.var_delta.cpu().numpy(), var_err=vs.var_err.cpu().numpy(),
                           mean_delta=vs.mean_delta.cpu().numpy(), counts=vs.counts.cpu().numpy(),
                           n_segments=vs.n_segments.cpu().numpy(), n_pixels=vs.n_pixels.cpu().numpy(),
                           out_of_range=vs.out_of_range().cpu().numpy(), seg_len=vs.L, sums=vs.buf.cpu().numpy(),
                           eta=ft.eta.cpu().numpy(), sigma2_lss=ft.sigma2_lss.cpu().numpy(), cov=ft.cov.cpu().numpy(),
                           chi2=ft.chi2.cpu().numpy(), ndof=ft.ndof.cpu().numpy(), n_bins=ft.n_bins.cpu().numpy())
                if vs.S > 1:
                    out["eta_std_over_draws"], out["sigma2_lss_std_over_draws"] = (
                        t.cpu().numpy() for t in vs.std_over_draws(min_count=int(cfg.MODEL.VAR_MIN_COUNT)))
                np.savez(os.path.join(cfg.DATA.OUTPUT_DIR, "variance_function.npz"), **out)
        print(f"Finish predicting {len(dataloader)} spectra in {time.time() - ts} seconds...")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
