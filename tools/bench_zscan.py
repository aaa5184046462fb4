"""Timing of the redshift finder's scan (QFA.redshift_scan; include/qfa_hip.h qfa_redshift_scan_f32) -- not the flagship benchmark:
that is bench.py.  Two shapes, B = 4096 spectra drawn from the model, max_shift = 20 (41 candidates): the SDSS shape (N_pix 1913,
N_h 8) and N_pix 4000 / N_h 16.  The call is timed between device events, medians after warm-up, against
  * the MFMA flop floor 2 B n_s N_pix (N_h (N_h + 1) / 2 + N_h) at the dense float32 matrix rate (157.3 Tflop/s), and
  * the eager composition on the same GPU in the same run: 2 m + 1 shifted batches materialised with torch indexing (data, mask
    and z moved onto the model pixels q = p + s, the window applied through the mask) and sent through ``predict``, whose ll is
    NLL_s.  It runs on `--eager_spectra` spectra and is scaled to B (it is linear in B).  The first eager spectra are rolled by known
    shifts, and the scan must give the eager composition's arg-max on every one of them (the tool fails otherwise).
One JSON line per shape, appended to profiles/zscan_bench.jsonl.

    python tools/bench_zscan.py [--steps 5] [--warmup 2] [--eager_spectra 256]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MFMA_F32_RATE = 157.3e12
SHAPES = (("sdss", None, 8), ("px4000_nh16", 4000, 16))
MAX_SHIFT = 20
ROLLS = (-7, -3, 0, 2, 5, 11)


def timed(fn, n):
    import torch
    out = []
    for _ in range(n):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        fn()
        s1.record()
        s1.synchronize()
        out.append(s0.elapsed_time(s1))
    return out


def eager_scan(m, flux, error, mask, zq1, ratio, ms):
    """NLL_s (b, 2 ms + 1) through predict on shifted batches"""
    import torch
    n, nb = flux.shape[1], m.Nb
    p = torch.arange(n, device=flux.device)
    out = []
    for s in range(-ms, ms + 1):
        src = p - s                                               # model pixel q holds data pixel q - s
        ok = (src >= ms) & (src < n - ms)
        idx = src.clamp(0, n - 1)
        f, e, k = flux[:, idx], error[:, idx], mask[:, idx] & ok[None, :]
        z = (zq1[:, None] * ratio[idx[:nb]][None, :] - 1.0).contiguous()
        out.append(m.predict(f.contiguous(), e.contiguous(), z, k.contiguous())[0].reshape(-1))
    return torch.stack(out, dim=1)


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eager_spectra", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    log = open(os.path.join(REPO, "profiles", "zscan_bench.jsonl"), "a")
    ms_ = MAX_SHIFT
    for name, npix, nh in SHAPES:
        wav, nb, nr = synthetic.wavelength_grid(npix)
        npix = len(wav)
        params, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
        flux, error, zq = synthetic.make_batch_torch(params, mu, wav, nb, a.batch, 20220701, dev, return_flux=True)
        for r, t in enumerate(ROLLS):                              # data pixel p holds what was drawn at p + t
            flux[r], error[r] = torch.roll(flux[r], -t), torch.roll(error[r], -t)
        mask = (flux != -999.0) & (error != -999.0)
        m = QFA(nb, nr, nh, dev, model_params=params)
        m.mu = torch.tensor(mu, device=dev)
        zqso = zq.double().cpu().numpy()
        fn = lambda: m.redshift_scan(flux, error, mask, zqso=zqso, wav_grid=wav, max_shift=ms_)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t_scan = float(np.median(timed(fn, a.steps)))
        be = min(a.eager_spectra, a.batch)
        ratio = torch.tensor((wav / synthetic.LYA).astype(np.float32), device=dev)
        zq1 = torch.tensor((1.0 + zqso[:be]).astype(np.float32), device=dev)
        efn = lambda: eager_scan(m, flux[:be], error[:be], mask[:be], zq1, ratio, ms_)
        ref = efn()
        got = m.redshift_scan(flux[:be], error[:be], mask[:be], zqso=zqso[:be], wav_grid=wav, max_shift=ms_)
        ref_best = torch.argmin(ref, dim=1) - ms_
        same = bool(torch.equal(ref_best.to(torch.int32), got.best_s))
        rolls_found = got.best_s[:len(ROLLS)].cpu().tolist()
        for _ in range(a.warmup):
            efn()
        torch.cuda.synchronize()
        t_eager = float(np.median(timed(efn, a.steps))) * a.batch / be
        ns = 2 * ms_ + 1
        flops = 2.0 * a.batch * ns * npix * (nh * (nh + 1) / 2 + nh)
        floor = flops / MFMA_F32_RATE * 1e3
        line = {"shape": name, "B": a.batch, "Npix": npix, "Nh": nh, "max_shift": ms_, "n_s": ns, "ms_scan": round(t_scan, 3),
                "ms_mfma_flop_floor": round(floor, 3), "x_floor": round(t_scan / floor, 2), "ms_eager_scaled": round(t_eager, 1),
                "eager_spectra": be, "x_eager": round(t_eager / t_scan, 1), "same_argmax_as_eager": same, "rolls": list(ROLLS),
                "rolls_found": rolls_found, "max_abs_llr_minus_eager": float((got.llr - (ref[:, ms_:ms_ + 1] - ref)).abs().max()),
                "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(line), flush=True)
        log.write(json.dumps(line) + "\n")
        log.flush()
        if not same:
            raise SystemExit("the scan's arg-max differs from the eager composition's")
        del flux, error, mask, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
