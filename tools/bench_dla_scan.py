"""Timing of the DLA finder's scan (QFA.template_scan; include/qfa_hip.h qfa_template_scan_f32) -- not the flagship benchmark: that
is bench.py.  Two shapes, B = 4096 spectra drawn from the model, 256 redshift nodes x 12 column densities: the SDSS shape
(N_pix 1913, N_h 8) and N_pix 4000 / N_h 16.  The call is timed between device events, medians after warm-up, against
  * the MFMA flop floor 2 B n_c N_pix (N_h (N_h + 1) / 2 + N_h + 1) at the dense float32 matrix rate (157.3 Tflop/s), and
  * the eager torch composition of the same rule on the same GPU in the same run.  Eager materialises (b, n_c, N_pix) weights, so
    it runs on `--eager_spectra` spectra in candidate chunks and is scaled to B (it is linear in B).
One JSON line per shape, appended to profiles/dla_scan_bench.jsonl.

    python tools/bench_dla_scan.py [--steps 5] [--warmup 2] [--eager_spectra 4]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MFMA_F32_RATE = 157.3e12
SHAPES = (("sdss", None, 8), ("px4000_nh16", 4000, 16))
GRID = dict(lam_hi=1200.0, dv_kms=150.0, nz=256, logn_lo=20.0, dlogn=0.2, n_logn=12)


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


def eager_scan(m, flux, error, zabs, mask, V, chunk=128):
    """the rule of include/qfa_hip.h composed from torch operations in float32 (Cholesky in float64): llr (b, nc)"""
    import torch
    nb, F, mu = m.Nb, m.F, m.mu
    z = zabs
    t = m._tau_model
    A = torch.ones_like(flux)
    A[:, :nb] = torch.exp(-(t.amp * ((1.0 + z) * t.scale) ** t.expo + t.offset))
    G = A * A * m.Psi[None, :]
    G[:, :nb] += m.omega[None, :] * (1.0 - m.c0 - torch.exp(-m.tau0 * (1.0 + z) ** m.beta)) ** 2
    w = mask.to(flux.dtype)
    x = torch.where(mask, flux, torch.zeros_like(flux))
    s2 = torch.where(mask, error * error, torch.ones_like(error))
    eye = torch.eye(F.shape[1], dtype=torch.float64, device=flux.device)

    def nll(Vc):                                                # Vc (c, Npix) -> (b, c)
        Ap = Vc[None] * A[:, None]
        Dp = Vc[None] ** 2 * G[:, None] + s2[:, None]
        wp = w[:, None] / Dp
        dp = x[:, None] - Ap * mu[None, None]
        C = torch.einsum("bck,ka,kd->bcad", wp * Ap * Ap, F, F).double() + eye
        bv = torch.einsum("bck,ka->bca", wp * Ap * dp, F).double()
        L = torch.linalg.cholesky(C)
        y = torch.linalg.solve_triangular(L, bv[..., None], upper=False)[..., 0]
        return 0.5 * ((wp * dp * dp).sum(-1).double() - (y * y).sum(-1) + (w[:, None] * torch.log(Dp)).sum(-1).double()
                      + 2.0 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1))
    n0 = nll(torch.ones_like(V[:1]))
    return torch.cat([n0 - nll(V[c0:c0 + chunk]) for c0 in range(0, V.shape[0], chunk)], dim=1).float()


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eager_spectra", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    log = open(os.path.join(REPO, "profiles", "dla_scan_bench.jsonl"), "a")
    for name, npix, nh in SHAPES:
        wav, nb, nr = synthetic.wavelength_grid(npix)
        npix = len(wav)
        params, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
        flux, error, zq = synthetic.make_batch_torch(params, mu, wav, nb, a.batch, 20220701, dev, return_flux=True)
        mask = (flux != -999.0) & (error != -999.0)
        zfac = ((1.0 + zq).contiguous(), torch.tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev))
        m = QFA(nb, nr, nh, dev, model_params=params)
        m.mu = torch.tensor(mu, device=dev)
        V = m.dla_profiles(wav, **GRID)
        nc = int(V.shape[0])
        fn = lambda: m.template_scan(flux, error, None, mask, V, zfac=zfac)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = float(np.median(timed(fn, a.steps)))
        be = a.eager_spectra
        zabs = (zfac[0][:be, None] * zfac[1][None, :] - 1.0).contiguous()
        efn = lambda: eager_scan(m, flux[:be], error[:be], zabs, mask[:be], V)
        ref = efn()
        got = m.template_scan(flux[:be], error[:be], zabs, mask[:be], V)[0]
        for _ in range(a.warmup):
            efn()
        torch.cuda.synchronize()
        ems = float(np.median(timed(efn, a.steps))) * a.batch / be
        flops = 2.0 * a.batch * nc * npix * (nh * (nh + 1) / 2 + nh + 1)
        line = {"shape": name, "B": a.batch, "Npix": npix, "Nh": nh, "nc": nc, "ms_scan": round(ms, 3),
                "ms_mfma_flop_floor": round(flops / MFMA_F32_RATE * 1e3, 3), "x_floor": round(ms / (flops / MFMA_F32_RATE * 1e3), 2),
                "ms_eager_scaled": round(ems, 1), "eager_spectra": be, "x_eager": round(ems / ms, 1),
                "max_abs_llr_minus_eager": float((got - ref).abs().max()), "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(line), flush=True)
        log.write(json.dumps(line) + "\n")
        log.flush()
        del flux, error, mask, V, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
