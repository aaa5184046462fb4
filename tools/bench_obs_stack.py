"""Timing of the observed-frame residual stack (QFA.observed_residuals; include/qfa_hip.h qfa_obs_stack_f32) -- not the flagship
benchmark: that is bench.py.  B = 4096 spectra drawn from the model at the SDSS shape (N_pix 1913, N_h 8, 4 607 bins of 1e-4 dex)
and at N_pix 4000 / N_h 16 with 7 781 linear bins of 0.8 A, S = 1 and S = 100 draws, the red side and the whole spectrum
separately.  The fused call is timed between device events, medians after warm-up, against
  * the byte floor: flux and error of the stacked pixels read once, 8 B (p_hi - p_lo) bytes, at the copy bandwidth DESIGN.md
    quotes (4 TB/s), and
  * the eager torch composition in the same run: continua materialised, division, float64 index_add_ (on `--eager_draws` draws,
    scaled to S: it is linear in S).
One JSON line per (shape, S, range), appended to profiles/obs_stack_bench.jsonl.

    python tools/bench_obs_stack.py [--steps 5] [--warmup 2] [--eager_draws 4]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_TBS = 4.0
SHAPES = (("sdss", None, 8, dict(lam_min=3600.0, nbin=4607, dloglam=1e-4)),
          ("px4000_nh16", 4000, 16, dict(lam_min=3600.0, nbin=7781, dlam=0.8)))


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


def eager_stack(m, flux, error, mask, h, k, nbin, p_lo):
    """the rule composed from torch operations: (S, 4, nbin) float64; k (B, Npix - p_lo) int64 bins, -1 = not stacked"""
    import torch
    c = m.mu[None, None, p_lo:] + torch.einsum("pj,bsj->bsp", m.F[p_lo:], h)
    r = flux[:, None, p_lo:] / c
    iv = c * c / (error[:, None, p_lo:] ** 2)
    use = mask[:, None, p_lo:] & (c > 0) & torch.isfinite(r) & torch.isfinite(iv) & (k >= 0)[:, None, :]
    w = torch.where(use, iv, torch.zeros_like(iv)).double()
    rd = torch.where(use, r, torch.zeros_like(r)).double()
    S = h.shape[1]
    idx = (torch.arange(S, device=flux.device)[None, :, None] * nbin + k.clamp(min=0)[:, None, :]).reshape(-1)
    out = torch.zeros((4, S * nbin), dtype=torch.float64, device=flux.device)
    for q, t in enumerate((w, w * rd, w * rd * rd, use.double())):
        out[q].index_add_(0, idx, t.reshape(-1))
    return out.reshape(4, S, nbin).permute(1, 0, 2).contiguous()


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA, synthetic
    from qfa_amd.calibration import coordinates, obs_grid
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eager_draws", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    log = open(os.path.join(REPO, "profiles", "obs_stack_bench.jsonl"), "a")
    for name, npix, nh, grid in SHAPES:
        wav, nb, nr = synthetic.wavelength_grid(npix)
        npix = len(wav)
        params, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
        flux, error, zq = synthetic.make_batch_torch(params, mu, wav, nb, a.batch, 20220701, dev, return_flux=True)
        mask = (flux != -999.0) & (error != -999.0)
        m = QFA(nb, nr, nh, dev, model_params=params)
        m.mu = torch.tensor(mu, device=dev)
        zq_h = zq.double().cpu().numpy()
        u0, du, nbin, mode = obs_grid(**grid)
        pix_u, spec_u = coordinates(wav, zq_h, mode)
        x = ((pix_u[None, :] * spec_u[:, None] if mode == "linear" else pix_u[None, :] + spec_u[:, None]) - u0) * (1.0 / du)
        kall = torch.tensor(np.where((x >= 0) & (x < nbin), np.floor(x), -1).astype(np.int64), device=dev)
        for S in (1, 100):
            h = torch.randn((a.batch, S, nh), device=dev)
            for rname, rest, p_lo in (("red", (synthetic.LYA, np.inf), nb), ("all", None, 0)):
                fn = lambda: m.observed_residuals(flux, error, mask, h=h, zqso=zq_h, wav_grid=wav, rest_range=rest, **grid)
                for _ in range(a.warmup):
                    st = fn()
                torch.cuda.synchronize()
                ms = float(np.median(timed(fn, a.steps)))
                se = min(S, a.eager_draws)
                efn = lambda: eager_stack(m, flux, error, mask, h[:, :se].contiguous(), kall[:, p_lo:], nbin, p_lo)
                ref = efn()
                for _ in range(a.warmup):
                    efn()
                torch.cuda.synchronize()
                ems = float(np.median(timed(efn, a.steps))) * S / se
                floor_ms = 8.0 * a.batch * (npix - p_lo) / (COPY_TBS * 1e12) * 1e3
                got = st.buf[:se]
                line = {"shape": name, "B": a.batch, "Npix": npix, "Nh": nh, "S": S, "nbin": nbin, "mode": mode, "range": rname,
                        "p_lo": p_lo, "ms_stack": round(ms, 4), "ms_byte_floor": round(floor_ms, 5), "copy_TBs": COPY_TBS,
                        "x_floor": round(ms / floor_ms, 1), "ms_eager_scaled": round(ems, 3), "eager_draws": se,
                        "x_eager": round(ems / ms, 2), "n_equal_eager": bool(torch.equal(got[:, 3], ref[:, 3])),
                        "max_rel_sum_w_minus_eager": float(((got[:, 0] - ref[:, 0]).abs() / ref[:, 0].abs().clamp(min=1e-300)).max()),
                        "steps": a.steps, "warmup": a.warmup}
                print(json.dumps(line), flush=True)
                log.write(json.dumps(line) + "\n")
                log.flush()
            del h
        del flux, error, mask, m, kall
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
