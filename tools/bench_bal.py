"""Timing of the BAL finder (QFA.bal_scan; include/qfa_hip.h qfa_bal_scan_f32) -- not the flagship benchmark: that is bench.py.
B = 4096 spectra drawn from the model at the SDSS shape (N_pix 1913, N_h 8) and at N_pix 4000 / N_h 16, the C IV and Si IV windows
with the default BI and AI, S = 1 and S = 100 draws.  Two times between device events, medians after warm-up: `ms_scan`, the Python
call QFA.bal_scan as a user makes it (window tables formed and uploaded, outputs allocated, one launch), and `ms_call`, the C entry
point alone on prepared arguments (outputs from torch's caching allocator, one launch) -- the nearer of the two to a kernel time;
no kernel trace is taken.  They stand against
  * the byte floor: flux, error and mask of the two windows read once per spectrum, h read and the 248 output bytes per (spectrum,
    draw, line) written once, at the copy bandwidth DESIGN.md quotes (4 TB/s), and
  * the eager torch composition in the same run: continua materialised, torch division, run lengths in torch (cumulative sums over
    the window; on `--eager_draws` draws, scaled to S: it is linear in S).
One JSON line per (shape, S), appended to profiles/bal_bench.jsonl.

    python tools/bench_bal.py [--steps 20] [--warmup 2] [--eager_draws 4]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_TBS = 4.0
SHAPES = (("sdss", None, 8), ("px4000_nh16", 4000, 16))
OUT_BYTES = 4 * (8 + 8 + 12) // 2 + 8 + 128                   # two indices: value, var, three counts; two line counts; the trough list


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


def eager_index(m, flux, error, mask, h, p_lo, p_hi, vedge, index, thr):
    """one index of one line composed from torch operations (smooth 1, max_gap 0): (B, S) float64 values"""
    import torch
    v_lo, v_hi, w_min, mode = index
    sl = slice(p_lo, p_hi)
    c = m.mu[None, None, sl] + torch.einsum("pj,bsj->bsp", m.F[sl], h)
    r = (flux[:, None, sl] / c).flip(-1)
    iv = (c * c / (error[:, None, sl] ** 2)).flip(-1)
    use = mask[:, None, sl].flip(-1) & (c.flip(-1) > 0) & torch.isfinite(r) & torch.isfinite(iv)
    lo, hi = torch.clamp(vedge[:-1], min=v_lo), torch.clamp(vedge[1:], max=v_hi)
    dom = (hi - lo) > 0
    member = use & (r.double() < thr) & dom
    # run ends by cumulative maxima / minima of the positions of the non-members
    n = member.shape[-1]
    pos = torch.arange(n, device=flux.device)
    first = torch.cummax(torch.where(member, torch.full_like(pos, -1), pos).expand_as(member), -1).values + 1
    rev = torch.where(member, torch.full_like(pos, -1), n - 1 - pos).expand_as(member)       # n - 1 - j at the non-members
    last = n - 2 - torch.cummax(rev.flip(-1), -1).values.flip(-1)                             # (first non-member >= i) - 1
    e0 = torch.clamp(vedge[first.clamp(max=n - 1)], min=v_lo)
    e1 = torch.clamp(vedge[(last + 1).clamp(max=n)], max=v_hi)
    if mode == "whole":
        w = torch.where(member & (e1 - e0 >= w_min), hi - lo, torch.zeros_like(e0))
    else:
        w = torch.where(member, torch.clamp(hi - torch.maximum(vedge[:-1].expand_as(e0), e0 + w_min), min=0.0), torch.zeros_like(e0))
    return ((1.0 - r.double() / thr) * w).sum(-1)


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA, synthetic
    from qfa_amd.bal import DEFAULT_INDICES, DEFAULT_LINES, check_indices, velocity_window
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--eager_draws", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    log = open(os.path.join(REPO, "profiles", "bal_bench.jsonl"), "a")
    for name, npix, nh in SHAPES:
        wav, nb, nr = synthetic.wavelength_grid(npix)
        npix = len(wav)
        params, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
        flux, error, zq = synthetic.make_batch_torch(params, mu, wav, nb, a.batch, 20220701, dev, return_flux=True)
        mask = (flux != -999.0) & (error != -999.0)
        m = QFA(nb, nr, nh, dev, model_params=params)
        m.mu = torch.tensor(mu, device=dev)
        wins = [velocity_window(wav, lam, 0.0, 25000.0, nb) for lam in DEFAULT_LINES]
        n_win = [w[1] - w[0] for w in wins]
        ved = [torch.tensor(w[2], device=dev) for w in wins]
        ind = check_indices(None)
        for S in (1, 100):
            h = torch.randn((a.batch, S, nh), device=dev)
            fn = lambda: m.bal_scan(flux, error, mask, h=h, wav_grid=wav)
            for _ in range(a.warmup):
                scan = fn()
            torch.cuda.synchronize()
            ms = float(np.median(timed(fn, a.steps)))
            bs, keep = m._flux_batch(flux, error, mask)
            dwin = m._bal_windows(wav, DEFAULT_LINES, ind)
            cfn = lambda: m._bal_call(bs, h, a.batch, dwin, DEFAULT_LINES, ind, 0.9, 1, 0, 0.0, "AI")
            for _ in range(a.warmup):
                cfn()
            torch.cuda.synchronize()
            ms_call = float(np.median(timed(cfn, a.steps)))
            se = min(S, a.eager_draws)
            hs = h[:, :se].contiguous()
            efn = lambda: [[eager_index(m, flux, error, mask, hs, w[0], w[1], v, d, 0.9) for d in DEFAULT_INDICES.values()]
                           for w, v in zip(wins, ved)]
            ref = efn()
            for _ in range(a.warmup):
                efn()
            torch.cuda.synchronize()
            ems = float(np.median(timed(efn, a.steps))) * S / se
            bytes_ = a.batch * (sum(n_win) * 9 + S * (nh * 4 + len(wins) * OUT_BYTES))
            floor_ms = bytes_ / (COPY_TBS * 1e12) * 1e3
            dmax = max(float(((scan.value[:, :se, l, x] - ref[l][x]).abs() / scan.value[:, :se, l, x].abs().clamp(min=1.0)).max())
                       for l in range(len(wins)) for x in range(2))
            line = {"shape": name, "B": a.batch, "Npix": npix, "Nh": nh, "S": S, "lines": list(DEFAULT_LINES), "n_win": n_win,
                    "ms_scan": round(ms, 4), "ms_call": round(ms_call, 4), "ms_byte_floor": round(floor_ms, 5), "copy_TBs": COPY_TBS,
                    "floor_over_call": round(floor_ms / ms_call, 4), "bytes_per_spectrum_draw": round(bytes_ / (a.batch * S), 1),
                    "ms_eager_scaled": round(ems, 3), "eager_draws": se, "x_eager": round(ems / ms_call, 2),
                    "max_rel_value_minus_eager": dmax, "frac_bal_bi": float((scan.bi()[:, 0] > 0).any(-1).double().mean()),
                    "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            log.write(json.dumps(line) + "\n")
            log.flush()
            del h, hs
        del flux, error, mask, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
