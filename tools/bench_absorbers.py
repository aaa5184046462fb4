#!/usr/bin/env python3
"""Time qfa_absorber_mask_f32 on the GPU: the SDSS shape (N 4 096 x 1 913 pixels) and N 100 000 x 4 000, with 0, 1 and 4
absorbers per spectrum (Ly-alpha and Ly-beta each).  Per (shape, absorbers) one JSON line: the median, minimum and maximum of
`--repeats` timed C-ABI calls on tensors made beforehand (device events around the one launch, after `--warmup` calls; chip time);
the same for the eager torch composition of the same rule on the same GPU in the same run -- a float64 (n, Npix, lines) broadcast,
in chunks of spectra that keep one temporary under `--chunk_gib` -- which forms T, the mask and the two quotients but no record;
the 16-byte-per-pixel floor (flux and error read, both written) at the copy bandwidth DESIGN.md quotes (4 TB/s), and the time of
the plain device copy of the two arrays measured in the same run.  No time is a pass / fail bar.

    python tools/bench_absorbers.py [--out profiles/absorber_bench.jsonl] [--repeats 7 --warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_TBS = 4.0
SHAPES = (("sdss", 4096, 1913, 1030.0, 1e-4), ("100k x 4000", 100000, 4000, 1030.0, 4.78e-5))
LINES = ((1215.67, 0.4164, 6.265e8), (1025.72, 0.07912, 1.897e8))
G = (2.0, -4.0, 5.0 / 3.0, 14.0 / 15.0, -8.0 / 5.0, 352.0 / 315.0, -169.0 / 315.0, 38.0 / 189.0, -884.0 / 14175.0,
     2584.0 / 155925.0)


def eager(torch, flux, error, zq, grid, off, za, lg, n_abs, chunk, t_min=0.8, b=30.0):
    """the rule as whole-tensor torch operations, float64; returns flux_out, error_out"""
    N, npix = flux.shape
    fo, eo = torch.empty_like(flux), torch.empty_like(error)
    lam0 = torch.tensor([l[0] for l in LINES], dtype=torch.float64, device=flux.device)
    f_osc = torch.tensor([l[1] for l in LINES], dtype=torch.float64, device=flux.device)
    gam = torch.tensor([l[2] for l in LINES], dtype=torch.float64, device=flux.device)
    ka = gam * lam0 * 1e-13 / (4.0 * np.pi * b) / np.sqrt(np.pi)
    for a in range(0, N, chunk):
        e = min(N, a + chunk)
        lam = grid[None, :] * (1.0 + zq[a:e, None])
        if n_abs:
            z = za[a * n_abs:e * n_abs].view(e - a, 1, n_abs, 1)
            coef = 1.497e-15 * 10.0 ** lg[a * n_abs:e * n_abs].view(e - a, 1, n_abs, 1) * f_osc * lam0 / b
            x = (299792.458 / b) * (lam[:, :, None, None] / (lam0 * (1.0 + z)) - 1.0)
            P = x * x
            H0, Q = torch.exp(-P), 1.5 / P
            main = H0 - (ka / P) * (H0 * H0 * (4.0 * P * P + 7.0 * P + 4.0 + Q) - Q - 1.0)
            g = torch.zeros_like(P)
            for c in G[::-1]:
                g = g * P + c
            H = torch.where(P < 0.0625, H0 - ka * g, torch.where(P > 750.0, (ka / P) * (1.0 + Q), main))
            T = torch.exp(-(coef * H).sum(dim=(2, 3)))
        else:
            T = torch.ones_like(lam)
        f, r = flux[a:e], error[a:e]
        keep = (f != -999.0) & (r != -999.0) & (T >= t_min) & torch.isfinite(T)
        fo[a:e] = torch.where(keep, (f.double() / T).float(), torch.full_like(f, -999.0))
        eo[a:e] = torch.where(keep, (r.double() / T).float(), torch.full_like(r, -999.0))
    return fo, eo


def timed(torch, fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "absorber_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager_repeats", type=int, default=3)
    ap.add_argument("--chunk_gib", type=float, default=1.0)
    ap.add_argument("--shapes", nargs="*", default=None, help="names of the shapes to run (default: all)")
    a = ap.parse_args(argv)
    import torch
    from qfa_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_absorbers needs a GPU: no time is taken anywhere else")
    dev = torch.device("cuda:0")
    h = _lib.lib()
    lines = []
    for name, N, npix, lam_min, step in SHAPES:
        if a.shapes and name not in a.shapes:
            continue
        gen = torch.Generator(device=dev).manual_seed(7)
        grid_h = lam_min * 10 ** (step * np.arange(npix))
        grid = torch.as_tensor(grid_h, device=dev)
        flux = 1.0 + 0.2 * torch.randn((N, npix), generator=gen, device=dev)
        error = 0.05 + 0.25 * torch.rand((N, npix), generator=gen, device=dev)
        bad = torch.rand((N, npix), generator=gen, device=dev) < 0.02
        flux[bad] = -999.0
        error[bad] = -999.0
        zq = 2.2 + 1.3 * torch.rand((N,), generator=gen, device=dev, dtype=torch.float64)
        fo, eo = torch.empty_like(flux), torch.empty_like(error)
        rf = torch.empty((N, 1), dtype=torch.float64, device=dev)
        ri = torch.empty((N, 6), dtype=torch.int32, device=dev)
        ws = torch.empty((16,), dtype=torch.uint8, device=dev)
        q = _lib.AbsorberParams(0.8, 30.0, 1270.0, 1600.0, _lib.ABS_LYB | _lib.ABS_CORRECT)
        st = _lib.current_stream(dev)
        p = _lib._ptr
        copy = timed(torch, lambda: (fo.copy_(flux), eo.copy_(error)), a.repeats, a.warmup)
        floor_ms = 16.0 * N * npix / (COPY_TBS * 1e12) * 1e3
        for n_abs in (0, 1, 4):
            # every absorber's Ly-alpha inside the spectrum's forest, log N_HI 20.3 .. 21.5
            lam_abs = 1050.0 + 150.0 * torch.rand((N, max(n_abs, 1)), generator=gen, device=dev, dtype=torch.float64)
            za = (lam_abs * (1.0 + zq[:, None]) / 1215.67 - 1.0)[:, :n_abs].reshape(-1).contiguous()
            lg = (20.3 + 1.2 * torch.rand((N * n_abs,), generator=gen, device=dev, dtype=torch.float64)).contiguous()
            off = torch.arange(N + 1, device=dev, dtype=torch.int64) * n_abs
            args = (p(off), p(za), p(lg)) if n_abs else (None, None, None)

            def fused():
                _lib.check(h.qfa_absorber_mask_f32(p(flux), p(error), p(zq), p(grid), N, npix, *args, None, 0, None, None,
                                                   C.byref(q), p(fo), p(eo), None, p(rf), p(ri), p(ws), 16, st),
                           "qfa_absorber_mask_f32")
            k = timed(torch, fused, a.repeats, a.warmup)
            n_lines = max(1, 2 * n_abs)
            chunk = max(1, min(N, int(a.chunk_gib * 2 ** 30 / (8.0 * npix * n_lines))))
            e = timed(torch, lambda: eager(torch, flux, error, zq, grid, off, za, lg, n_abs, chunk), a.eager_repeats, 1)
            ef, ee = eager(torch, flux, error, zq, grid, off, za, lg, n_abs, chunk)
            fused()
            same_mask = bool(torch.equal(ef == -999.0, fo == -999.0))
            kept = fo != -999.0
            max_rel = float(((ef[kept] - fo[kept]).abs() / fo[kept].abs().clamp_min(1e-30)).max()) if bool(kept.any()) else 0.0
            lines.append(dict(shape=name, N=N, Npix=npix, n_abs=n_abs, lines_per_spectrum=2 * n_abs,
                              kernel_ms_median=k[0], kernel_ms_min=k[1], kernel_ms_max=k[2], repeats=a.repeats, warmup=a.warmup,
                              eager_ms_median=e[0], eager_ms_min=e[1], eager_ms_max=e[2], eager_repeats=a.eager_repeats,
                              eager_chunk=chunk, eager_over_kernel=e[0] / k[0],
                              floor_bytes_per_pixel=16, copy_TBs=COPY_TBS, floor_ms=floor_ms, times_floor=k[0] / floor_ms,
                              copy_ms_median=copy[0], times_copy=k[0] / copy[0], achieved_TBs=16.0 * N * npix / (k[0] * 1e-3) / 1e12,
                              masked_fraction=float(((fo == -999.0) & ~bad).float().mean()), eager_same_mask=same_mask,
                              eager_max_rel_diff=max_rel, device=torch.cuda.get_device_name(0)))
            print(json.dumps(lines[-1]), flush=True)
        del flux, error, fo, eo
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
