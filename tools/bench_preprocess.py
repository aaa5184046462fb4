"""Time qfa_amd.preprocess.preprocess at survey size and write profiles/preprocess_bench.jsonl.

Two shapes, N spectra each (default 100 000): SDSS-like (n_in 4 600 on a 1e-4 dex grid, Npix 1 913) and DESI-like (n_in 7 800
linear 0.8 A, Npix 9 243).  Per shape one JSON line: the median, minimum and maximum of `--repeats` timed calls (device events
around the whole Python call -- host checks of the offsets, uploads and allocations of the wrapper included --, outputs
preallocated, after `--warmup` calls); the same for the C-ABI call alone on tensors made beforehand (`kernels_ms_*`: the two
launches of qfa_preprocess_f32 and nothing else between the events, i.e. chip time); the byte floor -- input bytes + 8 N Npix output
bytes at the copy bandwidth DESIGN.md quotes (4 TB/s) -- and the numpy float64 restatement (tests/_preprocess_ref.py) on 16
processes over a sub-sample of `--baseline` spectra, scaled to N.  The baseline runs first, before this process opens the GPU.

    python tools/bench_preprocess.py [--n 100000] [--repeats 7] [--warmup 2] [--baseline 32] [--out profiles/preprocess_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
COPY_TBS = 4.0

SHAPES = {
    "sdss": dict(n_in=4600, npix=1913, log=True, step=1e-4, w0=3600.0),
    "desi": dict(n_in=7800, npix=9243, log=False, step=0.8, w0=3600.0),
}


def grid_of(npix):
    return 1030.0 * 10 ** (np.log10(1600.0 / 1030.0) / npix * np.arange(npix))


def host_spectrum(shape, i):
    s = SHAPES[shape]
    rng = np.random.default_rng(1000 + i)
    j = np.arange(s["n_in"]) + rng.uniform(0, 1)
    w = s["w0"] * 10 ** (s["step"] * j) if s["log"] else s["w0"] + s["step"] * j
    return w, rng.normal(1, 0.2, s["n_in"]).astype(np.float32), rng.uniform(1, 9, s["n_in"]).astype(np.float32), 2.2 + 0.8 * rng.uniform()


def _baseline_one(arg):
    import _preprocess_ref as R
    shape, i = arg
    w, f, v, z = host_spectrum(shape, i)
    g = grid_of(SHAPES[shape]["npix"])
    t = time.perf_counter()
    R.preprocess_ref(w, f, v, np.array([0, len(w)]), np.array([z]), g)
    return time.perf_counter() - t


def baseline(shape, k):
    t = time.perf_counter()
    with ProcessPoolExecutor(max_workers=16) as ex:
        list(ex.map(_baseline_one, [(shape, i) for i in range(k)]))
    return (time.perf_counter() - t) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "preprocess_bench.jsonl"))
    a = ap.parse_args()
    base = {k: baseline(k, a.baseline) for k in SHAPES}      # seconds per spectrum on 16 processes, before the GPU is opened
    import torch
    from qfa_amd.preprocess import preprocess
    dev = torch.device("cuda:0")
    lines = []
    for name, s in SHAPES.items():
        N, n, npix = a.n, s["n_in"], s["npix"]
        gen = torch.Generator(device=dev).manual_seed(1)
        j = torch.arange(n, dtype=torch.float64, device=dev)[None, :] + torch.rand((N, 1), dtype=torch.float64, device=dev, generator=gen)
        wave = (s["w0"] * 10 ** (s["step"] * j) if s["log"] else s["w0"] + s["step"] * j).reshape(-1)
        del j
        flux = 1 + 0.2 * torch.randn(N * n, dtype=torch.float32, device=dev, generator=gen)
        ivar = 1 + 8 * torch.rand(N * n, dtype=torch.float32, device=dev, generator=gen)
        bad = torch.zeros(N * n, dtype=torch.uint8, device=dev)
        zq = 2.2 + 0.8 * torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
        off = np.arange(N + 1, dtype=np.int64) * n
        grid = grid_of(npix)
        out = (torch.empty((N, npix), dtype=torch.float32, device=dev), torch.empty((N, npix), dtype=torch.float32, device=dev))
        ms = []
        for r in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            p = preprocess(wave, flux, ivar, off, zq, grid, bad=bad, device=dev, out=out)
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        # the C-ABI call alone: every argument on the device beforehand, nothing but the two launches between the events
        import ctypes as C
        from qfa_amd import _lib
        from qfa_amd.preprocess import edges_from_grid
        h = _lib.lib()
        T = lambda x: torch.as_tensor(x, device=dev)
        off_d, e_d, g_d = T(off), T(edges_from_grid(grid)), T(grid)
        rf, ri = torch.empty((N, 2), dtype=torch.float64, device=dev), torch.empty((N, 5), dtype=torch.int32, device=dev)
        wsb = h.qfa_preprocess_workspace_bytes(N, npix, n)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        q = _lib.PreprocessParams(0.5, 1270.0, 1290.0, 1270.0, 1600.0, 5)
        kms = []
        for r in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(h.qfa_preprocess_f32(_lib._ptr(wave), _lib._ptr(flux), _lib._ptr(ivar), _lib._ptr(bad), _lib._ptr(off_d),
                                            _lib._ptr(zq), N, n, _lib._ptr(e_d), _lib._ptr(g_d), npix, C.byref(q), _lib._ptr(out[0]),
                                            _lib._ptr(out[1]), _lib._ptr(rf), _lib._ptr(ri), _lib._ptr(ws), wsb,
                                            _lib.current_stream(dev)), "qfa_preprocess_f32")
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                kms.append(e0.elapsed_time(e1))
        assert torch.equal(rf[:, 0], p.norm)                 # the same call as the wrapper's
        in_bytes = N * n * 17 + (N + 1) * 8 + N * 8
        out_bytes = 8 * N * npix
        floor_ms = (in_bytes + out_bytes) / (COPY_TBS * 1e12) * 1e3
        med = float(np.median(ms))
        lines.append(dict(shape=name, N=N, n_in=n, Npix=npix, ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)),
                          kernels_ms_median=float(np.median(kms)), kernels_ms_min=float(min(kms)), kernels_ms_max=float(max(kms)),
                          repeats=a.repeats, warmup=a.warmup, input_bytes=in_bytes, output_bytes=out_bytes, copy_TBs=COPY_TBS,
                          floor_ms=floor_ms, times_floor=med / floor_ms, kernels_times_floor=float(np.median(kms)) / floor_ms, ok_fraction=float(p.ok.float().mean()),
                          numpy16_s_per_spectrum=base[name], numpy16_ms_scaled_to_N=base[name] * N * 1e3,
                          numpy16_subsample=a.baseline, device=torch.cuda.get_device_name(0)))
        print(json.dumps(lines[-1]), flush=True)
        del wave, flux, ivar, bad, out, p
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
