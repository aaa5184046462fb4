"""Timing of the posterior draws (not the flagship benchmark: that is bench.py): k_sample_latent (qfa_sample_latent_f32) and
the continuum writer k_sample_cont (qfa_continua_f32) with events, on random F, mu and a random SPD posterior.  One JSON line
per shape: shape, S, median ms per call and the writer's rate in written TB/s (algorithmic bytes: 4 Npix per row written
plus the 4 Nh bytes of its h read; F and mu are read once per block and stay in L2).

    python tools/bench_sample.py [--shapes B:Npix:Nh:S ...] [--iters 20]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def time_ms(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:1913:8:100", "4096:4000:16:100", "4096:1913:32:100",
                                                    "4096:1913:8:16"])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in a.shapes:
        B, npix, nh, S = (int(x) for x in spec.split(":"))
        rng = np.random.default_rng(0)
        p = {"F": rng.uniform(-0.5, 0.5, (npix, nh)).astype(np.float32), "Psi": np.ones(npix, np.float32),
             "omega": np.ones(0, np.float32), "tau0": np.float32(0.02), "c0": np.float32(0.3), "beta": np.float32(2.0)}
        m = QFA(0, npix, nh, dev, model_params=p)
        m.mu = torch.tensor(rng.uniform(0.5, 2.0, npix).astype(np.float32), device=dev)
        G = torch.randn((B, nh, nh), device=dev)
        hcov = (G @ G.transpose(1, 2) / nh + 0.1 * torch.eye(nh, device=dev)).contiguous()
        hmean = torch.randn((B, nh), device=dev)
        h = torch.empty((B, S, nh), dtype=torch.float32, device=dev)
        out = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
        ms_lat = time_ms(lambda: m.sample_latent(hmean, hcov, S, seed=1, out=h), a.iters)
        ms_cont = time_ms(lambda: m.continua_from_latent(h, out=out), a.iters)
        R = B * S
        written = 4.0 * R * npix
        print(json.dumps({"B": B, "Npix": npix, "Nh": nh, "S": S, "GB_written": round(written / 1e9, 3),
                          "ms_latent": round(ms_lat, 4), "ms_cont": round(ms_cont, 4),
                          "latent_over_cont": round(ms_lat / ms_cont, 4),
                          "cont_TBps": round((written + 4.0 * R * nh) / ms_cont / 1e9, 3)}), flush=True)
        del out, h


if __name__ == "__main__":
    main()
