"""Timing of the forest transmission and its stack (not the flagship benchmark: that is bench.py): the fused call
(QFA.forest, qfa_forest_f32) against the eager composition it replaces, in the same process on the same GPU --
continua materialised by ``continua_from_latent`` (B, S, Npix), torch division and inverse variance on the blue side, then
``index_add_`` of w, w T, w T^2 and the count into the bins (float atomics).  The latent draws h are formed once outside both
timings.  One JSON line per shape and S into profiles/forest_bench.jsonl: median ms of each form over ``--iters`` calls after a
warm-up call, the fused call's algorithmic bytes and flops, and the rates they give.

    python tools/bench_forest.py [--shapes B:Npix:Nb:Nh:S ...] [--iters 10] [--nbin 64] [--out profiles/forest_bench.jsonl]"""
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
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:1913:720:8:1", "4096:1913:720:8:100", "4096:4000:2000:16:1",
                                                    "4096:4000:2000:16:100"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nbin", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forest_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for spec in a.shapes:
        B, npix, nb, nh, S = (int(x) for x in spec.split(":"))
        rng = np.random.default_rng(0)
        p = {"F": (rng.uniform(-1, 1, (npix, nh)) * 0.1 / np.sqrt(nh)).astype(np.float32), "Psi": np.ones(npix, np.float32),
             "omega": np.ones(nb, np.float32), "tau0": np.float32(0.02), "c0": np.float32(0.3), "beta": np.float32(2.0)}
        m = QFA(nb, npix - nb, nh, dev, model_params=p)
        m.mu = torch.tensor((1.0 + 0.1 * np.sin(np.arange(npix) / 7.0)).astype(np.float32), device=dev)
        flux = torch.rand((B, npix), device=dev)
        error = 0.01 + 0.09 * torch.rand((B, npix), device=dev)
        mask = torch.rand((B, npix), device=dev) > 0.1
        zq1 = (3.0 + 1.5 * torch.rand(B, device=dev)).contiguous()
        ratio = torch.tensor((10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32), device=dev)
        zabs = (zq1[:, None] * ratio[None, :] - 1.0).contiguous()
        h = torch.randn((B, S, nh), device=dev).clamp_(-3, 3)
        z0, dz = 1.5, 2.1 / a.nbin
        bins = (z0, dz, a.nbin)
        stack = m.forest(flux, error, zabs, mask, h=h, bins=bins, return_pixels=False)[2]

        def fused_stack():
            stack.buf.zero_()
            m.forest(flux, error, zabs, mask, h=h, stack=stack, return_pixels=False)

        def fused_all():
            stack.buf.zero_()
            return m.forest(flux, error, zabs, mask, h=h, stack=stack)

        def fused_factored():
            stack.buf.zero_()
            m.forest(flux, error, None, mask, h=h, stack=stack, zfac=(zq1, ratio), return_pixels=False)

        k = torch.floor((zabs - np.float32(z0)) * (np.float32(1.0) / np.float32(dz))).long().clamp_(0, a.nbin - 1)
        kk = k[:, None, :].expand(B, S, nb)

        def eager():
            cont = m.continua_from_latent(h)[:, :, :nb]                          # (B, S, Npix) materialised
            T = flux[:, None, :nb] / cont
            iv = cont * cont / (error[:, None, :nb] ** 2)
            use = mask[:, None, :nb] & (cont > 0.0) & torch.isfinite(T) & torch.isfinite(iv)
            T = torch.where(use, T, torch.zeros_like(T)).double()
            iv = torch.where(use, iv, torch.zeros_like(iv)).double()
            out = torch.zeros((S, 4, a.nbin), dtype=torch.float64, device=dev)
            idx = (torch.arange(S, device=dev)[None, :, None] * (4 * a.nbin) + kk).reshape(-1)
            flat = out.view(-1)
            for q, v in enumerate((iv, iv * T, iv * T * T, use.double())):
                flat.index_add_(0, idx + q * a.nbin, v.reshape(-1))
            return out

        ms_stack = time_ms(fused_stack, a.iters)
        ms_all = time_ms(fused_all, a.iters)
        ms_fac = time_ms(fused_factored, a.iters)
        ms_eager = time_ms(eager, max(3, a.iters // 3))
        # the fused call's algorithmic traffic: flux, error, z (4 bytes each) and the mask (1) per blue pixel and launch, h, and the
        # two outputs when asked for; flops per (b, s, p): the fma chain (2 Nh) + 2 divisions, 5 products / adds
        read = B * nb * 13.0 + 4.0 * B * S * nh
        written = 8.0 * B * S * nb
        flops = B * S * nb * (2.0 * nh + 7.0)
        line = {"B": B, "Npix": npix, "Nb": nb, "Nh": nh, "S": S, "nbin": a.nbin,
                "ms_fused_stack_only": round(ms_stack[0], 4), "ms_fused_pixels_and_stack": round(ms_all[0], 4),
                "ms_fused_stack_only_factored_z": round(ms_fac[0], 4), "ms_eager": round(ms_eager[0], 4),
                "min_max_ms_fused_stack_only": [round(ms_stack[1], 4), round(ms_stack[2], 4)],
                "min_max_ms_eager": [round(ms_eager[1], 4), round(ms_eager[2], 4)],
                "eager_over_fused_pixels_and_stack": round(ms_eager[0] / ms_all[0], 2),
                "eager_over_fused_stack_only": round(ms_eager[0] / ms_stack[0], 2),
                "GB_read": round(read / 1e9, 4), "GB_written_pixels": round(written / 1e9, 4),
                "pixels_and_stack_TBps": round((read + written) / ms_all[0] / 1e9, 3),
                "stack_only_Gpix_per_s": round(B * S * nb / ms_stack[0] / 1e6, 2),
                "stack_only_TFLOPs_f32": round(flops / ms_stack[0] / 1e9, 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del h, kk, k
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
