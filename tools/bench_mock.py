"""Timing of the mock-spectrum writer k_mock_spectra (qfa_mock_spectra_f32; not the flagship benchmark: that is bench.py) with
events, on the synthetic recipe's parameters and geometry (factored-z form, masks on).  One JSON line per shape: median ms per
call of the writer alone (h given), of the latent draw in front of it, the writer's rate in written TB/s (algorithmic bytes:
4 Npix per row written; per spectrum it reads 5 Npix bytes of error and mask once for all S replicates) and in normals per
second.  Two comparators in the same run: the continuum writer k_sample_cont on the same (B, S, Npix) -- the same bytes written
with no normals drawn, i.e. what HBM alone allows -- and, with --torch on the FIRST shape, synthetic.make_batch_torch, the
eager torch generator (about a dozen passes over (B, Npix) temporaries, torch's own random stream).

    python tools/bench_mock.py [--shapes B:Npix:Nh:S ...] [--iters 10] [--torch] [--out FILE]"""
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
    from qfa_amd import QFA, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["100000:4000:16:1", "4096:1913:8:100"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch", action="store_true", help="time synthetic.make_batch_torch on the first shape")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for k, spec in enumerate(a.shapes):
        B, npix, nh, S = (int(x) for x in spec.split(":"))
        wav, nb, nr = synthetic.wavelength_grid(None if npix == 1913 else npix)
        p, mu = synthetic.mock_parameters(npix, nb, nh, seed=1)
        m = QFA(nb, nr, nh, dev, model_params=p)
        m.mu = torch.tensor(mu, device=dev)
        res = {"B": B, "Npix": npix, "Nb": nb, "Nh": nh, "S": S}
        if a.torch and k == 0:
            fn = lambda: synthetic.make_batch_torch(p, mu, wav, nb, B, 3, dev, return_flux=True)
            res["ms_make_batch_torch"] = round(time_ms(fn, max(3, a.iters // 2)), 4)
            torch.cuda.empty_cache()
        flux, error, zq = synthetic.make_batch_torch(p, mu, wav, nb, B, 3, dev, return_flux=True)
        mask = (flux != -999.0).contiguous()
        del flux
        zfac = ((1.0 + zq).contiguous(), torch.tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev))
        hmean = torch.zeros((B, nh), dtype=torch.float32, device=dev)
        hcov = torch.eye(nh, dtype=torch.float32, device=dev).repeat(B, 1, 1).contiguous()
        h = torch.empty((B, S, nh), dtype=torch.float32, device=dev)
        out = torch.empty((B, S, npix), dtype=torch.float32, device=dev)
        ms_lat = time_ms(lambda: m.sample_latent(hmean, hcov, S, seed=1, out=h), a.iters)
        ms_mock = time_ms(lambda: m.sample_spectra(error, None, mask, n_samples=S, seed=1, h=h, zfac=zfac, out=out), a.iters)
        ms_cont = time_ms(lambda: m.continua_from_latent(h, out=out), a.iters)
        written = 4.0 * B * S * npix
        res.update({"GB_written": round(written / 1e9, 3), "ms_latent": round(ms_lat, 4), "ms_mock": round(ms_mock, 4),
                    "ms_cont_same_bytes": round(ms_cont, 4), "mock_over_cont": round(ms_mock / ms_cont, 3),
                    "mock_TBps_written": round(written / ms_mock / 1e9, 3),
                    "mock_Gnormals_per_s": round(B * S * npix / ms_mock / 1e6, 2)})
        if "ms_make_batch_torch" in res:
            res["torch_over_hip"] = round(res["ms_make_batch_torch"] / (ms_lat + ms_mock), 3)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del out, h, error, mask
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
