"""Timing of the sightline bootstrap of the P1D rows (not the flagship benchmark: that is bench.py): qfa_segment_codes_f32 and
qfa_bootstrap_f64 -- the bare C calls between two device events ("kernels") and QFA.segment_codes + QFA.segment_bootstrap ("call") --
against the eager composition on the same GPU in the same run: the (B, R) weight matrix from a host table (the contract's weights,
generated outside the timing), and per z-bin a float64 ``matmul`` of the gathered weights (R x n) with the gathered rows
(n x (1 + W)).  The rows [noise | power] of QFA.p1d are formed once outside both timings.  One JSON line per shape and R into
profiles/bootstrap_bench.jsonl: median / min / max ms over ``--iters`` calls after a warm-up call, the algorithmic bytes (the rows and
codes read once per tile of 256 replicates, boot written once) and float64 flops (2 R n (1 + W)), and the rates they give.

    python tools/bench_bootstrap.py [--shapes B:Nb:nseg:S ...] [--boots 100 1000] [--iters 7] [--nz 8] [--out profiles/bootstrap_bench.jsonl]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, inputs, ms, time_ms, write  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import numpy as np
    import torch
    import _bootstrap_ref
    from qfa_amd import QFA, _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:2000:3:1"])
    ap.add_argument("--boots", nargs="*", type=int, default=[100, 1000])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bootstrap_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = _lib.lib()
    for spec in a.shapes:
        c = inputs(spec, a.nz, dev)
        B, nb, nseg, S, L, nz = c.B, c.nb, c.nseg, c.S, c.L, c.nz
        m = QFA(nb, 8, 4, dev)
        bins = (c.z0, c.dz, nz)
        power, noise, _ = m.p1d(c.trans, c.ivar, **c.kw)
        rows = torch.cat([noise.unsqueeze(-1), power], -1).contiguous()          # (B, S, nseg, 1 + M)
        W = int(rows.shape[-1])
        codes = m.segment_codes(c.trans, c.ivar, bins=bins, **c.kw)
        n_valid = int((codes >= 0).sum())
        t_codes = time_ms(lambda: m.segment_codes(c.trans, c.ivar, bins=bins, **c.kw), a.iters)
        for R in a.boots:
            boot = torch.zeros((S, R, nz, 1 + W), dtype=torch.float64, device=dev)
            ws = torch.empty(h.qfa_bootstrap_workspace_bytes(B, S, nseg, W, nz, R), dtype=torch.uint8, device=dev)
            stream = _lib.current_stream(dev)

            def kernels():
                _lib.check(h.qfa_bootstrap_f64(C.c_void_p(rows.data_ptr()), 0, C.c_void_p(codes.data_ptr()), B, S, nseg, W, nz, R, a.seed, 0,
                                               _lib.F_ZERO_ACCUM, C.c_void_p(boot.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                               stream), "qfa_bootstrap_f64")

            def call():
                return m.segment_bootstrap(rows, codes, n_boot=R, seed=a.seed, nz=nz)

            def whole():
                cd = m.segment_codes(c.trans, c.ivar, bins=bins, **c.kw)
                return m.segment_bootstrap(rows, cd, n_boot=R, seed=a.seed, nz=nz)

            wt = torch.tensor(_bootstrap_ref.weights(a.seed, np.arange(B), R).astype(np.float64), device=dev)    # (B, R), host table
            x1 = torch.cat([torch.ones_like(rows[..., :1], dtype=torch.float64), rows.double()], -1)              # outside: [1 | x]
            spec_of = torch.arange(B, device=dev)[:, None].expand(B, nseg)
            est = torch.zeros_like(boot)

            def eager():
                for s in range(S):
                    for kz in range(nz):
                        sel = codes[:, s] == kz
                        est[s, :, kz] = wt[spec_of[sel]].T @ x1[:, s][sel]

            t_k, t_call, t_whole, t_eager = (time_ms(f, a.iters) for f in (kernels, call, whole, eager))
            kernels()
            eager()
            torch.cuda.synchronize()
            assert torch.equal(boot[..., 0], est[..., 0]), "weighted counts differ"
            rel = float(((boot - est).abs() / est.abs().clamp_min(1e-300))[est != 0].max())
            tiles = (R + 255) // 256
            byts = tiles * (n_valid * W * 4 + B * S * nseg * 4) + S * R * nz * (1 + W) * 8
            flops = 2 * R * n_valid * (1 + W)
            rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "M": L // 2, "S": S, "nz": nz, "W": W, "R": R, "valid_segments": n_valid},
                   "codes_call_ms": ms(t_codes), "bootstrap_kernels_ms": ms(t_k), "bootstrap_call_ms": ms(t_call),
                   "codes_and_bootstrap_call_ms": ms(t_whole), "eager_ms": ms(t_eager),
                   "eager_over_kernels": t_eager[0] / t_k[0], "eager_over_call": t_eager[0] / t_call[0],
                   "algorithmic_bytes": byts, "algorithmic_f64_flops": flops,
                   "kernels_TBps": byts / t_k[0] * 1e-9, "kernels_f64_TFLOPs": flops / t_k[0] * 1e-9,
                   "max_rel_diff_to_eager": rel, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
            write(a.out, rec)
            del boot, est, wt, x1
            torch.cuda.empty_cache()
        del c, rows, codes, power, noise


if __name__ == "__main__":
    main()
