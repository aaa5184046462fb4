"""Timing of the 1D flux power spectrum and its stack (not the flagship benchmark: that is bench.py): the fused call (QFA.p1d,
qfa_p1d_f32) against the eager composition it replaces, in the same process on the same GPU -- delta_F and the noise variance
materialised (B, S, Nb), ``torch.fft.rfft`` per segment, |X|^2 / L, then ``index_add_`` of [1 | N | P | P^2] in float64 into the
(draw, z-bin) rows (float atomics).  trans / ivar are formed once outside both timings.  One JSON line per shape and S into
profiles/p1d_bench.jsonl: median / min / max ms of each form over ``--iters`` calls after a warm-up call, the fused call's
algorithmic bytes and flops, and the rates they give.

    python tools/bench_p1d.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--out profiles/p1d_bench.jsonl]"""
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
    from qfa_amd.model import P1DStack
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:720:3:100", "4096:2000:3:1", "4096:2000:3:100"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "p1d_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for spec in a.shapes:
        B, nb, nseg, S = (int(x) for x in spec.split(":"))
        L, nT, nz = nb // nseg, 64, a.nz
        M = L // 2
        min_used = int(np.ceil(0.75 * L))
        m = QFA(nb, 8, 4, dev)
        torch.manual_seed(0)
        trans = torch.rand((B, S, nb), device=dev) * 1.2
        ivar = 10.0 + 90.0 * torch.rand((B, S, nb), device=dev)
        ivar.mul_(torch.rand((B, S, nb), device=dev) > 0.2)               # 20 % unused pixels: segments on both sides of min_used
        zq1 = (3.0 + 1.5 * torch.rand(B, device=dev)).contiguous()
        ratio = torch.tensor((10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32), device=dev)
        zabs = (zq1[:, None] * ratio[None, :] - 1.0).contiguous()
        zT0, dzT = np.float32(1.5), np.float32(2.1 / nT)
        z0, dz = np.float32(1.6), np.float32(1.8 / nz)
        tbar = (0.3 + 0.6 * torch.rand((S, nT), device=dev)).contiguous()
        stack = P1DStack.zeros(S, z0, dz, nz, L, 69.0, dev)
        kw = dict(zabs=zabs, tbar=tbar, tbar_bins=(zT0, dzT, nT), seg_len=L, n_segments=nseg, min_used=min_used)

        def fused_stack():
            stack.buf.zero_()
            m.p1d(trans, ivar, stack=stack, return_segments=False, **kw)

        def fused_all():
            stack.buf.zero_()
            return m.p1d(trans, ivar, stack=stack, **kw)

        est = torch.zeros_like(stack.buf)
        kT = torch.floor((zabs - zT0) * (np.float32(1.0) / dzT)).long()
        okT = (kT >= 0) & (kT < nT)
        kT.clamp_(0, nT - 1)
        zc = zabs[:, torch.arange(nseg, device=dev) * L + L // 2]
        kz = torch.floor((zc - z0) * (np.float32(1.0) / dz)).long()
        okz = (kz >= 0) & (kz < nz)
        row = torch.arange(S, device=dev)[None, :, None] * nz + kz.clamp(0, nz - 1)[:, None, :]     # (B, S, nseg)

        def eager():
            est.zero_()
            tb = tbar[:, kT].permute(1, 0, 2)                            # (B, S, Nb)
            used = (ivar > 0) & okT[:, None, :] & (tb > 0)
            zero = torch.zeros((), device=dev)
            d = torch.where(used, trans / tb - 1.0, zero)[..., :nseg * L].reshape(B, S, nseg, L)
            v = torch.where(used, 1.0 / (ivar * (tb * tb)), zero)[..., :nseg * L].reshape(B, S, nseg, L)
            X = torch.fft.rfft(d, dim=-1)[..., 1:M + 1]
            P = (X.real * X.real + X.imag * X.imag) / L
            N = v.sum(-1) / L
            ok = (used[..., :nseg * L].reshape(B, S, nseg, L).sum(-1) >= min_used) & okz[:, None, :]
            Pd = P.double()
            terms = torch.cat([torch.ones_like(N, dtype=torch.float64)[..., None], N.double()[..., None], Pd, Pd * Pd], -1)
            est.view(S * nz, 2 + 2 * M).index_add_(0, row[ok], terms[ok])
            return P, N

        t_stack, t_all, t_eager = time_ms(fused_stack, a.iters), time_ms(fused_all, a.iters), time_ms(eager, a.iters)
        # the two forms agree (the eager sums are float64 atomics in another order)
        fused_stack()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(stack.n, est[:, :, 0]), "counts differ"
        rel = float(((stack.buf - est).abs() / est.abs().clamp_min(1e-300))[est != 0].max())
        nsegs = B * S * nseg
        byts = 2 * 4 * nsegs * L                                           # trans and ivar of the segments, read once
        flops = nsegs * 2 * L * 2 * M                                      # the product: L x 2M multiply-adds per segment
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "min_used": min_used},
               "fused_stack_ms": {"median": t_stack[0], "min": t_stack[1], "max": t_stack[2]},
               "fused_stack_and_segments_ms": {"median": t_all[0], "min": t_all[1], "max": t_all[2]},
               "eager_ms": {"median": t_eager[0], "min": t_eager[1], "max": t_eager[2]},
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "algorithmic_bytes": byts, "algorithmic_flops": flops,
               "fused_stack_TBps": byts / t_stack[0] * 1e-9, "fused_stack_TFLOPs": flops / t_stack[0] * 1e-9,
               "max_rel_diff_of_stacks": rel, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
        del trans, ivar, tbar, stack, est
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(ln + "\n")


if __name__ == "__main__":
    main()
