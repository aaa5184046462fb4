"""Timing of the variance function and its (v-bin, z) stack (not the flagship benchmark: that is bench.py): the fused call
(QFA.variance_segments, qfa_variance_f32) against the eager composition it replaces, in the same process on the same GPU -- `used`,
delta_F, its noise variance and the bin code formed in torch (B, S, Nb), then ``index_add_`` of 1, v, d, d^2 and d^4 in float64 into
the (draw, z-bin, v-bin) rows (float atomics).  trans / ivar are formed once outside both timings.  One JSON line per shape and S into
profiles/variance_bench.jsonl: median / min / max ms of each form over ``--iters`` calls after a warm-up call (timed as
tools/bench_p1d.py times them), the bytes the call must read (8 per pixel-draw of the segments) and the fraction of the time they
take at 4 TB/s that the fused call reaches.

    python tools/bench_variance.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--e_lo -12] [--n_oct 14] [--sub 1]
                                   [--out profiles/variance_bench.jsonl]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_p1d import time_ms  # noqa: E402

HBM_BYTES_PER_S = 4.0e12                                     # what the project's streaming kernels reach


def main():
    import numpy as np
    import torch
    from qfa_amd import QFA
    from qfa_amd.model import VarianceStack
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:720:3:100", "4096:2000:3:1", "4096:2000:3:100"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--e_lo", type=int, default=-12)
    ap.add_argument("--n_oct", type=int, default=14)
    ap.add_argument("--sub", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "variance_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nv, c0 = a.n_oct << a.sub, (a.e_lo + 127) << a.sub
    for spec in a.shapes:
        B, nb, nseg, S = (int(x) for x in spec.split(":"))
        L, nT, nz = nb // nseg, 64, a.nz
        min_used = int(np.ceil(0.75 * L))
        m = QFA(nb, 8, 8 if nb < 1000 else 16, dev)
        torch.manual_seed(0)
        trans = torch.rand((B, S, nb), device=dev) * 1.2 - 0.05
        ivar = torch.exp(torch.rand((B, S, nb), device=dev) * 6.0)       # ivar over 2.6 decades: v spreads over some 9 octaves
        ivar.mul_(torch.rand((B, S, nb), device=dev) > 0.2)               # 20 % unused pixels: segments on both sides of min_used
        zq1 = (3.0 + 1.5 * torch.rand(B, device=dev)).contiguous()
        ratio = torch.tensor((10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32), device=dev)
        zabs = (zq1[:, None] * ratio[None, :] - 1.0).contiguous()
        zT0, dzT = np.float32(1.5), np.float32(2.1 / nT)
        z0, dz = np.float32(1.6), np.float32(1.8 / nz)
        tbar = (0.3 + 0.6 * torch.rand((S, nT), device=dev)).contiguous()
        kT = torch.floor((zabs - zT0) * (np.float32(1.0) / dzT)).long()
        okT = (kT >= 0) & (kT < nT)
        kT.clamp_(0, nT - 1)
        zc = zabs[:, torch.arange(nseg, device=dev) * L + L // 2]
        kz = torch.floor((zc - z0) * (np.float32(1.0) / dz)).long()
        okz = (kz >= 0) & (kz < nz)
        row = torch.arange(S, device=dev)[None, :, None] * nz + kz.clamp(0, nz - 1)[:, None, :]     # (B, S, nseg)
        stack = VarianceStack.zeros(S, z0, dz, nz, L, a.e_lo, a.n_oct, a.sub, None, dev)
        kw = dict(zabs=zabs, tbar=tbar, tbar_bins=(zT0, dzT, nT), seg_len=L, n_segments=nseg, min_used=min_used, e_lo=a.e_lo,
                  n_oct=a.n_oct, sub=a.sub)

        def fused_stack():
            stack.buf.zero_()
            m.variance_segments(trans, ivar, stack=stack, **kw)

        def fused_all():
            stack.buf.zero_()
            return m.variance_segments(trans, ivar, stack=stack, return_segments=True, **kw)

        head = torch.zeros((S * nz, 2), dtype=torch.float64, device=dev)
        sums = torch.zeros((5, S * nz * nv), dtype=torch.float64, device=dev)

        def eager():
            head.zero_()
            sums.zero_()
            tb = tbar[:, kT].permute(1, 0, 2)                            # (B, S, Nb)
            used = (ivar > 0) & okT[:, None, :] & (tb > 0)
            d = trans / tb - 1.0
            v = 1.0 / (ivar * (tb * tb))
            c = (v.contiguous().view(torch.int32) >> (23 - a.sub)) - c0
            seg = lambda t: t[..., :nseg * L].reshape(B, S, nseg, L)
            nused = seg(used).sum(-1)
            ok = (nused >= min_used) & okz[:, None, :]
            cs = seg(c)
            counted = seg(used) & ok[..., None] & (cs >= 0) & (cs < nv) & torch.isfinite(seg(d))
            idx = (row[..., None] * nv + cs.clamp(0, nv - 1))[counted]
            dd, vv = seg(d)[counted].double(), seg(v)[counted].double()
            d2 = dd * dd
            sums[0].index_add_(0, idx, torch.ones_like(dd))
            sums[1].index_add_(0, idx, vv)
            sums[2].index_add_(0, idx, dd)
            sums[3].index_add_(0, idx, d2)
            sums[4].index_add_(0, idx, d2 * d2)
            head.index_add_(0, row[ok], torch.stack([torch.ones_like(nused[ok]), nused[ok]], -1).double())

        nsegs = B * S * nseg
        t_stack, t_all = time_ms(fused_stack, a.iters), time_ms(fused_all, a.iters)
        t_eager = time_ms(eager, a.iters)
        fused_stack()
        eager()
        torch.cuda.synchronize()
        got = stack.buf[:, :, 2:].reshape(S, nz, 5, nv).permute(2, 0, 1, 3).reshape(5, -1)
        # (the eager v and d are torch's float32 arithmetic, not the contract's: a pixel on a bin edge may differ, so the counts are
        # compared as totals and the equality is recorded, not required)
        assert torch.equal(stack.buf[:, :, :2].reshape(-1, 2), head), "n_seg / n_used differ"
        counts_equal = bool(torch.equal(got[0], sums[0]))
        assert abs(got[0].sum().item() - sums[0].sum().item()) <= 1e-6 * sums[0].sum().item(), "the counted pixels differ"
        assert torch.allclose(got.reshape(5, S * nz, nv).sum(-1), sums.reshape(5, S * nz, nv).sum(-1), rtol=1e-5, atol=0.0), "the sums differ"
        floor_ms = nsegs * L * 8 / HBM_BYTES_PER_S * 1e3
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nv": nv, "e_lo": a.e_lo, "sub": a.sub,
                         "min_used": min_used},
               "fused_stack_ms": {"median": t_stack[0], "min": t_stack[1], "max": t_stack[2]},
               "fused_stack_and_moments_ms": {"median": t_all[0], "min": t_all[1], "max": t_all[2]},
               "eager_ms": {"median": t_eager[0], "min": t_eager[1], "max": t_eager[2]},
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "counts_equal": counts_equal, "counted_fraction": float(sums[0].sum().item() / max(1.0, head[:, 1].sum().item())),
               "occupied_bins": int((sums[0].reshape(S * nz, nv).sum(0) > 0).sum().item()),
               "bytes_read": nsegs * L * 8, "floor_ms_at_4TBs": floor_ms,
               "fraction_of_floor": floor_ms / t_stack[0], "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:                                        # (line by line: a later shape may not fit the device)
            f.write(json.dumps(rec) + "\n")
        del stack, head, sums, trans, ivar, tbar
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
