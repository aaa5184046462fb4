"""Timing of the flux PDF and its covariance stack (not the flagship benchmark: that is bench.py): the fused call
(QFA.flux_pdf_segments, qfa_flux_pdf_f32) against the eager composition it replaces, in the same process on the same GPU -- `used`
and the bins formed in torch (B, S, Nb), ``scatter_add_`` into per-segment histograms, ``einsum`` for the outer products, then
``index_add_`` of [1 | n_cnt | h | h h^T] in float64 into the (draw, z-bin) rows (float atomics; exact all the same, the terms being
integers).  trans / ivar are formed once outside both timings.  One JSON line per shape and S into profiles/pdf_bench.jsonl: median
/ min / max ms of each form over ``--iters`` calls after a warm-up call (timed as tools/bench_p1d.py times them), the bytes the call
must read (8 per pixel-draw of the segments) and the fraction of the time they take at 4 TB/s that the fused call reaches.

    python tools/bench_pdf.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--nt 20] [--out profiles/pdf_bench.jsonl]"""
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
    from qfa_amd.model import PDFStack
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:720:3:100", "4096:2000:3:1", "4096:2000:3:100"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--nt", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pdf_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in a.shapes:
        B, nb, nseg, S = (int(x) for x in spec.split(":"))
        L, nT, nz, nt = nb // nseg, 64, a.nz, a.nt
        min_used = int(np.ceil(0.75 * L))
        m = QFA(nb, 8, 8 if nb < 1000 else 16, dev)
        torch.manual_seed(0)
        trans = torch.rand((B, S, nb), device=dev) * 1.2 - 0.05       # a few per cent below 0 and above 1: the clamp has work
        ivar = 10.0 + 90.0 * torch.rand((B, S, nb), device=dev)
        ivar.mul_(torch.rand((B, S, nb), device=dev) > 0.2)               # 20 % unused pixels: segments on both sides of min_used
        zq1 = (3.0 + 1.5 * torch.rand(B, device=dev)).contiguous()
        ratio = torch.tensor((10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32), device=dev)
        zabs = (zq1[:, None] * ratio[None, :] - 1.0).contiguous()
        zT0, dzT = np.float32(1.5), np.float32(2.1 / nT)
        z0, dz = np.float32(1.6), np.float32(1.8 / nz)
        t0, dt = np.float32(0.0), np.float32(1.0 / nt)
        tbar = (0.3 + 0.6 * torch.rand((S, nT), device=dev)).contiguous()
        kT = torch.floor((zabs - zT0) * (np.float32(1.0) / dzT)).long()
        okT = (kT >= 0) & (kT < nT)
        kT.clamp_(0, nT - 1)
        zc = zabs[:, torch.arange(nseg, device=dev) * L + L // 2]
        kz = torch.floor((zc - z0) * (np.float32(1.0) / dz)).long()
        okz = (kz >= 0) & (kz < nz)
        row = torch.arange(S, device=dev)[None, :, None] * nz + kz.clamp(0, nz - 1)[:, None, :]     # (B, S, nseg)
        stack = PDFStack.zeros(S, z0, dz, nz, L, t0, dt, nt, False, True, 0.0, dev)
        kw = dict(zabs=zabs, tbar=tbar, tbar_bins=(zT0, dzT, nT), seg_len=L, n_segments=nseg, min_used=min_used, t_min=0.0, t_max=1.0,
                  n_tbins=nt, clamp=True)

        def fused_stack():
            stack.buf.zero_()
            m.flux_pdf_segments(trans, ivar, stack=stack, return_segments=False, **kw)

        def fused_all():
            stack.buf.zero_()
            return m.flux_pdf_segments(trans, ivar, stack=stack, **kw)

        est = torch.zeros_like(stack.buf)
        inv_dt = np.float32(1.0) / dt

        def eager():
            est.zero_()
            tb = tbar[:, kT].permute(1, 0, 2)                            # (B, S, Nb)
            used = (ivar > 0) & okT[:, None, :] & (tb > 0)
            fa = torch.floor((trans - t0) * inv_dt)
            inbin = used & ~torch.isnan(fa)
            k = fa.clamp(0, nt - 1).long()                               # (the clamp convention)
            seg = lambda t: t[..., :nseg * L].reshape(B, S, nseg, L)
            hist = torch.zeros((B, S, nseg, nt), dtype=torch.float64, device=dev)
            hist.scatter_add_(-1, seg(k), seg(inbin).double())
            nused = seg(used).sum(-1)
            ok = (nused >= min_used) & okz[:, None, :]
            outer = torch.einsum("bsga,bsgc->bsgac", hist, hist).reshape(B, S, nseg, nt * nt)
            one = torch.ones((B, S, nseg, 1), dtype=torch.float64, device=dev)
            terms = torch.cat([one, nused.double()[..., None], hist, outer], -1)
            est.view(S * nz, 2 + nt + nt * nt).index_add_(0, row[ok], terms[ok])
            return hist

        nsegs = B * S * nseg
        t_stack, t_all = time_ms(fused_stack, a.iters), time_ms(fused_all, a.iters)
        t_eager = time_ms(eager, a.iters)
        fused_stack()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(stack.buf, est), "the stacks differ"
        floor_ms = nsegs * L * 8 / HBM_BYTES_PER_S * 1e3
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nt": nt, "min_used": min_used},
               "fused_stack_ms": {"median": t_stack[0], "min": t_stack[1], "max": t_stack[2]},
               "fused_stack_and_hist_ms": {"median": t_all[0], "min": t_all[1], "max": t_all[2]},
               "eager_ms": {"median": t_eager[0], "min": t_eager[1], "max": t_eager[2]},
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "stacks_equal": True, "bytes_read": nsegs * L * 8, "floor_ms_at_4TBs": floor_ms,
               "fraction_of_floor": floor_ms / t_stack[0], "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:                                        # (line by line: a later shape may not fit the device)
            f.write(json.dumps(rec) + "\n")
        del stack, est, trans, ivar, tbar
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
