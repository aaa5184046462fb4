"""Timing of the flux PDF and its covariance stack (not the flagship benchmark: that is bench.py): the fused call
(QFA.flux_pdf_segments, qfa_flux_pdf_f32) against the eager composition it replaces, in the same process on the same GPU -- `used`
and the bins formed in torch (B, S, Nb), ``scatter_add_`` into per-segment histograms, ``einsum`` for the outer products, then
``index_add_`` of [1 | n_cnt | h | h h^T] in float64 into the (draw, z-bin) rows (float atomics; exact all the same, the terms being
integers).  trans / ivar are formed once outside both timings.  One JSON line per shape and S into profiles/pdf_bench.jsonl: median
/ min / max ms of each form over ``--iters`` calls after a warm-up call (timed as tools/bench_p1d.py times them), the bytes the call
must read (8 per pixel-draw of the segments) and the fraction of the time they take at 4 TB/s that the fused call reaches.

    python tools/bench_pdf.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--nt 20] [--out profiles/pdf_bench.jsonl]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, floor_ms, inputs, ms, time_ms, write  # noqa: E402


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
        c = inputs(spec, a.nz, dev, trans_lo=-0.05)
        B, nb, nseg, S, L, nz, min_used, trans, ivar, tbar = c.B, c.nb, c.nseg, c.S, c.L, c.nz, c.min_used, c.trans, c.ivar, c.tbar
        kT, okT, okz, row, z0, dz = c.kT, c.okT, c.okz, c.row, c.z0, c.dz
        nt = a.nt                                                      # (trans a few per cent below 0 and above 1: the clamp has work)
        m = QFA(nb, 8, 8 if nb < 1000 else 16, dev)
        t0, dt = np.float32(0.0), np.float32(1.0 / nt)
        stack = PDFStack.zeros(S, z0, dz, nz, L, t0, dt, nt, False, True, 0.0, dev)
        kw = dict(c.kw, t_min=0.0, t_max=1.0, n_tbins=nt, clamp=True)

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
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nt": nt, "min_used": min_used},
               "fused_stack_ms": ms(t_stack),
               "fused_stack_and_hist_ms": ms(t_all),
               "eager_ms": ms(t_eager),
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "stacks_equal": True, "bytes_read": nsegs * L * 8, "floor_ms_at_4TBs": floor_ms(nsegs, L),
               "fraction_of_floor": floor_ms(nsegs, L) / t_stack[0], "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        write(a.out, rec)
        del c, stack, est, trans, ivar, tbar
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
