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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, floor_ms, inputs, ms, time_ms, write  # noqa: E402


def main():
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
        c = inputs(spec, a.nz, dev, trans_lo=-0.05, ivar_of=lambda u: torch.exp(u * 6.0))
        B, nb, nseg, S, L, nz, min_used, trans, ivar, tbar = c.B, c.nb, c.nseg, c.S, c.L, c.nz, c.min_used, c.trans, c.ivar, c.tbar
        kT, okT, okz, row, z0, dz = c.kT, c.okT, c.okz, c.row, c.z0, c.dz
        # (ivar over 2.6 decades: v spreads over some 9 octaves)
        m = QFA(nb, 8, 8 if nb < 1000 else 16, dev)
        stack = VarianceStack.zeros(S, z0, dz, nz, L, a.e_lo, a.n_oct, a.sub, None, dev)
        kw = dict(c.kw, e_lo=a.e_lo, n_oct=a.n_oct, sub=a.sub)

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
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nv": nv, "e_lo": a.e_lo, "sub": a.sub,
                         "min_used": min_used},
               "fused_stack_ms": ms(t_stack),
               "fused_stack_and_moments_ms": ms(t_all),
               "eager_ms": ms(t_eager),
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "counts_equal": counts_equal, "counted_fraction": float(sums[0].sum().item() / max(1.0, head[:, 1].sum().item())),
               "occupied_bins": int((sums[0].reshape(S * nz, nv).sum(0) > 0).sum().item()),
               "bytes_read": nsegs * L * 8, "floor_ms_at_4TBs": floor_ms(nsegs, L),
               "fraction_of_floor": floor_ms(nsegs, L) / t_stack[0], "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        write(a.out, rec)
        del c, stack, head, sums, trans, ivar, tbar
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
