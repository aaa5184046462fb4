"""Timing of the 1D flux power spectrum and its stack (not the flagship benchmark: that is bench.py): the fused call (QFA.p1d,
qfa_p1d_f32) against the eager composition it replaces, in the same process on the same GPU -- delta_F and the noise variance
materialised (B, S, Nb), ``torch.fft.rfft`` per segment, |X|^2 / L, then ``index_add_`` of [1 | N | P | P^2] in float64 into the
(draw, z-bin) rows (float atomics).  trans / ivar are formed once outside both timings.  One JSON line per shape and S into
profiles/p1d_bench.jsonl: median / min / max ms of each form over ``--iters`` calls after a warm-up call, the fused call's
algorithmic bytes and flops, and the rates they give.

    python tools/bench_p1d.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--out profiles/p1d_bench.jsonl]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, inputs, ms, time_ms, write  # noqa: E402


def main():
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
    for spec in a.shapes:
        c = inputs(spec, a.nz, dev)
        B, nb, nseg, S, L, nz, min_used, trans, ivar, tbar = c.B, c.nb, c.nseg, c.S, c.L, c.nz, c.min_used, c.trans, c.ivar, c.tbar
        kT, okT, okz, row, z0, dz = c.kT, c.okT, c.okz, c.row, c.z0, c.dz
        M = L // 2
        m = QFA(nb, 8, 4, dev)
        stack = P1DStack.zeros(S, z0, dz, nz, L, 69.0, dev)
        kw = c.kw

        def fused_stack():
            stack.buf.zero_()
            m.p1d(trans, ivar, stack=stack, return_segments=False, **kw)

        def fused_all():
            stack.buf.zero_()
            return m.p1d(trans, ivar, stack=stack, **kw)

        est = torch.zeros_like(stack.buf)

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
               "fused_stack_ms": ms(t_stack),
               "fused_stack_and_segments_ms": ms(t_all),
               "eager_ms": ms(t_eager),
               "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
               "algorithmic_bytes": byts, "algorithmic_flops": flops,
               "fused_stack_TBps": byts / t_stack[0] * 1e-9, "fused_stack_TFLOPs": flops / t_stack[0] * 1e-9,
               "max_rel_diff_of_stacks": rel, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
        write(a.out, rec)
        del c, trans, ivar, tbar, stack, est
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
