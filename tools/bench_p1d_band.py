"""Timing of the band powers of the P1D and their covariance stack (not the flagship benchmark: that is bench.py), three forms in the
same process on the same GPU, whole-call medians as tools/bench_p1d.py takes them:

  (a) ``QFA.p1d``, stack only: what the diagonal-only statistic costs
  (b) ``QFA.p1d_bands``, stack only (qfa_p1d_band_f32)
  (c) the eager composition (b) replaces: ``p1d(return_segments=True)``, a matmul with the (M, nband) band matrix, outer products
      and ``index_add_`` of [1 | Q | Q Q^T] in float64 into the (draw, z-bin) rows (float atomics)

One JSON line per shape and S into profiles/p1d_band_bench.jsonl: median / min / max ms of each form over ``--iters`` calls after a
warm-up call, and (b) - (a), what the band reduction adds to the call.

    python tools/bench_p1d_band.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--nband 35] [--out profiles/p1d_band_bench.jsonl]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, inputs, ms, time_ms, write  # noqa: E402


def main():
    import torch
    from qfa_amd import QFA
    from qfa_amd.model import P1DBandStack, P1DStack
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:720:3:100", "4096:2000:3:1", "4096:2000:3:100"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--nband", type=int, default=35)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "p1d_band_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in a.shapes:
        c = inputs(spec, a.nz, dev)
        B, nb, nseg, S, L, nz, min_used, trans, ivar, tbar = c.B, c.nb, c.nseg, c.S, c.L, c.nz, c.min_used, c.trans, c.ivar, c.tbar
        okz, row, z0, dz = c.okz, c.row, c.z0, c.dz
        nband, dv, M = a.nband, 69.0, L // 2
        m = QFA(nb, 8, 4, dev)
        edges = P1DBandStack.linear_k_edges(L, dv, nband)
        stack = P1DStack.zeros(S, z0, dz, nz, L, dv, dev)
        bstack = P1DBandStack.zeros(S, z0, dz, nz, L, dv, edges, dev)
        kw = c.kw

        def p1d_stack():
            stack.buf.zero_()
            m.p1d(trans, ivar, stack=stack, return_segments=False, **kw)

        def band_stack():
            bstack.buf.zero_()
            m.p1d_bands(trans, ivar, stack=bstack, k_edges=edges, **kw)

        band, weight = m._p1d_band_tables(L, dv, edges, None)
        A = torch.zeros((M, nband), dtype=torch.float64, device=dev)       # Q = (P - N) A
        idx = torch.arange(M, device=dev)
        A[idx, band[:M].long().clamp_min(0)] = torch.where(band[:M] >= 0, weight[:M].double(), torch.zeros((), dtype=torch.float64, device=dev))
        est = torch.zeros_like(bstack.buf)

        def eager():
            est.zero_()
            P, N, _ = m.p1d(trans, ivar, return_segments=True, **kw)
            ok = (N > 0) & okz[:, None, :]
            Q = (P.double() - N.double()[..., None])[ok] @ A                # (hits, nband)
            terms = torch.cat([torch.ones_like(Q[:, :1]), Q, (Q[:, :, None] * Q[:, None, :]).reshape(Q.shape[0], -1)], -1)
            est.view(S * nz, -1).index_add_(0, row[ok], terms)

        t_a, t_b, t_c = time_ms(p1d_stack, a.iters), time_ms(band_stack, a.iters), time_ms(eager, a.iters)
        band_stack()
        eager()
        torch.cuda.synchronize()
        assert torch.equal(bstack.n, est[:, :, 0]), "counts differ"
        scale = est.abs().amax(-1, keepdim=True).clamp_min(1e-300)
        rel = float(((bstack.buf - est).abs() / scale).max())
        rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nband": nband, "min_used": min_used},
               "p1d_stack_ms": ms(t_a),
               "band_stack_ms": ms(t_b),
               "eager_ms": ms(t_c),
               "band_minus_p1d_ms": t_b[0] - t_a[0], "band_minus_p1d_over_p1d": (t_b[0] - t_a[0]) / t_a[0],
               "eager_over_band": t_c[0] / t_b[0], "max_diff_of_stacks_over_row_max": rel, "iters": a.iters,
               "device": torch.cuda.get_device_name(0)}
        write(a.out, rec)
        del c, trans, ivar, tbar, stack, bstack, est
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
