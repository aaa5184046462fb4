"""Timing of the line-of-sight correlation function and its stack (not the flagship benchmark: that is bench.py): the fused call
(QFA.xi, qfa_xi_f32) against the eager composition it replaces, in the same process on the same GPU -- delta_F, the weights and
x = w delta_F materialised (B, S, Nb), the autocorrelation of x and of w per segment by a zero-padded ``torch.fft.rfft`` /
``irfft`` pair, then ``index_add_`` of [1 | N0 | W | A | W^2 | A W | A^2] in float64 into the (draw, z-bin) rows (float atomics).
trans / ivar are formed once outside both timings.  One JSON line per shape, S and nlag into profiles/xi_bench.jsonl: median / min /
max ms of each form over ``--iters`` calls after a warm-up call (timed as tools/bench_p1d.py times them), the fused call's
algorithmic flops and the rate they give.

    python tools/bench_xi.py [--shapes B:Nb:nseg:S ...] [--iters 7] [--nz 8] [--out profiles/xi_bench.jsonl]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _segment_bench import REPO, inputs, ms, time_ms, write  # noqa: E402


def main():
    import torch
    from qfa_amd import QFA
    from qfa_amd.model import XiStack
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096:720:3:1", "4096:720:3:100", "4096:2000:3:1", "4096:2000:3:100"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--sigma2", type=float, default=0.05)
    ap.add_argument("--eager_bytes", type=float, default=200e9, help="skip the eager form when its arrays would pass this")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "xi_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in a.shapes:
        c = inputs(spec, a.nz, dev)
        B, nb, nseg, S, L, nz, min_used, trans, ivar, tbar = c.B, c.nb, c.nseg, c.S, c.L, c.nz, c.min_used, c.trans, c.ivar, c.tbar
        kT, okT, okz, row, z0, dz = c.kT, c.okT, c.okz, c.row, c.z0, c.dz
        m = QFA(nb, 8, 4, dev)
        for nlag in sorted({min(64, L), L // 2}):
            stack = XiStack.zeros(S, z0, dz, nz, L, nlag, 69.0, dev)
            kw = dict(c.kw, n_lags=nlag, sigma2_lss=a.sigma2)

            def fused_stack():
                stack.buf.zero_()
                m.xi(trans, ivar, stack=stack, return_segments=False, **kw)

            def fused_all():
                stack.buf.zero_()
                return m.xi(trans, ivar, stack=stack, **kw)

            est = torch.zeros_like(stack.buf)
            s2 = torch.tensor(a.sigma2, dtype=torch.float32, device=dev)

            def eager():
                est.zero_()
                tb = tbar[:, kT].permute(1, 0, 2)                            # (B, S, Nb)
                used = (ivar > 0) & okT[:, None, :] & (tb > 0)
                zero = torch.zeros((), device=dev)
                d = torch.where(used, trans / tb - 1.0, zero)
                v = torch.where(used, 1.0 / (ivar * (tb * tb)), zero)
                wv = 1.0 / (v + s2)
                w = torch.where(used & torch.isfinite(wv), wv, zero)
                seg = lambda t: t[..., :nseg * L].reshape(B, S, nseg, L)
                w, x, v = seg(w), seg(w * d), seg(v)
                N0 = ((w * w) * v).sum(-1)
                fx, fw = torch.fft.rfft(x, 2 * L, dim=-1), torch.fft.rfft(w, 2 * L, dim=-1)
                A = torch.fft.irfft(fx.real * fx.real + fx.imag * fx.imag, 2 * L, dim=-1)[..., :nlag]
                W = torch.fft.irfft(fw.real * fw.real + fw.imag * fw.imag, 2 * L, dim=-1)[..., :nlag]
                ok = (seg(used).sum(-1) >= min_used) & okz[:, None, :]
                Wd, Ad = W.double(), A.double()
                terms = torch.cat([torch.ones_like(N0, dtype=torch.float64)[..., None], N0.double()[..., None], Wd, Ad, Wd * Wd,
                                   Ad * Wd, Ad * Ad], -1)
                est.view(S * nz, 2 + 5 * nlag).index_add_(0, row[ok], terms[ok])
                return W, A

            nsegs = B * S * nseg
            # the eager form holds a dozen (B, S, Nb) float32 arrays, two complex spectra of 2L and the float64 terms
            eager_bytes = nsegs * (12 * 4 * L + 2 * 8 * (L + 1) + 2 * 4 * 2 * L + 2 * 8 * (2 + 5 * nlag))
            t_stack, t_all = time_ms(fused_stack, a.iters), time_ms(fused_all, a.iters)
            rec = {"shape": {"B": B, "Nb": nb, "nseg": nseg, "L": L, "S": S, "nz": nz, "nlag": nlag, "min_used": min_used},
                   "fused_stack_ms": ms(t_stack),
                   "fused_stack_and_segments_ms": ms(t_all)}
            if eager_bytes <= a.eager_bytes:
                t_eager = time_ms(eager, a.iters)
                fused_stack()
                eager()
                torch.cuda.synchronize()
                assert torch.equal(stack.n, est[:, :, 0]), "counts differ"
                # the FFT's error is absolute, of the size of lag 0: compare against the row's largest entry of the same kind
                scale = torch.cat([stack.buf[:, :, :2].abs()] + [stack.buf[:, :, 2 + i * nlag:2 + (i + 1) * nlag].abs().amax(-1, keepdim=True)
                                                                 .expand(-1, -1, nlag) for i in range(5)], -1)
                rel = float(((stack.buf - est).abs() / scale.clamp_min(1e-300))[scale > 0].max())
                rec.update({"eager_ms": ms(t_eager),
                            "eager_over_fused_stack": t_eager[0] / t_stack[0], "eager_over_fused_all": t_eager[0] / t_all[0],
                            "max_diff_of_stacks_over_lag0": rel})
            else:
                rec["eager_ms"] = None
                rec["eager_skipped"] = f"its arrays would take {eager_bytes / 1e9:.0f} GB"
            # counted: 2 (W and A) x nlag x (L - (nlag - 1) / 2) multiply-adds per segment (pairs inside the segment only)
            flops = nsegs * 2 * 2 * nlag * (L - (nlag - 1) / 2.0)
            rec.update({"algorithmic_flops": flops, "fused_stack_TFLOPs": flops / t_stack[0] * 1e-9, "iters": a.iters,
                        "device": torch.cuda.get_device_name(0)})
            write(a.out, rec)
            del stack, est
            torch.cuda.empty_cache()
        del c, trans, ivar, tbar
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
