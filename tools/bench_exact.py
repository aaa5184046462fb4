"""Timing of the exact gradient mode (QFA.exact_gradients, include/qfa_hip.h QFA_F_EXACT_GRAD) against the reference mode
(not the flagship benchmark: that is bench.py, which times the reference mode).  For each shape, bench.py's inputs (same
seeds, the factored-z input form of its headline), the two modes interleaved in rounds on one model: the median training
step (forward + fused finalize / Adam / clip) and the median stages {pass 1 incl. images, solve, pass 2} from the
library's events.  One JSON line per shape and mode.

    python tools/bench_exact.py [--configs c3 c2 c5 desi] [--steps 20] [--rounds 3]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import numpy as np
    import torch
    import bench
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["c3", "c2", "c5", "desi"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfg in a.configs:
        B, npix, nh, masks, _ = bench.CONFIGS[cfg]
        wav, nb, nr = synthetic.desi_grid() if cfg == "desi" else synthetic.wavelength_grid(npix)
        npix = len(wav)
        params, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
        parts = []
        for i, s0 in enumerate(range(0, B, 25000)):
            parts.append(synthetic.make_batch_torch(params, mu, wav, nb, min(25000, B - s0), 20220700 + 17 * i, dev,
                                                    masks=masks, return_zq=True))
        batch = tuple(torch.cat([p[j] for p in parts]) for j in range(4))
        zfac = ((1.0 + torch.cat([p[4] for p in parts])).contiguous(),
                torch.tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev))
        del parts
        model = QFA(nb, nr, nh, dev, model_params=params)
        opt = Adam(model.parameters, dev, scheduler=step_scheduler(0.9, 10), learning_rate=1e-3, weight_decay=1e-1)
        res = {False: {"step": [], "pass1": [], "solve": [], "pass2": []}, True: None}
        res[True] = {k: [] for k in res[False]}

        def step(ev=None):
            model.step(opt, batch[0], batch[1], None, batch[3], events=ev, zfac=zfac)
        for exact in (False, True):                        # warm-up of both modes
            model.exact_gradients = exact
            for _ in range(5):
                step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for exact in (False, True):
                model.exact_gradients = exact
                for _ in range(a.steps):
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                    for e in ev:                             # (recorded once, so that they exist; the library re-records them)
                        e.record()
                    s0.record()
                    step(ev)
                    s1.record()
                    s1.synchronize()
                    r = res[exact]
                    r["step"].append(s0.elapsed_time(s1))
                    r["pass1"].append(ev[0].elapsed_time(ev[2]))
                    r["solve"].append(ev[2].elapsed_time(ev[3]))
                    r["pass2"].append(ev[3].elapsed_time(ev[4]))
        for exact in (False, True):
            med = {k: round(float(np.median(v)), 4) for k, v in res[exact].items()}
            print(json.dumps({"config": cfg, "B": B, "Npix": npix, "Nh": nh, "mode": "exact" if exact else "reference",
                              "ms_step": med["step"], "ms_pass1": med["pass1"], "ms_solve": med["solve"],
                              "ms_pass2": med["pass2"], "steps": a.steps * a.rounds}), flush=True)
        del batch, zfac, model, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
