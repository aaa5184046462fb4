"""Timing of the closed-form EM update of F (QFA.em_statistics / em_update_F; include/qfa_hip.h qfa_em_*) beside the training
step of the same batch (not the flagship benchmark: that is bench.py).  For each shape, bench.py's inputs (same seeds, the
factored-z input form of its headline), interleaved in rounds in one process: the medians of em_statistics, em_update_F and
QFA.step, and em_statistics against the HBM floor of reading the spectra once more (bytes / 6.29 TB/s measured copy rate).
The stages inside em_statistics (pass 1, solve, k_em_record, k_em_stats, k_em_reduce) are kernels of one stream: take them
from `rocprofv3 --kernel-trace --stats -- python tools/bench_em.py --configs c3`.  `--converge` adds the convergence leg:
epochs and wall time of train(f_update="em") and of the default loop to reach the same mean NLL on one resident data set.
One JSON line per shape, appended to profiles/em_bench.jsonl.

    python tools/bench_em.py [--configs c2 c3 desi c5] [--steps 20] [--rounds 3] [--converge]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_RATE = 6.29e12


def timed(fn, n):
    import torch
    out = []
    for _ in range(n):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        fn()
        s1.record()
        s1.synchronize()
        out.append(s0.elapsed_time(s1))
    return out


def converge(dev, out):
    import numpy as np
    import torch
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    from qfa_amd.dataloader import DeviceDataloader
    npix, nh, N, bs = 2000, 8, 20000, 2000
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=20220700)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, N, seed=20220701)
    res = {}
    for mode in ("em", "adam"):
        torch.manual_seed(1)
        dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, bs, dev, shuffle=False)
        m = QFA(nb, nr, nh, dev)
        opt = Adam(m.parameters, dev, scheduler=step_scheduler(0.9, 10), learning_rate=1e-2, weight_decay=1e-3)
        hist, t0 = [], time.time()

        class Log:
            def info(self, msg):
                hist.append((float(msg.split("loss:")[1].split(";")[0]), time.time() - t0))
        m.train(opt, dl, 30, output_dir=os.path.join(REPO, "bench_out", "em_converge"), quiet=True, logger=Log(),
                smooth_interval=1000, save_interval=1000, f_update=mode)
        res[mode] = hist
    target = min(l for l, _ in res["adam"])
    line = {"leg": "convergence", "Npix": npix, "Nh": nh, "N": N, "batch": bs, "target_mean_nll": target}
    for mode in ("em", "adam"):
        hit = [(i + 1, t) for i, (l, t) in enumerate(res[mode]) if l <= target]
        line[mode + "_epochs"], line[mode + "_seconds"] = hit[0] if hit else (None, None)
        line[mode + "_final"] = res[mode][-1][0]
    out(line)


def main():
    import numpy as np
    import torch
    import bench
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["c2", "c3", "desi", "c5"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--converge", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    log = open(os.path.join(REPO, "profiles", "em_bench.jsonl"), "a")

    def out(line):
        print(json.dumps(line), flush=True)
        log.write(json.dumps(line) + "\n")
        log.flush()
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
        st = model.em_statistics(batch[0], batch[1], None, batch[3], zfac=zfac)
        F0 = model.F.clone()
        fns = {"em_statistics": lambda: model.em_statistics(batch[0], batch[1], None, batch[3], zfac=zfac, stats=st),
               "em_update_F": lambda: model._em_update(st, 0.0, 0.0),          # damping 0: F stays where it is
               "step": lambda: model.step(opt, batch[0], batch[1], None, batch[3], zfac=zfac)}
        for f in fns.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                res[k] += timed(f, a.steps)
        med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
        floor = B * (npix * 9 + 4) / COPY_RATE * 1e3                           # delta, error (4 B), mask (1 B), zq1
        out({"config": cfg, "B": B, "Npix": npix, "Nh": nh, "ms_em_statistics": med["em_statistics"],
             "ms_em_update_F": med["em_update_F"], "ms_step": med["step"], "ms_hbm_floor_spectra_once": round(floor, 4),
             "steps": a.steps * a.rounds})
        del batch, zfac, model, opt, st, F0
        torch.cuda.empty_cache()
    if a.converge:
        converge(dev, out)


if __name__ == "__main__":
    main()
