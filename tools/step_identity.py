#!/usr/bin/env python3
"""Bit identity and launch identity of the training step, the posterior call and the E-step between two builds of the library (same ABI).

    python tools/step_identity.py PARENT.so RESULT.so [--out FILE] [--traces FILE] [--timeout S] [--keep DIR]

Each library runs the same seeded cases twice (runs A and B), every run in a child process of its own with a time limit; the first child
that does not exit 0 ends the tool with its status.  A child writes every output tensor of every case into one file; the parent process
compares the four files bytewise, tensor by tensor, for the pairs parent A / parent B, result A / result B, parent A / result A, parent B /
result B, and prints the table (profiles/step_plan_identity.txt was made with it).  With --traces, each library additionally runs one
training step per branch of the step's plan under `rocprofv3 --kernel-trace` (one child each, no counters), and the two traces are
compared launch by launch: kernel name (modulo --rename), order, grid, workgroup and LDS sizes.

Cases (small: a few milliseconds each): N_h x N_pix x N_b in {0, N_pix, inside a tile} x B, every pass-2 form the flags can force, reference
and exact gradients, with and without the deterministic slab, the four input forms; the shapes on both sides of the thresholds of the
default form selection; the posterior call with both writers; the E-step.

    python tools/step_identity.py --child LIB OUT {cases|trace}       (what the children run)
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = (1, 8, 9, 16, 17, 32)
NPIX_NB = {33: 13, 97: 45, 200: 77}            # N_pix -> the N_b with the blue / red boundary inside a tile
ALIGNED = (64, 29)                             # (N_pix, N_b) with rows that start on a 64-byte boundary: the aligned store form of the N_h <= 8 writer
BS = (1, 17, 65, 130)
FORMS = ("zabs", "zfac", "rows", "ablue")
# (B, N_pix, N_h) at flags 0: both sides of the pixel-resident thresholds (128 spectra at KP = 16 and 512 at KP = 8 from 1024 pixels on) and
# of the batch size up to which the solve sums the NLL itself (2048)
THRESHOLDS = ((127, 1024, 16), (128, 1024, 16), (128, 1023, 16), (511, 1024, 8), (512, 1024, 8), (2048, 33, 8), (2049, 33, 8), (2049, 33, 24))


def custom_tau(z):                               # a callable tau: the library gets exp(-tau) as A_blue
    return 0.0025 * (1.0 + z) ** 3.5


class Bench(object):
    """models and batches of one (N_h, N_pix, N_b), every input form of B of its spectra"""

    def __init__(self, dev, nh, npix, nb, nmax, seed):
        import numpy as np
        import torch
        from qfa_amd import QFA, synthetic
        self.torch, self.dev, self.npix, self.nb = torch, dev, npix, nb
        wav = np.linspace(1216.0 - 180.0 * nb / npix - 1.0, 1216.0 + 300.0 * (npix - nb) / npix + 1.0, npix)
        p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
        self.N = nmax + 7                          # (the resident set holds more rows than any batch takes)
        b = synthetic.make_batch_numpy(p, mu, wav, nb, self.N, seed=1000 + seed, masks=True)
        f32 = torch.float32
        T = lambda x, dt=f32: torch.as_tensor(x, device=dev).to(dt).contiguous()
        self.d, self.e, self.fx, self.mk = T(b["delta"]), T(b["error"]), T(b["flux"]), T(b["mask"], torch.bool)
        self.z = T(b["zabs"]).reshape(self.N, nb)
        self.zq1 = T((1.0 + b["zqso"].astype(np.float64)).astype(np.float32))
        self.ratio = T((wav[:nb] / synthetic.LYA).astype(np.float32))
        self.perm = np.random.default_rng(seed).permutation(self.N)
        self.models = {}
        for name, tau in (("std", None), ("ablue", custom_tau)):
            m = QFA(nb, npix - nb, nh, dev, model_params=p) if tau is None else QFA(nb, npix - nb, nh, dev, tau=tau, model_params=p)
            m.mu = T(mu)
            m.auto_factor_zabs = False
            self.models[name] = m

    def args(self, form, B, flux=False):
        """(model, positional arguments, keyword arguments) of accumulate / predict / em_statistics"""
        torch = self.torch
        from qfa_amd.resident import ResidentBatch
        x = self.fx if flux else self.d
        if form == "rows":
            stride = (self.npix + 31) // 32 * 32

            def pad(t, fill):
                out = torch.full((self.N, stride), fill, dtype=t.dtype, device=self.dev)
                out[:, :self.npix] = t
                return out
            rows = torch.as_tensor(self.perm[:B].astype("int32"), device=self.dev)
            rb = ResidentBatch(pad(self.fx, 3.0e9) if flux else None, pad(self.d, -7.0e9), pad(self.e, float("nan")), pad(self.mk, True),
                               self.zq1, self.ratio, rows, self.npix, self.nb)
            return self.models["std"], (), {"batch": rb}
        if form == "zfac":
            return self.models["std"], (x[:B], self.e[:B], None, self.mk[:B]), {"zfac": (self.zq1[:B], self.ratio)}
        return self.models["ablue" if form == "ablue" else "std"], (x[:B], self.e[:B], self.z[:B].contiguous(), self.mk[:B]), {}


class Sink(object):
    """every tensor of every case, appended to one file; the index goes beside it"""

    def __init__(self, path):
        self.f, self.index, self.path = open(path, "wb"), [], path

    def put(self, case, names, tensors):
        import torch
        flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for t in tensors]).cpu().numpy()
        o = 0
        for n, t in zip(names, tensors):
            self.index.append((case, n, self.f.tell() + 4 * o, 4 * t.numel()))
            o += t.numel()
        self.f.write(flat.tobytes())

    def close(self):
        self.f.close()
        json.dump(self.index, open(self.path + ".json", "w"))


def step_case(bench, sink, case, form, B, flags, exact, slab):
    torch = bench.torch
    m, a, kw = bench.args(form, B)
    m.flags, m.exact_gradients, m.deterministic = flags, bool(exact), bool(slab)
    nll = torch.empty(B, dtype=torch.float32, device=bench.dev)
    acc = m.accumulate(*a, nll=nll, **kw)
    loss, g = m._finalize(acc.clone(), True)
    keys = ("F", "Psi", "omega", "tau0", "c0", "beta")
    sink.put(case, ("accum", "nll", "loss") + tuple("g_" + k for k in keys), [acc, nll, loss] + [g[k] for k in keys])


def run_cases(sink, dev):
    from qfa_amd import _lib
    seed = 0
    for nh in NH:
        flagset = (0, _lib.F_PASS2_F32, _lib.F_PASS2_XDL, _lib.F_PASS2_PIXRES) if nh <= 16 else (0, _lib.F_S3_FAST)
        for npix, mid in NPIX_NB.items():
            for nbname, nb in (("red", 0), ("blue", npix), ("mid", mid)):
                seed += 1
                bench = Bench(dev, nh, npix, nb, max(BS), seed)
                for B in BS:
                    for form in FORMS:
                        tag = f"nh{nh}/npix{npix}/{nbname}/B{B}/{form}"
                        for flags in flagset:
                            for exact in (0, 1):
                                for slab in (0, 1):
                                    step_case(bench, sink, f"step/{tag}/f{flags:#x}/ex{exact}/slab{slab}", form, B, flags, exact, slab)
                        if form == "ablue":
                            continue               # (the posterior call takes the built-in tau models)
                        for flags in (0, _lib.F_PREDICT_F32):
                            m, a, kw = bench.args(form, B, flux=True)
                            m.flags = flags
                            sink.put(f"predict/{tag}/f{flags:#x}", ("ll", "hmean", "hcov", "cont", "unc"), list(m.predict(*a, **kw)))
                if npix == 97 and nbname == "mid":   # the E-step (run_estep), every KP
                    for form in ("zabs", "zfac", "rows"):
                        m, a, kw = bench.args(form, 65)
                        m.flags = 0
                        nll = bench.torch.empty(65, dtype=bench.torch.float32, device=dev)
                        st = m.em_statistics(*a, nll=nll, **kw)
                        sink.put(f"estep/nh{nh}/{form}", ("stats", "nll"), [st.buf, nll])
    for B, npix, nh in THRESHOLDS:
        seed += 1
        bench = Bench(dev, nh, npix, npix // 2 - 3, B, seed)
        for form in ("zabs", "zfac"):
            for exact in (0, 1):
                for slab in (0, 1):
                    step_case(bench, sink, f"threshold/B{B}/npix{npix}/nh{nh}/{form}/ex{exact}/slab{slab}", form, B, 0, exact, slab)
    # the XDL writer of N_h <= 8 with rows of cont / unc that start on a 64-byte boundary (N_pix a multiple of 16): none of the N_pix above
    # is one, so every N_h <= 8 prediction there takes the re-aligned store form
    for nh in (1, 8):
        seed += 1
        bench = Bench(dev, nh, ALIGNED[0], ALIGNED[1], max(BS), seed)
        for B in BS:
            m, a, kw = bench.args("zabs", B, flux=True)
            m.flags = 0
            sink.put(f"predict/nh{nh}/npix{ALIGNED[0]}/mid/B{B}/zabs/f0x0", ("ll", "hmean", "hcov", "cont", "unc"), list(m.predict(*a, **kw)))


def run_trace(dev):
    """one training step per branch of the plan: every pass-2 form and solve flavour, with and without the slab, both NLL-sum forms,
    the separate and the fused preparations, the factored-z form (k_zfac_* / the ZS block range of k_prep_step); a custom tau and exact
    gradients in the default form (the remaining instantiations of k_grads_x and k_s12_x); the posterior call with the XDL writers"""
    import torch
    from qfa_amd import _lib
    for nh in (8, 16, 24):
        bench = Bench(dev, nh, 97, 45, 130, 100 + nh)
        flagset = (0, _lib.F_PASS2_F32, _lib.F_PASS2_XDL, _lib.F_PASS2_PIXRES) if nh <= 16 else (0, _lib.F_S3_FAST)
        for flags in flagset:
            for slab in (0, 1):
                for form in ("zabs", "zfac"):
                    m, a, kw = bench.args(form, 130)
                    m.flags, m.exact_gradients, m.deterministic = flags, False, bool(slab)
                    m.accumulate(*a, **kw)
        for form, exact in (("ablue", 0), ("ablue", 1), ("zabs", 1), ("zfac", 1)):
            m, a, kw = bench.args(form, 130)
            m.flags, m.exact_gradients, m.deterministic = 0, bool(exact), False
            m.accumulate(*a, **kw)
        m, a, kw = bench.args("zabs", 130, flux=True)
        m.flags = 0
        m.predict(*a, **kw)
    bench = Bench(dev, 8, ALIGNED[0], ALIGNED[1], 130, 300)
    m, a, kw = bench.args("zabs", 130, flux=True)
    m.flags = 0
    m.predict(*a, **kw)
    for B, npix, nh in THRESHOLDS:
        bench = Bench(dev, nh, npix, npix // 2 - 3, B, 200)
        for slab in (0, 1):
            m, a, kw = bench.args("zfac", B)
            m.flags, m.exact_gradients, m.deterministic = 0, False, bool(slab)
            m.accumulate(*a, **kw)
    torch.cuda.synchronize()


def child(lib, out, what):
    sys.path.insert(0, ROOT)
    from qfa_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    import torch
    dev = torch.device("cuda:0")
    if what == "trace":
        run_trace(dev)
    else:
        sink = Sink(out)
        run_cases(sink, dev)
        torch.cuda.synchronize()
        sink.close()


def spawn(cmd, limit):
    r = subprocess.run(cmd, timeout=limit)
    if r.returncode != 0:
        print("child failed with status", r.returncode, ":", " ".join(cmd), flush=True)
        sys.exit(r.returncode if r.returncode > 0 else 1)


def load(path):
    return json.load(open(path + ".json")), open(path, "rb").read()


def compare(runs, out):
    pairs = (("parent A", "parent B"), ("result A", "result B"), ("parent A", "result A"), ("parent B", "result B"))
    data = {k: load(p) for k, p in runs.items()}
    index = data["parent A"][0]
    for k in data:
        assert data[k][0] == index, f"{k}: the runs did not record the same cases and sizes"
    groups, differ = {}, {p: [] for p in pairs}
    nz = nan = 0
    import numpy as np
    for case, name, off, nbytes in index:
        g = groups.setdefault(case.split("/")[0] + " " + name, [0, 0, 0])
        same = all(data[a][1][off:off + nbytes] == data[b][1][off:off + nbytes] for a, b in pairs)
        g[0] += 1
        g[1] += nbytes // 4
        g[2] += same
        v = np.frombuffer(data["parent A"][1], np.float32, nbytes // 4, off)
        nz += int(np.count_nonzero(v))
        nan += int(np.isnan(v).sum())
        for p in pairs:
            if data[p[0]][1][off:off + nbytes] != data[p[1]][1][off:off + nbytes]:
                differ[p].append(case + " " + name)
    for k in sorted(groups):
        n, el, same = groups[k]
        print(f"{k:28s} tensors {n:6d}  elements {el:10d}  bytewise identical in all four pairs {same:6d}", file=out)
    print(f"total tensors {len(index)}; non-zero elements {nz}, NaN elements {nan} (run parent A)", file=out)
    # Pass 2 without a slab adds its block sums with float32 atomics in every form but k_grads_t (which always goes through rows): from
    # three blocks of 64 spectra on, the order of the additions is free and a library need not reproduce its own bits.  So the cases are
    # judged by class -- kind, B, slab or not, pixel-resident form forced (f0x40) or not; the threshold shapes also by N_h -- and a class in
    # which the PARENT differs from itself is reported and is no reference.
    def cls(name):
        c = name.split(" ")[0].split("/")
        keep = r"(step|threshold|predict|estep|B\d+|f0x40|slab\d)$" if c[0] != "threshold" else r"(threshold|nh\d+|B\d+|slab\d)$"
        return " ".join(x for x in c if re.match(keep, x))
    total = {}
    for case in sorted({c for c, _, _, _ in index}):
        total[cls(case)] = total.get(cls(case), 0) + 1
    count = {p: {} for p in pairs}
    for p in pairs:
        for case in sorted({d.rsplit(" ", 1)[0] for d in differ[p]}):
            count[p][cls(case)] = count[p].get(cls(case), 0) + 1
    no_ref = set(count[pairs[0]])
    print("\nCases with a differing tensor, per pair of runs:", file=out)
    for p in pairs:
        print(f"  {p[0]} / {p[1]:10s} {len(differ[p]):6d} tensors in {sum(count[p].values())} cases", file=out)
    shown = sorted(set().union(*[set(count[p]) for p in pairs]))
    print("\nClasses with a differing case (cases that differ per pair, in the order above | cases in the class):", file=out)
    for k in shown:
        print(f"  {k:44s} " + " ".join(f"{count[p].get(k, 0):4d}" for p in pairs) + f" | {total[k]:4d}" + ("" if k in no_ref else "   <-- the parent reproduces itself here"), file=out)
    names = sorted({d.rsplit(" ", 1)[1] for p in pairs for d in differ[p]})
    print(f"tensors that differ anywhere: {names}", file=out)
    bad = sum(n for p in pairs for k, n in count[p].items() if k not in no_ref)
    print(f"\nclasses in which the parent does not reproduce itself (no reference): {len(no_ref)} of {len(total)}, {sum(total[k] for k in no_ref)} of {len({c for c, _, _, _ in index})} cases;"
          f" differing cases in the other classes: {bad}", file=out)
    return bad


def trace_rows(d, renames):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(f) == 1, (d, f)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    cols = [c for c in rows[0] if re.search(r"Grid_Size|Workgroup_Size|LDS", c)]
    out = []
    for r in rows:
        n = r["Kernel_Name"]
        for pat, rep in renames:
            n = re.sub(pat, rep, n)
        out.append(n + "  " + " ".join(f"{c}={r[c]}" for c in cols))
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(*sys.argv[2:5])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("--out", default=None, help="the identity table (default: stdout)")
    ap.add_argument("--traces", default=None, help="also compare kernel traces; the diff goes to this file")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="applied to the parent's kernel names")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--keep", default=None, help="directory for the children's files (default: a temporary one)")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="step_identity_")
    os.makedirs(tmp, exist_ok=True)
    me = os.path.abspath(__file__)
    runs = {}
    for run in ("A", "B"):
        for who, lib in (("parent", a.parent), ("result", a.result)):
            runs[f"{who} {run}"] = os.path.join(tmp, f"{who}_{run}.bin")
            spawn([sys.executable, me, "--child", lib, runs[f"{who} {run}"], "cases"], a.timeout)
    out = open(a.out, "w") if a.out else sys.stdout
    bad = compare(runs, out)
    if a.traces:
        import difflib
        rows = {}
        for who, lib in (("parent", a.parent), ("result", a.result)):
            d = os.path.join(tmp, "trace_" + who)
            spawn(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, me, "--child", lib, "-", "trace"], a.timeout)
            rows[who] = trace_rows(d, [tuple(r.split("=", 1)) for r in a.rename] if who == "parent" else [])
        diff = list(difflib.unified_diff(rows["parent"], rows["result"], "parent", "result", lineterm="", n=0))
        with open(a.traces, "w") as f:
            print(f"kernel launches traced: parent {len(rows['parent'])}, result {len(rows['result'])}; lines of diff: {len(diff)}", file=f)
            by = {}
            for r in rows["result"]:
                k = re.sub(r"^void ", "", r.split("(")[0].split("  ")[0])
                by[k] = by.get(k, 0) + 1
            for k in sorted(by):
                if k.startswith("k_"):
                    print(f"  {by[k]:5d} x {k}", file=f)
            f.write("\n".join(diff) + ("\n" if diff else ""))
        bad += len(diff)
    if a.out:
        out.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
