"""Static instruction census of the steady-state loop of a kernel in a -save-temps .s file (the design metric of the walk of
k_grads_t): for every kernel whose demangled name contains KERNEL, the loop (backward branch) with
the largest body, its instructions counted per class, and the kernel's registers / scratch.

    python tools/gt_walk_census.py [FILE.s] [KERNEL ...]
    (defaults: qfa_amd/csrc/build/qfa_gt-hip-amdgcn-amd-amdhsa-gfx950.s; the two reference-mode batch-order walks,
     'k_grads_t<16, false, true, false, false>' and 'k_grads_t<8, false, true, false, false>')

--loops N also lists the N next largest loops (the walk of waves 0..3 and of waves 4..7 are two loops; with the walk
unrolled by two, a loop body holds two groups: --groups G divides the counts)."""
import argparse
import re
import subprocess
from collections import Counter

CLASSES = ("MFMA", "VALU", "LDS", "vector memory", "scalar ALU", "scalar memory", "wait/nop", "branch", "barrier/prio")


def classify(op):
    if "mfma" in op:
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vector memory"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait/nop"
    if op.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if op.startswith(("s_barrier", "s_setprio", "s_sleep")):
        return "barrier/prio"
    if op.startswith("s_load") or op.startswith("s_buffer_load") or op.startswith("s_memtime"):
        return "scalar memory"
    if op.startswith("s_"):
        return "scalar ALU"
    return "other"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def loops_of(body):
    """(size, first line, last line, Counter of classes) of every backward branch, largest first"""
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    found = []
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            a = labels[m.group(1)]
            ops = [x.group(1) for x in (re.match(r"^\s+([a-z_0-9]+)", y) for y in body[a:i + 1]) if x]
            found.append((len(ops), a, i, Counter(classify(o) for o in ops), Counter(ops)))
    return sorted(found, key=lambda f: -f[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("args", nargs="*")
    ap.add_argument("--loops", type=int, default=1, help="how many of the largest loops to list per kernel")
    ap.add_argument("--groups", type=int, default=1, help="groups of spectra a loop body processes (2: the unrolled walk)")
    ap.add_argument("--moves", action="store_true", help="also count v_mov / v_accvgpr instructions of each loop (copies of W)")
    a = ap.parse_args()
    path = "qfa_amd/csrc/build/qfa_gt-hip-amdgcn-amd-amdhsa-gfx950.s"
    want = []
    for x in a.args:
        if x.endswith(".s"):
            path = x
        else:
            want.append(x)
    if not want:
        want = ["k_grads_t<16, false, true, false, false>", "k_grads_t<8, false, true, false, false>"]
    lines = open(path).read().split("\n")
    starts = [(i, m.group(1)) for i, m in ((i, re.match(r"^(_Z\w+):", l)) for i, l in enumerate(lines)) if m]
    names = demangle([n for _, n in starts])
    for i, n in starts:
        if not any(w.replace(" ", "") in names[n].replace(" ", "") for w in want):
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        body = lines[i:end]
        # the kernel's record in the amdhsa.kernels metadata: from its "  - ." line to the next one
        at = next((j for j, l in enumerate(lines) if re.match(r"^\s+\.name:\s+%s\s*$" % re.escape(n), l)), None)
        rec = []
        if at is not None:
            b0 = max(j for j in range(at + 1) if re.match(r"^  - \.", lines[j]))
            b1 = next((j for j in range(at + 1, len(lines)) if re.match(r"^  - \.|^\.\.\.|^amdhsa\.", lines[j])), len(lines))
            rec = lines[b0:b1]
        res = {}
        for key in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size"):
            mm = next((x for x in (re.search(r"\.%s:\s+(\d+)" % key, l) for l in rec) if x), None)
            res[key] = int(mm.group(1)) if mm else -1
        print(f"{names[n].split('(')[0]}")
        ninstr = sum(1 for y in body if re.match(r"^\s+[a-z]", y))
        print(f"  registers: vgpr {res['vgpr_count']} agpr {res['agpr_count']} sgpr {res['sgpr_count']} scratch {res['private_segment_fixed_size']} B; "
              f"kernel {ninstr} instructions")
        for size, lo, hi, cls, ops in loops_of(body)[:a.loops]:
            g = a.groups
            per = ", ".join(f"{c} {cls[c] / g:g}" for c in CLASSES + ("other",) if cls[c])
            print(f"  loop lines {lo}-{hi}: {size / g:g} instructions per group ({g} per body): {per}")
            if a.moves:
                mv = sum(v for k, v in ops.items() if k.startswith(("v_mov", "v_accvgpr")))
                print(f"    register moves (v_mov / v_accvgpr): {mv / g:g} per group")


if __name__ == "__main__":
    main()
