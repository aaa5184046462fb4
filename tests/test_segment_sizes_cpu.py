"""The size functions of the four segment statistics (p1d, p1d_band, xi, flux_pdf) against recorded values: what
`qfa_*_stack_doubles`, `qfa_*_workspace_bytes` and `qfa_p1d_band_chunk_segments` return defines the callers' stacks and workspaces
and the cuts of a call into launches, so a change of the launch plans must not move any of them.  tests/golden/segment_sizes.npz
holds the arguments and the values of the library before the four calls were folded onto one plan; as a script,

    python tests/test_segment_sizes_cpu.py path/to/libqfa_hip.so

records the fixture from that library.  These functions need no GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment_sizes.npz")

# the own size of each call: (stack_doubles, workspace_bytes, its largest value or None for "the segment's length")
OWN = {"p1d": None, "p1d_band": 64, "xi": None, "flux_pdf": 64}


def grid():
    """{function name: int32 (n, k) arguments}: accepted shapes at the ends of every range, around the chunk of 64 segments and at
    the benchmark's 4096 x 100, and refused ones (R no multiple of S, segments past Nb, every count one outside its range)"""
    stack, work = {k: set() for k in OWN}, {k: set() for k in OWN}
    for S, nz in itertools.product((0, 1, 3, 100), (0, 1, 8, 4096, 4097)):
        for x in (-1, 0, 1, 2, 9, 37, 64, 65, 240, 4096, 4097):
            for k in OWN:
                stack[k].add((S, nz, x))
    for S, nseg, L, nz in itertools.product((1, 3, 100), (1, 2, 3, 64, 65), (1, 37, 240, 4096), (8, 4096)):
        for R in sorted({0, 1, 63, 64, 65, 4096 * 100} | {b * S for b in (1, 63, 64, 65)}):
            for Nb in (nseg * L, nseg * L + 5, nseg * L - 1):
                work["p1d"].add((R, S, Nb, L, nseg, nz))
                for k, top in OWN.items():
                    if k != "p1d":
                        for x in (0, 1, min(9, L), top or L, (top or L) + 1):
                            work[k].add((R, S, Nb, L, nseg, nz, x))
    for bad in ((-3, 3, 120, 40, 3, 8), (6, 0, 120, 40, 3, 8), (6, 3, 0, 40, 3, 8), (6, 3, 120, 0, 3, 8), (6, 3, 12291, 4097, 3, 8),
                (6, 3, 120, 40, 0, 8), (6, 3, 120, 40, 3, 0), (6, 3, 120, 40, 3, 4097)):
        work["p1d"].add(bad)
        for k in ("p1d_band", "xi", "flux_pdf"):
            work[k].add(bad + (5,))
    out = {}
    for k in OWN:
        out[f"qfa_{k}_stack_doubles"] = np.array(sorted(stack[k]), np.int32)
        out[f"qfa_{k}_workspace_bytes"] = np.array(sorted(work[k]), np.int32)
    return out


def evaluate(path):
    """{name: uint64 values over grid()[name]} and the chunk constant of the library at `path`"""
    h = C.CDLL(path)
    out = {}
    for name, args in grid().items():
        f = getattr(h, name)
        f.restype, f.argtypes = C.c_size_t, [C.c_int] * args.shape[1]
        out[name] = np.array([f(*(int(v) for v in a)) for a in args], np.uint64)
    h.qfa_p1d_band_chunk_segments.restype = C.c_int
    out["qfa_p1d_band_chunk_segments"] = np.array([h.qfa_p1d_band_chunk_segments()], np.uint64)
    return out


def test_size_functions_return_the_recorded_values():
    from qfa_amd import _lib
    want, args, got = np.load(FIXTURE), grid(), evaluate(_lib.LIB_PATH)
    assert set(want.files) == set(got) | {"args:" + k for k in args}
    for name, a in args.items():
        assert np.array_equal(want["args:" + name], a), name                         # (the fixture was recorded on this grid)
        accepted = want[name] > 0
        assert accepted.sum() > len(a) // 8 and (~accepted).sum() > 8, name          # (both sides of every check are in it)
    for name, v in got.items():
        differ = np.flatnonzero(v != want[name])
        assert differ.size == 0, (name, args[name][differ[:5]].tolist() if name in args else None, v[differ[:5]], want[name][differ[:5]])


if __name__ == "__main__":
    rec = evaluate(os.path.abspath(sys.argv[1]))
    rec.update({"args:" + k: v for k, v in grid().items()})
    np.savez_compressed(FIXTURE, **rec)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes;", {k: len(v) for k, v in rec.items() if not k.startswith("args:")})
