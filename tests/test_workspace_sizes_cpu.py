"""`qfa_workspace_bytes` and `qfa_em_workspace_bytes` against recorded values.  tests/golden/workspace_sizes.npz holds the shapes and
the values of the library that still reserved the pass-1 float32 image PF as the first region of every workspace (16-pixel tiles of
16 x NCPL floats, NCPL = 68 / 164 / 564 at KP = 8 / 16 / 32, rounded to 64 floats like every region).  That region is gone and nothing
else moved: both sizes are the recorded ones minus exactly that term -- which also pins the rows of the pixel-resident pass 2
(pixres_rows_layout sizes them and the step's plan addresses them).

`qfa_det_slab_bytes` against tests/golden/det_slab_sizes.npz: the same shapes with N_b = N_pix // 2 and N_b = N_pix, recorded from the
library as it stood before the row region of the slab and of the workspace got one builder (rows_region); the values are the recorded
ones exactly.  As a script,

    python tests/test_workspace_sizes_cpu.py path/to/libqfa_hip.so [--workspace]

records det_slab_sizes.npz from that library (and, with --workspace, workspace_sizes.npz: only from the older library that still had
the PF region).  These functions need no GPU: with no device visible the library plans for 256 compute units and 8 XCDs."""
import ctypes as C
import os
import sys

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.npz")
SLAB_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_slab_sizes.npz")

# (B, Npix, N_h): KP = 8 / 16 / 32, Npix no multiple of 16 or 32, B = 1, and B on both sides of what selects the pixel-resident
# pass 2 (128 spectra at KP = 16 and 512 at KP = 8 from 1024 pixels on, 96 spectra per CU = 24 576 below that)
SHAPES = np.array([
    (1, 1, 1), (1, 33, 5), (1, 2000, 8), (1, 97, 9), (1, 4000, 16), (1, 200, 17), (1, 1913, 32),
    (17, 33, 1), (65, 97, 5), (130, 200, 8), (511, 1024, 8), (512, 1024, 8), (513, 1023, 8), (512, 1025, 7),
    (10000, 2000, 8), (24575, 640, 8), (24576, 640, 8), (24577, 647, 3), (9216, 9243, 8),
    (17, 33, 9), (65, 97, 13), (130, 200, 16), (127, 1024, 16), (128, 1024, 16), (129, 1023, 12), (128, 1031, 16),
    (8000, 4000, 16), (24575, 640, 16), (24576, 640, 16), (24577, 999, 10), (32768, 4000, 16), (100000, 640, 16),
    (17, 33, 17), (65, 97, 24), (130, 200, 32), (127, 1024, 20), (128, 1031, 32), (2048, 9243, 32), (2049, 4001, 17),
    (24576, 640, 32), (20000, 1913, 24),
], np.int32)
NCPL = {8: 68, 16: 164, 32: 564}


def pf_bytes(npix, nh):
    """bytes of the retired PF region"""
    kp = 8 if nh <= 8 else (16 if nh <= 16 else 32)
    floats = (npix + 15) // 16 * 16 * NCPL[kp]
    return 4 * ((floats + 63) // 64 * 64)


def evaluate(path):
    h = C.CDLL(path)
    out = {}
    for name in ("qfa_workspace_bytes", "qfa_em_workspace_bytes"):
        f = getattr(h, name)
        f.restype, f.argtypes = C.c_size_t, [C.c_int] * 3
        out[name] = np.array([f(*(int(v) for v in s)) for s in SHAPES], np.uint64)
    return out


def evaluate_slab(path):
    """qfa_det_slab_bytes(B, Npix, Nb, Nh) on SHAPES: column 0 with Nb = Npix // 2, column 1 with Nb = Npix"""
    f = C.CDLL(path).qfa_det_slab_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * 4
    return np.array([[f(int(b), int(n), nb, int(k)) for nb in (int(n) // 2, int(n))] for b, n, k in SHAPES], np.uint64)


def test_workspaces_shrank_by_the_pf_region_and_nothing_else():
    from qfa_amd import _lib
    want, got = np.load(FIXTURE), evaluate(_lib.LIB_PATH)
    assert np.array_equal(want["shapes"], SHAPES)                                        # (the fixture was recorded on these shapes)
    pf = np.array([pf_bytes(int(n), int(k)) for _, n, k in SHAPES], np.uint64)
    for name, v in got.items():
        assert (want[name] > pf).all(), name
        differ = np.flatnonzero(v != want[name] - pf)
        assert differ.size == 0, (name, SHAPES[differ[:5]].tolist(), v[differ[:5]], (want[name] - pf)[differ[:5]])


def test_det_slab_sizes_are_the_recorded_ones():
    from qfa_amd import _lib
    want, got = np.load(SLAB_FIXTURE), evaluate_slab(_lib.LIB_PATH)
    assert np.array_equal(want["shapes"], SHAPES)
    assert (want["qfa_det_slab_bytes"] > 0).all()
    differ = np.flatnonzero((got != want["qfa_det_slab_bytes"]).any(axis=1))
    assert differ.size == 0, (SHAPES[differ[:5]].tolist(), got[differ[:5]], want["qfa_det_slab_bytes"][differ[:5]])


if __name__ == "__main__":
    path = os.path.abspath(sys.argv[1])
    if "--workspace" in sys.argv[2:]:
        rec = evaluate(path)
        rec["shapes"] = SHAPES
        np.savez_compressed(FIXTURE, **rec)
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes;", {k: len(v) for k, v in rec.items()})
    np.savez_compressed(SLAB_FIXTURE, shapes=SHAPES, qfa_det_slab_bytes=evaluate_slab(path))
    print(SLAB_FIXTURE, os.path.getsize(SLAB_FIXTURE), "bytes")
