"""The judge and the plan port of tests/test_s12_walk_edges.py judged, without a GPU.

  * On every case of E.S12_CASES (and the deterministic-only and QFA_F_S3_FAST cases) the numpy float32 oracle passes
    E.check_gradient against the float64 oracle at no more than HALF of each bar -- the bars were measured on E.GRADIENT_CASES,
    and a case at which float32 arithmetic alone came near one would say nothing about the kernels' indexing --, nothing but
    count-0 elements is left out of the units, and the per-pixel count that the kernels keep is the oracle's (pixel, column) count.
  * The Python port of plan_work / plan_item (qfa_host.h, qfa_common.h), from which the GPU test's census derives which walk
    edges its cases reach, is pinned: every block of spectra meets every tile exactly once, no segment is empty, and plan_work
    equals the C++ function's values in tests/golden/plan_work_values.npz.  (plan_item is a __device__ function: a host program
    cannot call it; its port is held by the structural checks.)  Recorded by
        python tests/test_s12_walk_edges_cpu.py
    which builds tools/plan_work_dump.hip (host code including qfa_host.h as it is) with hipcc and runs it.
  * The census holds on 256 compute units (the GPU test asserts it on the device's own count).
  * Two planted faults of the kind a wrong wrap or a wrong sink address produces fail by at least 3 x their bar and are named
    by element; the whole-tensor rel-L2 at TOL_G passes the first (the second, at its mildest pixel, moves it to 1.7e-4).
"""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:                                    # (run as a script: pytest has tests/conftest.py do this)
    sys.path.insert(0, REPO)
import _elementwise_ref as E
from conftest import rel_l2

TOL_G = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5}             # (tests/test_hip_parity.py)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_work_values.npz")
ALL_CASES = E.S12_CASES + [E.S12_DET_CASE] + [c for c in E.S12_FAST_CASES if c not in E.S12_CASES]
FAULT_CASE = (149, 55, 17, 199)


def units_of(ref, key, ours):
    return E.grad_error_units(ours, ref[key]["grad"], ref[key]["abssum"], ref[key]["count"])


def fails_naming(fn, *names):
    with pytest.raises(AssertionError) as ei:
        fn()
    for n in names:
        assert n in str(ei.value), (n, str(ei.value))


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_float32_oracle_stays_below_half_of_every_bar(case):
    p, mu, wav, nb, b, rows = E.s12_case(*case)
    ref = E.gradient_units(p, b, rows)
    f32 = E.gradient_units(p, b, rows, dtype=np.float32)
    seen = E.select(b, rows)["mask"].sum(axis=0)
    if case[1] is not None:
        (a, e), none, last = E.thin_pixels(case[0])
        assert np.all(seen[a:e] == 1) and seen[none] == 0 and seen[last] == 1
    for k in E.GKEYS:
        n = ref[k]["grad"].shape[0]
        assert np.array_equal(ref[k]["count"], np.broadcast_to(seen[:n].reshape((n,) + (1,) * (ref[k]["count"].ndim - 1)),
                                                               ref[k]["count"].shape)), k
        u = units_of(ref, k, f32[k]["grad"])
        assert np.array_equal(np.isnan(u), ref[k]["count"] == 0), k           # only count-0 elements are left out
        half = tuple(0.5 * x for x in E.GRADIENT_BARS[k])
        E.check_gradient(k, f32[k]["grad"], ref, half, counts=f32[k]["count"], what=f"{case} (float32 oracle, HALF the bars)")


# ---------------------------------------------------------------------------------------------------------------------
# the plan port
# ---------------------------------------------------------------------------------------------------------------------
def test_every_block_meets_every_tile_once_and_no_segment_is_empty():
    shapes = {(c[0], c[3]) for c in ALL_CASES} | {(2053, 1207), (640, 3000), (7781, 20000), (33, 1)}
    for npix, B in sorted(shapes):
        for ncu in (1, 64, 256, 304):
            for name, (wp, nt) in E.s12_plans(npix, B, ncu).items():
                full, rem, nseg, st = wp
                items = E.plan_items(wp, nt)
                assert len(items) == full + rem * nseg and full + rem == (B + 63) // 64, (npix, B, ncu, name, wp)
                met = np.zeros(((B + 63) // 64, nt), dtype=int)
                for blk, seg, t0, t1 in items:
                    assert 0 <= t0 < t1 <= nt, (npix, B, ncu, name, wp, (blk, seg, t0, t1))
                    met[blk, t0:t1] += 1
                    for window in (4, 32):
                        assert 0 <= E.rot_of(blk, t1 - t0, window) < min(t1 - t0, window)
                assert np.all(met == 1), (npix, B, ncu, name, wp)
                if name == "wp1":
                    assert max(t1 - t0 for _, _, t0, t1 in items) <= E.P1_MAX_CHAIN, (npix, B, ncu, wp)


def test_plan_work_equals_the_recorded_values_of_the_host_function():
    rows = np.load(FIXTURE)["rows"]
    assert rows.shape[1] == 10 and len(rows) > 4000
    assert {tuple(r) for r in rows[:, 2:6:3]} >= {(4, 0), (3, 0), (1, 0), (1, E.P1_MAX_CHAIN)}          # (pro, max_chain)
    for B, nt, pro, slots, spb, mc, full, rem, nseg, st in rows.tolist():
        assert E.plan_work(B, nt, pro, slots, spb, mc) == (full, rem, nseg, st), (B, nt, pro, slots, spb, mc)


def test_the_cases_reach_the_walk_edges_on_256_compute_units():
    c = E.assert_s12_census(ALL_CASES, 256)
    # what the case table's comments say of the plans
    assert {4, 2} <= {t1 - t0 for _, _, t0, t1 in E.plan_items(*E.s12_plans(293, 17, 256)["wp2x"])}
    assert [t1 - t0 for _, _, t0, t1 in E.plan_items(*E.s12_plans(389, 65, 256)["wp2x"])][-1] == 1
    assert E.s12_plans(69, 513, 256)["wp2"] == ((0, 9, 1, 5), 5) and E.rot_of(8, 5, 32) == 4
    assert all(E.rot_of(blk, 5, 4) == blk for blk in range(4))            # N_pix = 149, B = 199: rot = 0..3 in k_s12_x
    assert c["nseg1"][(1029, None, 17, 17)] == 2 and E.s12_plans(1029, 17, 256)["wp1"][0][3] == 17     # chains of 17 and 16 tiles


# ---------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fault():
    p, mu, wav, nb, b, rows = E.s12_case(*FAULT_CASE)
    return E.gradient_units(p, b, rows), E.gradient_units(p, b, rows, dtype=np.float32)


def test_a_pixel_of_the_wrapped_to_tile_given_the_next_tiles_value_fails_where_the_whole_tensor_norm_passes(fault):
    """k_s12_x walks the one item of this case (tiles 0..4, the last ragged) from tile rot = blk % 4 on and wraps to tile 0; a
    wrap that is off by a tile gives a pixel of tile 0 the sums of the same pixel of tile 1"""
    ref, f32 = fault
    wp, nt = E.s12_plans(FAULT_CASE[0], FAULT_CASE[3], 256)["wp2x"]
    assert [(t0, t1) for _, _, t0, t1 in E.plan_items(wp, nt)] == [(0, 5)] * 4
    blind = 0
    for k in ("Psi", "F"):
        r = ref[k]["grad"]
        dense = (ref[k]["count"][:32] >= 2) & (ref[k]["count"][32:64] >= 2)
        planted = f32[k]["grad"].astype(np.float64).copy()
        planted[:32] = planted[32:64]
        u = units_of(ref, k, planted)[:32]
        # of the elements at which the fault is at least 3 x the bar, the one it changes least: what a whole-tensor norm sees least
        cand = dense & (u >= 3 * E.GRADIENT_BARS[k][0])
        assert cand.any(), k
        d = np.where(cand, np.abs(planted[:32] - r[:32]), np.inf)
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmin(d)), d.shape))
        g = f32[k]["grad"].astype(np.float64).copy()
        g[idx] = g[(idx[0] + 32,) + idx[1:]]
        assert units_of(ref, k, g)[idx] >= 3 * E.GRADIENT_BARS[k][0]
        fails_naming(lambda: E.check_gradient(k, g, ref, E.GRADIENT_BARS[k], what=str(FAULT_CASE)), str(idx))
        ok = ~np.isnan(r)
        blind += rel_l2(g[ok], r[ok]) < TOL_G[k]
    assert blind >= 1, "the whole-tensor rel-L2 at TOL_G was expected to miss this fault"


def test_column_16_of_F_given_column_0s_value_fails(fault):
    """the second k_grads_s3 launch at N_h = 17 has ONE live column; its lanes of the columns b = 17 .. 31 address column b % 17
    and must add 0 or store to the sink: a lane that does not gives (px, 16) and (px, 0) each other's sums"""
    ref, f32 = fault
    r = ref["F"]["grad"]
    assert r.shape[1] == 17
    planted = f32["F"]["grad"].astype(np.float64).copy()
    planted[:, 16] = planted[:, 0]
    u = units_of(ref, "F", planted)[:, 16]
    cand = (ref["F"]["count"][:, 16] >= 2) & (u >= 3 * E.GRADIENT_BARS["F"][0])
    assert cand.sum() >= 100, "nearly every pixel shows it"
    px = int(np.argmin(np.where(cand, np.abs(planted[:, 16] - r[:, 16]), np.inf)))
    g = f32["F"]["grad"].astype(np.float64).copy()
    g[px, 16] = g[px, 0]
    assert units_of(ref, "F", g)[px, 16] >= 3 * E.GRADIENT_BARS["F"][0]
    fails_naming(lambda: E.check_gradient("F", g, ref, E.GRADIENT_BARS["F"], what=str(FAULT_CASE)), f"({px}, 16)")


if __name__ == "__main__":
    import subprocess
    import tempfile
    repo = REPO
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "plan_work_dump")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--offload-arch=gfx950", "-I",
                        os.path.join(repo, "qfa_amd", "csrc"), os.path.join(repo, "tools", "plan_work_dump.hip"), "-o", exe], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()
    rows = np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int32)
    np.savez_compressed(FIXTURE, rows=rows)
    print("recorded", FIXTURE, rows.shape)
