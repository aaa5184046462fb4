"""The walk of the pixel-resident pass 2 (k_grads_t, qfa_grads_t.h) at the edges of its group count.

The walk takes the groups of 16 spectra of a range in three forms: a prologue (the first two groups' staging), a steady
state unrolled by two groups and a general step for what is left (the last groups of the range, the partial last group of the
batch; at N_h = 9..16 also every step of the ragged last tile and of the tile that holds the boundary).  A range of n groups
runs (n - 2) & ~1 steps in the steady state (N_h = 9..16 in batch order: (full groups - 2) & ~1), the rest in the general step.

How many groups a range has follows from the batch (qfa_gt.hip, gt_plan; ``plan_groups`` below recomputes it and
``test_the_cases_reach_the_group_counts`` asserts what is said here).  PB = pixel blocks of 8 wave tiles (16 pixels a tile at
N_h = 9..16, 32 at N_h <= 8); the planner takes the smallest number of ranges R <= groups / 2 whose PB R workgroups fill
whole rounds of the compute units to within 3 % of the best R, in deterministic mode at most one range per 64 spectra.
  * N_pix = 149 (PB = 2, at N_h = 8 PB = 1): every R up to groups / 2 is a fraction of one round, so R = groups / 2 (atomics) or
    ceil(B / 64) (deterministic): over ``SMALL_B`` a range has 1, 2, 3 or 4 groups (0: the workgroups that pad the grid),
    never more -- B = 247 = 16 groups is 8 ranges of 2 or, deterministic, 4 of 4.  The steady state is entered with 4 groups
    (deterministic; B = 64, 247, at N_h = 8 also B = 49), once.  ``F_PASS2_PIXRES`` forces the kernel onto these sizes.
  * N_pix = 2053 on 256 compute units: N_h = 12 has 129 tiles, PB = 17, and 15 ranges are one round (255 workgroups); N_h = 8
    has 65 tiles, PB = 9, 28 ranges (252).  ``LONG_B`` gives every range 5 groups (one steady iteration, three general
    steps) or 6 (two iterations, two steps), the batch's last group full or of 7 spectra, in both accumulation modes.

N_pix = 16 k + 5 (a ragged last tile), the boundary inside a tile (N_b = 55: tile 3; the long axis: where the grid puts it),
N_h = 12 (one tile per wave) and 8 (two), the three input forms, atomic and deterministic accumulation.  (N_b = 55 and not 53:
the shapes are those at which the numpy float32 oracle alone passes the bars, as tests/test_elementwise_ref_cpu.py asks of
E.GRADIENT_CASES.  At B = 1 every element is a sum of ONE term, and at N_b = 53, N_h = 8 the float32 oracle itself reads
1.32e-5 on omega[31] against that class's bar of 8.6e-6 -- k_grads_t reads 1.32e-5 there as well; over all cases at N_b = 55 the
float32 oracle stays below 0.28 of every bar.)

Every case is judged per element against the float64 oracle under the bars of tests/_elementwise_ref.py and its counts must be
the oracle's.  Its scalar gradients tau0 / c0 / beta, and those of k_grads_x (``F_PASS2_XDL``) on the same input, must be
within 1e-5 of the sum of |terms| per term counted of the float64 oracle's (the bar tests/test_fuzz_shapes.py asserts for
every form over drawn shapes), and within twice that of each other: two float32 sums of the same terms in another order.
"""
import numpy as np
import pytest

import _elementwise_ref as E
from oracle import qfa_oracle as O
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

SKEYS = ("tau0", "c0", "beta")
TOL_NLL = 5e-6
TOL_SCALAR = 1e-5           # (module docstring: against the oracle)
TOL_FORMS = 2e-5            # (between the two kernels)
# the batch sizes of the group edges; the last one is 16 groups less 9 spectra (the planner's ranges: module docstring)
SMALL_B = (1, 15, 16, 17, 33, 48, 49, 64, 81, 129, 16 * 3 * 5 + 7)
# N_h -> (groups per range, B): 15 (N_h = 12) or 28 (N_h = 8) ranges of five / six groups, the last group of 7 spectra / full
LONG_B = {12: ((5, 16 * 74 + 7), (5, 16 * 75), (6, 16 * 89 + 7), (6, 16 * 90)),
          8: ((5, 16 * 139 + 7), (5, 16 * 140), (6, 16 * 167 + 7), (6, 16 * 168))}
LONG_RANGES = {12: 15, 8: 28}
CASES = [(149, 55, nh, B) for nh in (12, 8) for B in SMALL_B] + [(2053, None, nh, B) for nh in (12, 8) for _, B in LONG_B[nh]]


def plan_groups(nh, B, npix, det, ncu, nxcd=8):
    """groups of 16 spectra per range of the launch of k_grads_t, as gt_plan (qfa_gt.hip) and its caller (qfa_host.h: at most
    ceil(B / 64) ranges with a slab) decide them; ``nxcd``: 8 on MI355X in SPX mode"""
    pxw = 32 if nh <= 8 else 16
    PB = -(-(-(-npix // pxw)) // 8)
    G = -(-B // 16)
    rmax = max(1, min(4 * ncu // max(1, PB) + 1, max(1, G // 2)))
    cost = lambda r: ((PB * r + ncu - 1) // ncu) / r
    best = min(cost(r) for r in range(1, rmax + 1))
    R = next(r for r in range(1, rmax + 1) if cost(r) <= 1.03 * best)
    up = (R + nxcd - 1) // nxcd * nxcd
    if R >= nxcd and R % nxcd and up <= rmax and cost(up) <= cost(R):
        R = up
    R = max(1, min(R, -(-B // 64) if det else 1 << 30))
    gpr = -(-G // R)
    return [min(gpr, G - r * gpr) for r in range(-(-G // gpr))]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def oracle_sums(p, b, rows):
    """one float64 pass over the spectra: what E.gradient_units gives for F, Psi, omega, and for the three scalar gradients
    (sum of the terms, sum of |terms|, number of non-zero terms)"""
    out, sc = None, {k: [0.0, 0.0, 0] for k in SKEYS}
    nll = np.empty(len(rows))
    for j, r in enumerate(rows):
        nll[j], g, ab = O.nll_and_grads_single(p, b["delta"][r], b["error"][r], b["zabs"][r], b["mask"][r], return_abs=True)
        if out is None:
            out = {k: {"sum": np.zeros_like(g[k]), "count": np.zeros(g[k].shape), "abssum": np.zeros_like(g[k])} for k in E.GKEYS}
        for k in E.GKEYS:
            out[k]["sum"] = out[k]["sum"] + g[k]
            out[k]["count"] = out[k]["count"] + (g[k] != 0.0)
            out[k]["abssum"] = out[k]["abssum"] + np.abs(g[k])
        for k in SKEYS:
            sc[k][0] += float(g[k]); sc[k][1] += float(ab[k]); sc[k][2] += int(g[k] != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in E.GKEYS:
            out[k]["grad"] = out[k]["sum"] / out[k]["count"]
    out["nll"] = nll
    return out, sc


@pytest.mark.parametrize("npix,nb,nh,B", CASES)
def test_walk_edges_against_the_oracle_and_k_grads_x(dev, npix, nb, nh, B):
    import torch
    from qfa_amd import QFA, synthetic
    from qfa_amd.resident import ResidentBatch
    from tools import parity_sections as PS
    p, mu, wav, nb, b, rows = E.gradient_case(npix, nb, nh, B) if nb is not None else E.long_case(npix, nh, B)
    ref, sc = oracle_sums(p, b, rows)                                          # (once per case)
    sel = E.select(b, rows)
    scale = np.maximum(np.maximum(np.abs(ref["nll"]), sel["mask"].sum(axis=1)), 1.0)
    f32 = torch.float32
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    N = len(b["delta"])
    d, er, mk = (torch.as_tensor(b[k], device=dev) for k in ("delta", "error", "mask"))
    idx = torch.as_tensor(rows.astype(np.int64), device=dev)
    zq1 = torch.as_tensor((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), device=dev)
    ratio = torch.as_tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev)
    stride = (npix + 31) // 32 * 32

    def pad(t, fill):
        out = torch.full((N, stride), fill, dtype=t.dtype, device=dev)
        out[:, :npix] = t
        return out
    rb = ResidentBatch(None, pad(d, -7.0e9), pad(er, float("nan")), pad(mk, True), zq1, ratio,
                       torch.as_tensor(rows.astype(np.int32), device=dev), npix, nb)
    sd, ser, smk = d[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
    z = torch.as_tensor(sel["zabs"], device=dev).to(f32).reshape(B, nb).contiguous()
    cnt_sl = PS.sections(m)["cnt"]

    def run(flags, form, det):
        m.flags, m.deterministic = flags, det
        nll = torch.empty(B, dtype=f32, device=dev)
        if form == "zabs":
            acc = m.accumulate(sd, ser, z, smk, nll=nll)
        elif form == "zfac":
            acc = m.accumulate(sd, ser, None, smk, nll=nll, zfac=(zq1[idx].contiguous(), ratio))
        else:
            acc = m.accumulate(batch=rb, nll=nll)
        acc = acc.clone()
        cnt = acc[cnt_sl].cpu().numpy()
        loss, gr = m._finalize(acc, True)
        return nll.cpu().numpy(), cnt, {k: v.cpu().numpy() for k, v in gr.items()}

    try:
        for det in (False, True):
            for form in ("zabs", "zfac", "rows"):
                what = f"(N_pix {npix}, N_b {nb}, N_h {nh}, B {B}; {form}, {'deterministic' if det else 'atomics'})"
                nll_t, cnt, gt = run(_lib.F_PASS2_PIXRES, form, det)
                _, _, gx = run(_lib.F_PASS2_XDL, form, det)
                assert np.all(np.isfinite(nll_t)), what
                assert np.max(np.abs(nll_t - ref["nll"]) / scale) < TOL_NLL, what
                for k in E.GKEYS:
                    E.check_gradient(k, gt[k], ref, E.GRADIENT_BARS[k], counts=cnt[:gt[k].shape[0]], what=what)
                for k in SKEYS:
                    total, absum, n = sc[k]
                    assert np.isfinite(gt[k]) == np.isfinite(gx[k]) == (n > 0), (k, what, gt[k], gx[k], n)
                    if n > 0 and absum > 0:
                        for kernel, ours in (("k_grads_t", gt[k]), ("k_grads_x", gx[k])):
                            units = abs(float(ours) - total / n) * n / absum
                            assert units <= TOL_SCALAR, f"{k} {what}: {kernel} {float(ours)!r}, oracle {total / n!r}: {units:.3e} of " \
                                                        f"the sum of |terms| per term (bar {TOL_SCALAR:.0e})"
                        units = abs(float(gt[k]) - float(gx[k])) * n / absum
                        assert units <= TOL_FORMS, f"{k} {what}: k_grads_t {float(gt[k])!r}, k_grads_x {float(gx[k])!r}, " \
                                                   f"{units:.3e} of the sum of |terms| per term apart (bar {TOL_FORMS:.0e}); oracle {total / n!r}"
    finally:
        m.flags, m.deterministic = 0, False


def test_the_cases_reach_the_group_counts(dev):
    """what the module docstring says about the planner, on this device: the coverage of the cases above stands and falls with it"""
    import torch
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    for nh in (12, 8):
        small = {(B, det): plan_groups(nh, B, 149, det, ncu) for B in SMALL_B for det in (False, True)}
        assert {n for g in small.values() for n in g} == {1, 2, 3, 4}, (nh, ncu, small)
        assert set(small[(247, False)]) == {2} and small[(247, True)] == [4, 4, 4, 4], (nh, ncu)
        # the steady state entered at N_pix = 149: ranges of four groups, all full but the batch's last
        for B in (64, 247) + ((49,) if nh == 8 else ()):
            assert 4 in small[(B, True)], (nh, B, ncu, small[(B, True)])
        for gpr, B in LONG_B[nh]:
            for det in (False, True):
                assert plan_groups(nh, B, 2053, det, ncu) == [gpr] * LONG_RANGES[nh], (nh, B, det, ncu)
    assert [B % 16 for _, B in LONG_B[12]] == [B % 16 for _, B in LONG_B[8]] == [7, 0, 7, 0]
