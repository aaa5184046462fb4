"""The N_h = 17..32 training step at the edges of its walks, every gradient element against the float64 oracle.

At N_h = 17..32 the step runs kernels that no other shape uses: pass 1 (k_moments_x<32>) with its accumulation chain cut at
QFA_P1_MAX_CHAIN = 32 tiles and k_sum_segments adding the partial records; pass 2 as k_s12_x (stages 1 and 2, beta / gamma
through HBM) and k_grads_s3 (stage 3, one launch per 16 output columns) -- qfa_amd/csrc/qfa_s12_x.h.  Both pass-2 kernels walk
the tiles of a work item in a ROTATED order (the walk of block blk starts at tile blk 2654435761 % min(n, 4), in k_grads_s3
% min(n, 32), and wraps), stream their operands through rings of LDS-DMA with counted waits (k_s12_x: a three-slot quarter
ring; a tile staged by the "ragged" path -- the last tile of the axis, and in the zabs form the tile that holds the boundary --
turns the counted wait into a full drain), keep inactive waves issuing every request, and flush with lanes outside the arrays
adding 0 or storing to a sink (k_grads_s3 addresses column b % N_h there).  A miscounted wait or a wrong wrap corrupts a few
elements of a few pixels: what the element judge of tests/_elementwise_ref.py sees and a whole-tensor rel-L2 does not.

The cases (E.S12_CASES; tests/test_s12_walk_edges_cpu.py judges the judge on the same inputs):
  * N_pix = 149 = 16 k + 5 (a ragged last tile of 16 and of 32 pixels), N_b = 55 (inside 32-pixel tile 1: ragged staging in the
    zabs form, the fast path in the factored one), thin coverage as E.gradient_case adds it; B = 15 .. 199 at N_h = 17 (one to
    four blocks of 64 spectra: rotations 0..3; 0 to 3 inactive waves in the last block; columns 16 .. 31 of the second
    k_grads_s3 launch hold ONE live column), B = 65, 199 at N_h = 24, B = 17, 65, 129 at N_h = 32.
  * N_pix = 1029 (33 tiles of 32 pixels: pass 1 in two chains of 17 and 16 tiles; the last tile has 5 pixels), N_h = 17, 24, 32,
    B = 17 and 70: every gradient element behind k_sum_segments.
  * Item lengths from the plan (E.plan_work, a port of qfa_host.h's; ``test_the_cases_reach_the_walk_edges`` asserts what is
    said here on the device's compute units): 293 and 389 pixels give k_s12_x items of 2 and of 1 tile next to the 3, 4 and 5 of
    the others; 69 pixels x 513 spectra give k_grads_s3 an item whose walk starts at tile 4.
  * B = 1 (every element ONE term) at the two (N_b, N_h) of those tried at which the numpy float32 oracle stays below half of
    every bar: (60, 17) and (100, 32) -- E.S12_B1 lists the others.
  * deterministic only, zabs only: B = 64 * 32 + 1 = 33 slab rows, the second chunk of the fixed-order reducer.

Every case runs the three input forms (zabs tensor, factored z, resident rows with padded rows), each with atomic and with
deterministic accumulation, flags = 0, exact_gradients off.  Each run: the per-spectrum NLL within TOL_NLL; F, Psi, omega by
E.check_gradient under E.GRADIENT_BARS with the kernel's own counts (the ``cnt`` section of the packed buffer); tau0 / c0 / beta
within 1e-5 of the sum of |terms| per term counted (the bar of tests/test_gt_walk_edges.py and tests/test_fuzz_shapes.py); in
deterministic mode a second identical call must return the same bits of the packed buffer.

QFA_F_S3_FAST (three bf16 piece products in k_grads_s3) on two cases: in deterministic mode everything but the F section of the
packed buffer, and the NLL, must equal the flags = 0 run bit for bit (the flag changes k_grads_s3 only); F keeps its count and
NaN-pattern check and the whole-tensor bar 1e-4 the suite asserts for this flag; its per-element units have no bar that could
be derived or measured against the reference and are recorded, not asserted (profiles/elementwise_accuracy.txt).
"""
import time

import numpy as np
import pytest

import _elementwise_ref as E
from conftest import rel_l2
from qfa_amd import _lib
from test_gt_walk_edges import SKEYS, oracle_sums

pytestmark = pytest.mark.gpu

TOL_NLL = 5e-6
TOL_SCALAR = 1e-5
TOL_F_FAST = 1e-4           # (whole tensor: tests/test_hip_parity.py, tests/test_stage3_precision.py)
FORMS = ("zabs", "zfac", "rows")
NO_BAR = (np.inf, np.inf)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Runner:
    """one case on the device: the model, the three input forms of its batch and the float64 oracle's sums (computed once)"""

    def __init__(self, dev, case):
        import torch
        from qfa_amd import QFA, synthetic
        from qfa_amd.resident import ResidentBatch
        from tools import parity_sections as PS
        self.torch, self.dev, self.case = torch, dev, case
        npix, nb, nh, B = case
        p, mu, wav, nb, b, rows = E.s12_case(*case)
        self.npix, self.nb, self.nh, self.B = npix, nb, nh, B
        t = time.perf_counter()
        self.ref, self.sc = oracle_sums(p, b, rows)
        self.oracle_seconds = time.perf_counter() - t
        sel = E.select(b, rows)
        self.scale = np.maximum(np.maximum(np.abs(self.ref["nll"]), sel["mask"].sum(axis=1)), 1.0)
        self.m = m = QFA(nb, npix - nb, nh, dev, model_params=p)
        assert m.exact_gradients is False
        N = len(b["delta"])
        d, er, mk = (torch.as_tensor(b[k], device=dev) for k in ("delta", "error", "mask"))
        self.idx = idx = torch.as_tensor(rows.astype(np.int64), device=dev)
        self.zq1 = zq1 = torch.as_tensor((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), device=dev)
        self.ratio = ratio = torch.as_tensor((wav[:nb] / synthetic.LYA).astype(np.float32), device=dev)
        stride = (npix + 31) // 32 * 32

        def pad(t, fill):
            out = torch.full((N, stride), fill, dtype=t.dtype, device=dev)
            out[:, :npix] = t
            return out
        self.rb = ResidentBatch(None, pad(d, -7.0e9), pad(er, float("nan")), pad(mk, True), zq1, ratio,
                                torch.as_tensor(rows.astype(np.int32), device=dev), npix, nb)
        self.sd, self.ser, self.smk = d[idx].contiguous(), er[idx].contiguous(), mk[idx].contiguous()
        self.z = torch.as_tensor(sel["zabs"], device=dev).to(torch.float32).reshape(B, nb).contiguous()
        self.sections = PS.sections(m)

    def what(self, form, det, extra=""):
        return f"(N_pix {self.npix}, N_b {self.nb}, N_h {self.nh}, B {self.B}; {form}, {'deterministic' if det else 'atomics'}{extra})"

    def run(self, flags, form, det):
        """(per-spectrum NLL, the packed buffer, the normalised gradients) as numpy"""
        torch, m = self.torch, self.m
        m.flags, m.deterministic = flags, det
        try:
            nll = torch.empty(self.B, dtype=torch.float32, device=self.dev)
            if form == "zabs":
                acc = m.accumulate(self.sd, self.ser, self.z, self.smk, nll=nll)
            elif form == "zfac":
                acc = m.accumulate(self.sd, self.ser, None, self.smk, nll=nll, zfac=(self.zq1[self.idx].contiguous(), self.ratio))
            else:
                acc = m.accumulate(batch=self.rb, nll=nll)
            acc = acc.clone()
            packed = acc.cpu().numpy().copy()
            loss, gr = m._finalize(acc, True)
            return nll.cpu().numpy(), packed, {k: v.cpu().numpy() for k, v in gr.items()}
        finally:
            m.flags, m.deterministic = 0, False

    def judge(self, nll, packed, gr, what, f_bar=E.GRADIENT_BARS["F"]):
        """the assertions of one run; returns the record line's columns"""
        ref = self.ref
        assert np.all(np.isfinite(nll)), what
        err = float(np.max(np.abs(nll - ref["nll"]) / self.scale))
        print(f"{what}: NLL {err:.3e}")
        assert err < TOL_NLL, (what, err)
        cnt = packed[self.sections["cnt"]]
        cols = []
        for k in E.GKEYS:
            bar = f_bar if k == "F" else E.GRADIENT_BARS[k]
            worst = E.check_gradient(k, gr[k], ref, bar, counts=cnt[:gr[k].shape[0]], what=what)
            print(f"{what}: {k} {worst[0]:.3e} (bar {bar[0]:.2e}), one term {worst[1]:.3e} (bar {bar[1]:.2e})")
            cols.append(f"{worst[0]:9.2e} {worst[1]:9.2e}")
        sca = []
        for k in SKEYS:
            total, absum, n = self.sc[k]
            assert bool(np.isfinite(gr[k])) == (n > 0), (k, what, gr[k], n)
            units = 0.0
            if n > 0 and absum > 0:
                units = abs(float(gr[k]) - total / n) * n / absum
                print(f"{what}: {k} {units:.3e} (bar {TOL_SCALAR:.0e})")
                assert units <= TOL_SCALAR, f"{k} {what}: ours {float(gr[k])!r}, oracle {total / n!r}: {units:.3e} of the sum of " \
                                            f"|terms| per term (bar {TOL_SCALAR:.0e})"
            sca.append(f"{units:8.2e}")
        return cols, sca, err


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def record(r, mode, form, det, cols, sca, err):
    E.record(f"s12 {r.npix:4d} {r.nb:3d} {r.nh:2d} {r.B:4d} {mode:4s} {form:4s} {'det' if det else 'atom'} | " + " | ".join(cols) +
             " | " + " ".join(sca) + f" | {err:8.2e}")


@pytest.mark.parametrize("case", E.S12_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_every_element_at_the_walk_edges(dev, case):
    r = Runner(dev, case)
    for det in (False, True):
        for form in FORMS:
            what = r.what(form, det)
            nll, packed, gr = r.run(0, form, det)
            cols, sca, err = r.judge(nll, packed, gr, what)
            record(r, "six", form, det, cols, sca, err)
            if det:
                nll2, packed2, _ = r.run(0, form, det)
                assert same_bits(packed, packed2) and same_bits(nll, nll2), f"{what}: a second identical call differs"


def test_the_second_chunk_of_the_fixed_order_reducer(dev):
    """33 slab rows: the reducer's first stage sums rows 0..31 and row 32 in two chunks; block 32 holds one spectrum"""
    r = Runner(dev, E.S12_DET_CASE)
    print(f"float64 oracle pass of {E.S12_DET_CASE}: {r.oracle_seconds:.2f} s")
    assert (r.B + 63) // 64 == 33
    what = r.what("zabs", True)
    nll, packed, gr = r.run(0, "zabs", True)
    cols, sca, err = r.judge(nll, packed, gr, what)
    record(r, "six", "zabs", True, cols, sca, err)
    nll2, packed2, _ = r.run(0, "zabs", True)
    assert same_bits(packed, packed2) and same_bits(nll, nll2), f"{what}: a second identical call differs"


@pytest.mark.parametrize("case", E.S12_FAST_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_s3_fast_changes_nothing_but_F(dev, case):
    r = Runner(dev, case)
    fsl = r.sections["accF"]
    for det in (False, True):
        for form in FORMS:
            what = r.what(form, det, ", QFA_F_S3_FAST")
            nll, packed, gr = r.run(_lib.F_S3_FAST, form, det)
            # Psi, omega, the counts, the scalars and the NLL under their own bars; F: NaN pattern and counts (no bar on the units)
            cols, sca, err = r.judge(nll, packed, gr, what, f_bar=NO_BAR)
            ok = ~np.isnan(r.ref["F"]["grad"])
            whole = rel_l2(gr["F"][ok], r.ref["F"]["grad"][ok])
            print(f"{what}: F whole tensor {whole:.3e} (bar {TOL_F_FAST:.0e})")
            assert whole < TOL_F_FAST, (what, whole)
            record(r, "fast", form, det, cols, sca, err)
            E.record(f"s12 fast F units NOT ASSERTED {r.npix:4d} {r.nb:3d} {r.nh:2d} {r.B:4d} {form:4s} {'det' if det else 'atom'} | {cols[0]}"
                     f" | whole tensor {whole:8.2e}")
            if det:
                what0 = r.what(form, det)
                nll0, packed0, gr0 = r.run(0, form, det)
                cols, sca, err = r.judge(nll0, packed0, gr0, what0)
                record(r, "six", form, det, cols, sca, err)
                assert same_bits(nll, nll0), f"{what}: the NLL differs from the flags = 0 run"
                assert same_bits(packed[fsl.stop:], packed0[fsl.stop:]), \
                    f"{what}: a section behind F of the packed buffer differs from the flags = 0 run (first at float " \
                    f"{fsl.stop + int(np.flatnonzero(packed[fsl.stop:].view(np.uint32) != packed0[fsl.stop:].view(np.uint32))[0])})"
                assert not same_bits(packed[fsl], packed0[fsl]), f"{what}: F is the flags = 0 run's bit for bit -- the flag did nothing"


def test_the_cases_reach_the_walk_edges(dev):
    """what the module docstring says about the plans, on this device: the coverage of the cases above stands and falls with it"""
    import torch
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    E.assert_s12_census(E.S12_CASES + [E.S12_DET_CASE] + E.S12_FAST_CASES, ncu)
