"""Every element of the EM statistics and every solved row of F (qfa_em_stats_f32, qfa_em_update_f_f32; kernels in
qfa_amd/csrc/qfa_em.h) against float64, by the judges of tests/_em_ref.py:

* S2 and S1 element by element in units of the element's own sum of |terms| (``stat_units``) under STAT_BARS = 8 x the float32
  numpy restatement's distance from float64 on these very cases (tools/em_bars.py, profiles/em_accuracy.txt); cnt exactly --
  at the shapes of tests/test_em_step.py in every input form, at the smallest shapes whose ranges hold more than 256 spectra
  (the fold of k_em_stats' MFMA accumulators, in each launch_stats instantiation and column pass), and for two different
  batches accumulated into one buffer;
* the solve row by row on hand-built float32 statistics against ``solve_rows`` on the same numbers, under the derived bar of
  ``solve_bar``; the skipped rows exactly.

QFA_EM_LOG=<file>: the achieved worst units are appended there (profiles/em_accuracy.txt, section 3)."""
import ctypes as C
import os

import numpy as np
import pytest

import _em_ref as E
from test_em_step import T, setup, tensors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def record(line):
    print(line)
    path = os.environ.get("QFA_EM_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run_case(dev, case, plant=None, batch_seed=None):
    """the model's statistics of a case of E.ELEMENT_CASES in its input form and the float64 terms of the same inputs:
    (model, st, a second call's st, ref, p, b, dead, zfac, model call)"""
    import torch
    from qfa_amd import QFA, utils
    kind, npix, nh, B, form, seed = case
    m, p, b, zfac, dead = setup(dev, npix, nh, B, seed, plant=plant, batch_seed=batch_seed)
    d, e, z, mk = tensors(b, dev)
    ab = None
    if form == "zabs":
        call = lambda **kw: m.em_statistics(d, e, z, mk, **kw)
        zref = b["zabs"]
    elif form == "factored":
        call = lambda **kw: m.em_statistics(d, e, None, mk, zfac=zfac, **kw)
        zref = E.zabs_of((zfac[0].cpu().numpy(), zfac[1].cpu().numpy()))
    else:                                                               # the host-supplied A_blue: a tau callable
        tau = lambda zz: utils.tau(zz, which="becker")
        m = QFA(m.Nb, m.Nr, nh, dev, tau=tau, model_params=p)
        assert m._tau_callable is not None
        call = lambda **kw: m.em_statistics(d, e, z, mk, **kw)
        zref = b["zabs"]
        ab = torch.exp(-1. * tau(z)).to(torch.float32).cpu().numpy()    # the very array the kernels are handed
    st = call()
    ref = E.em_terms(p, b["delta"], b["error"], zref, b["mask"], A_blue=ab)
    return m, st, ref, p, b, dead, zfac, call


def judge(st, ref, tag):
    """every element of st under its bar; the worst units and where they sit are printed before anything is asserted"""
    import torch
    S2, S1 = st.S2.double().cpu().numpy(), st.S1.double().cpu().numpy()
    for k, ours in (("S2", S2), ("S1", S1)):
        (w, idx), (w1, idx1) = E.class_worst(E.stat_units(ours, ref[k], ref["abs" + k]), ref["cnt"])
        record(f"em elements {tag} {k}: cnt >= 2 worst {w:.3e} at {idx} (bar {E.STAT_BARS[k][0]:.2e}); "
               f"cnt = 1 worst {w1:.3e} at {idx1} (bar {E.STAT_BARS[k][1]:.2e})")
    w = E.check_stat_elements(S2, S1, st.cnt.cpu().numpy(), ref, what=str(tag))
    assert torch.equal(st.S2, st.S2.transpose(1, 2)), tag               # symmetric bit for bit
    return w


# ----------------------------------------------------------------------------------------------------------------------
# 1. every element at the shapes the rel-L2 tests use
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in E.ELEMENT_CASES if c[0] == "shape"], ids=lambda c: "-".join(str(x) for x in c[1:5]))
def test_every_element_at_the_existing_shapes(dev, case):
    m, st, ref, p, b, dead, zfac, call = run_case(dev, case)
    judge(st, ref, case[1:5])
    if dead is not None:
        assert (st.cnt[dead[0]:dead[1]] == 0).all() and (st.S2[dead[0]:dead[1]] == 0).all() and (st.S1[dead[0]:dead[1]] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. past the fold of the MFMA accumulators
# ----------------------------------------------------------------------------------------------------------------------
def assert_past_the_fold(B, npix, nh):
    """the test is where it means to be: ranges of more than 256 spectra and a last range that is no multiple of 4"""
    from qfa_amd import _lib
    h = _lib.lib()
    R, per, last = E.plan_from_bytes(h.qfa_em_workspace_bytes(B, npix, nh), h.qfa_workspace_bytes(B, npix, nh), B, npix, nh)
    assert per > 256 and last % 4 != 0 and (B % per) % 4 != 0, (R, per, last)
    assert (R, per, last) == (E.FOLD_R, E.FOLD_PER, B - (E.FOLD_R - 1) * E.FOLD_PER), (R, per, last)   # (fold_plant's ranges)
    return R, per, last


@pytest.mark.parametrize("nh,form", E.FOLD_CASES)
def test_every_element_past_the_fold(dev, nh, form):
    import torch
    case = [c for c in E.ELEMENT_CASES if c[0] == "fold" and c[2] == nh][0]
    assert case[4] == form
    B, npix = E.FOLD_B, E.FOLD_NPIX
    R, per, last = assert_past_the_fold(B, npix, nh)
    m, st, ref, p, b, dead, zfac, call = run_case(dev, case, plant=E.fold_plant)
    # the planted columns are what they are meant to be (the 1 % masks may take single observers away, never add one)
    seen = {k: np.flatnonzero(b["mask"][:, c]) for k, c in E.FOLD_COLUMNS.items()}
    assert len(seen["late"]) >= 30 and (seen["late"] % per >= 256).all()
    assert len(seen["early"]) >= 1000 and (seen["early"] % per < 256).all() and (seen["early"] >= (R - 1) * per).any()
    assert seen["single"].tolist() == [B - 1] and ref["cnt"][E.FOLD_COLUMNS["single"]] == 1
    judge(st, ref, ("fold", npix, nh, B, form))
    for k, c in E.FOLD_COLUMNS.items():
        u2 = E.stat_units(st.S2[c].double().cpu().numpy(), ref["S2"][c], ref["absS2"][c]).max()
        u1 = E.stat_units(st.S1[c].double().cpu().numpy(), ref["S1"][c], ref["absS1"][c]).max()
        record(f"em elements fold nh {nh} column {k} ({c}, cnt {ref['cnt'][c]:.0f}): S2 {u2:.3e} S1 {u1:.3e}")
    assert torch.equal(st.buf, call().buf)                              # two calls, the same bits
    assert (st.cnt[dead[0]:dead[1]] == 0).all() and (st.S2[dead[0]:dead[1]] == 0).all() and (st.S1[dead[0]:dead[1]] == 0).all()


def test_resident_form_past_the_fold_is_bit_equal_to_the_gathered_batch(dev):
    import torch
    from qfa_amd.resident import ResidentBatch
    nh = 4
    B, npix, stride = E.FOLD_B, E.FOLD_NPIX, E.FOLD_NPIX + 24
    assert_past_the_fold(B, npix, nh)
    N = B + 11
    m, p, b, zfac, _ = setup(dev, npix, nh, N, seed=100 + nh)
    def pad(a, dt, fill):
        out = torch.full((N, stride), fill, dtype=dt, device=dev)
        out[:, :npix] = a
        return out
    d, e, z, mk = tensors(b, dev)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:B].to(torch.int32).to(dev)
    rb = ResidentBatch(None, pad(d, torch.float32, 0.0), pad(e, torch.float32, 0.0), pad(mk, torch.bool, False),
                       zfac[0], zfac[1], rows, npix, m.Nb)
    st = m.em_statistics(batch=rb)
    (gd, ge, gz, gm), gzf = rb.materialize()
    st2 = m.em_statistics(gd, ge, gz, gm, zfac=gzf)
    assert torch.equal(st.buf, st2.buf)
    assert float(st.tail[1].item()) == B and torch.isfinite(st.buf).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3. two different batches into one buffer
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in E.ELEMENT_CASES if c[0] == "accum"], ids=lambda c: "-".join(str(x) for x in c[1:4]))
def test_two_different_batches_accumulate(dev, case):
    kind, npix, nh, B, form, seed = case
    m, st, ref1, p, b1, dead, zfac, call = run_case(dev, case)
    one = st.clone()
    p2, b2 = E.em_inputs(npix, nh, B, seed, batch_seed=seed + 50)[:2]
    assert np.array_equal(p2["F"], p["F"]) and not np.array_equal(b2["mask"], b1["mask"])
    ref2 = E.em_terms(p, b2["delta"], b2["error"], b2["zabs"], b2["mask"])
    out = m.em_statistics(*tensors(b2, dev), stats=st)
    assert out is st
    both = {k: ref1[k] + ref2[k] for k in ("S2", "S1", "absS2", "absS1", "cnt")}
    judge(st, both, ("accum", npix, nh, B))
    assert float(st.tail[1].item()) == 2.0 * B and float(st.tail[2].item()) == 0.0
    nll = ref1["nll_sum"] + ref2["nll_sum"]
    assert abs(float(st.tail[0].item()) - nll) <= 5e-6 * abs(nll)
    # and the second batch alone, into a fresh buffer, is what was added: float32 add of the two, element by element
    two = m.em_statistics(*tensors(b2, dev))
    import torch
    assert torch.equal(st.buf[:-4], one.buf[:-4] + two.buf[:-4])


# ----------------------------------------------------------------------------------------------------------------------
# 4. the solve, row by row, on hand-built statistics
# ----------------------------------------------------------------------------------------------------------------------
def gpu_solve(dev, buf, F, npix, nh, ridge, damping, in_place):
    """qfa_em_update_f_f32 through the C-ABI: (F_out, number skipped or None).  Out of place: n_skipped = NULL"""
    import torch
    from qfa_amd import _lib
    Fin = F.clone()
    if in_place:
        out, nsk = Fin, torch.full((1,), 12345, dtype=torch.int32, device=dev)
    else:
        out, nsk = torch.full_like(F, 7.0), None
    _lib.check(_lib.lib().qfa_em_update_f_f32(C.c_void_p(buf.data_ptr()), C.c_void_p(Fin.data_ptr()), npix, nh, float(ridge),
                                              float(damping), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(nsk.data_ptr()) if nsk is not None else None,
                                              _lib.current_stream(dev)), "update")
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(Fin, F)                                      # F untouched
    return out.cpu().numpy(), None if nsk is None else int(nsk.item())


def stats_buffer(dev, S2, S1, cnt):
    from qfa_amd import _lib
    npix, nh = S1.shape
    flat = np.concatenate([S2.ravel(), S1.ravel(), cnt.ravel(), np.zeros(4, np.float32)]).astype(np.float32)
    assert flat.size == _lib.lib().qfa_em_floats(npix, nh)
    return T(flat, dev)


@pytest.mark.parametrize("npix", E.SOLVE_NPIX)
@pytest.mark.parametrize("nh", E.SOLVE_NH)
def test_every_solved_row(dev, nh, npix):
    S2, S1, cnt, F, planted = E.solve_case(npix, nh)
    buf, Fd = stats_buffer(dev, S2, S1, cnt), T(F, dev)
    worst = used = 0.0
    for ridge, damping in E.SOLVE_RIDGE_DAMPING:
        want, skipped, cond, x = E.solve_rows((S2, S1, cnt), F, ridge, damping)
        if ridge == 0.0:
            for name, i in planted.items():
                assert skipped[i], (name, i)                            # kept, whatever else the reference thinks
                for j in range(4 * (i // 4), min(npix, 4 * (i // 4) + 4)):
                    assert skipped[j] == (j in planted.values()), (name, i, j)     # its neighbours in the block are solved
        bar = E.solve_bar(want, np.where(skipped[:, None], 0.0, x), np.where(skipped, 0.0, cond), nh, damping)
        for in_place in (True, False):
            got, n = gpu_solve(dev, buf, Fd, npix, nh, ridge, damping, in_place)
            tag = (npix, nh, ridge, damping, "in place" if in_place else "out of place")
            if in_place:
                assert n == int(skipped.sum()), (tag, n, int(skipped.sum()))
            kept = (got.view(np.uint32) == F.view(np.uint32)).all(axis=1)
            assert np.array_equal(got[skipped].view(np.uint32), F[skipped].view(np.uint32)), tag     # bit-equal to the old F
            if damping != 0.0:
                assert not kept[~skipped].any(), (tag, np.flatnonzero(kept & ~skipped)[:5])          # the mask is exact
            assert np.isfinite(got).all(), tag
            err = np.abs(got.astype(np.float64) - want)
            ratio = np.where(skipped[:, None], 0.0, err / np.where(bar > 0, bar, 1.0))
            ratio = np.where((bar == 0) & (err > 0), np.inf, ratio)
            i = int(np.argmax(ratio.max(axis=1)))
            worst = max(worst, float(ratio.max()))
            # how much of the bar's solve term is used once the float32 rounding is taken off (a figure, not a bar)
            term = bar - 2.0 ** -24 * np.abs(want)
            beyond = np.where(skipped[:, None] | (term <= 0), 0.0, np.maximum(err - 2.0 ** -24 * np.abs(want), 0.0) / np.where(term > 0, term, 1.0))
            used = max(used, float(beyond.max()))
            assert ratio.max() <= 1.0, f"{tag}: row {i} (cond {cond[i]:.3e}) is {ratio[i].max():.3e} of its bar from float64: " \
                                       f"ours {got[i]}, float64 {want[i]}"
    record(f"em solve npix {npix} nh {nh}: worst |error| / bar {worst:.3e}; beyond the float32 rounding {used:.3e} of the solve "
           f"term ({len(E.SOLVE_RIDGE_DAMPING)} (ridge, damping) x 2 calls)")


@pytest.mark.parametrize("nh,npix", [(5, 64), (32, 130)])
def test_a_ridge_past_1e300_skips_every_row(dev, nh, npix):
    S2, S1, cnt, F, planted = E.solve_case(npix, nh)
    buf, Fd = stats_buffer(dev, S2, S1, cnt), T(F, dev)
    want, skipped, _, _ = E.solve_rows((S2, S1, cnt), F, 1e301, 1.0)
    assert skipped.all() and np.array_equal(want, F.astype(np.float64))
    for in_place in (True, False):
        got, n = gpu_solve(dev, buf, Fd, npix, nh, 1e301, 1.0, in_place)
        assert np.array_equal(got.view(np.uint32), F.view(np.uint32))
        assert n in (None, npix)
