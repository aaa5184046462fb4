"""The closed-form EM update of F on the GPU (QFA.em_statistics / em_update_F / em_step; include/qfa_hip.h qfa_em_*) against
the float64 closed form of tests/_em_ref.py: the statistics at every N_h class, ragged pixel axes, batch sizes from 1 to 4 096
and every input form; their determinism and symmetry; the identity with the exact-gradient mode on the device; the update;
monotone descent."""
import numpy as np
import pytest

import _em_ref as E
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_STAT = 2e-5        # S2, S1 (rel-L2): the project's bar for learned parameters; these sums do not cancel
TOL_LOSS = 5e-6        # the project's NLL bar
TOL_F = 1e-4           # quantities that pass through a k x k solve


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    return torch.tensor(x, dtype=torch.bool if x.dtype == bool else torch.float32, device=dev)


def setup(dev, npix, nh, B, seed, random_F=True, junk=True, batch_seed=None, plant=None):
    """model + numpy batch (_em_ref.em_inputs, which the CPU side shares): masks on, one red-only spectrum, one pixel range
    masked in every spectrum, NaN / inf / -999 under the masks; F ~ U(-0.5, 0.5) like random_init_func"""
    from qfa_amd import QFA
    p, b, dead, wav, nb, zf = E.em_inputs(npix, nh, B, seed, random_F=random_F, junk=junk, batch_seed=batch_seed, plant=plant)
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    zfac = (T(zf[0], dev), T(zf[1], dev))
    return m, p, b, zfac, dead


def tensors(b, dev):
    return T(b["delta"], dev), T(b["error"], dev), T(b["zabs"], dev), T(b["mask"], dev)


def check_stats(st, ref, tag):
    S2 = st.S2.double().cpu().numpy(); S1 = st.S1.double().cpu().numpy()
    e2, e1 = rel_l2(S2, ref["S2"]), rel_l2(S1, ref["S1"])
    loss = float(st.loss.item()); rl = ref["nll_sum"] / ref["n"]
    print("stats", tag, "S2", e2, "S1", e1, "loss", loss, rl)
    assert np.isfinite(S2).all() and np.isfinite(S1).all(), tag
    assert e2 <= TOL_STAT and e1 <= TOL_STAT, (tag, e2, e1)
    assert np.array_equal(st.cnt.cpu().numpy().astype(np.float64), ref["cnt"]), tag
    assert abs(loss - rl) <= TOL_LOSS * abs(rl), (tag, loss, rl)
    assert float(st.tail[1].item()) == ref["n"] and float(st.tail[2].item()) == 0.0 and float(st.tail[3].item()) == 0.0
    import torch
    assert torch.equal(st.S2, st.S2.transpose(1, 2)), tag            # symmetric bit for bit


SHAPES = E.SHAPES      # (npix, nh, B): every N_h class, ragged pixel axes (N_pix = 1 included), B from 1 to 4 096


@pytest.mark.parametrize("npix,nh,B", SHAPES)
@pytest.mark.parametrize("form", ["zabs", "factored"])
def test_statistics_match_closed_form(dev, npix, nh, B, form):
    import torch
    m, p, b, zfac, dead = setup(dev, npix, nh, B, seed=npix + 5 * nh)
    d, e, z, mk = tensors(b, dev)
    zf = b["zabs"]
    nll = torch.empty(B, device=dev)
    if form == "zabs":
        st = m.em_statistics(d, e, z, mk, nll=nll)
        st2 = m.em_statistics(d, e, z, mk)
    else:
        st = m.em_statistics(d, e, None, mk, zfac=zfac, nll=nll)
        st2 = m.em_statistics(d, e, None, mk, zfac=zfac)
        zf = np.outer(zfac[0].double().cpu().numpy(), zfac[1].double().cpu().numpy()) - 1.0
    ref = E.em_statistics(p, b["delta"], b["error"], zf, b["mask"])
    check_stats(st, ref, (npix, nh, B, form))
    assert torch.equal(st.buf, st2.buf)                              # two calls, the same bits
    assert np.allclose(nll.double().cpu().numpy(), ref["nll"], rtol=2e-5, atol=1e-4)
    if dead is not None:
        assert (st.cnt[dead[0]:dead[1]] == 0).all() and (st.S2[dead[0]:dead[1]] == 0).all() and (st.S1[dead[0]:dead[1]] == 0).all()


def test_statistics_add_into_a_given_buffer(dev):
    import torch
    m, p, b, zfac, _ = setup(dev, 203, 8, 96, seed=11)
    bt = tensors(b, dev)
    st = m.em_statistics(*bt)
    one = st.clone()
    m.em_statistics(*bt, stats=st)
    assert torch.allclose(st.buf, 2 * one.buf, rtol=1e-6, atol=0)
    assert torch.equal(st.S2, st.S2.transpose(1, 2))
    assert float(st.tail[1].item()) == 192.0


def test_custom_tau_callable(dev):
    """the host-supplied A_blue form (a tau callable evaluated on zabs by the caller)"""
    import torch
    from qfa_amd import QFA, utils
    m, p, b, _, _ = setup(dev, 203, 8, 70, seed=13)
    m2 = QFA(m.Nb, m.Nr, 8, dev, tau=lambda z: utils.tau(z, which="becker"), model_params=p)
    assert m2._tau_callable is not None
    st = m2.em_statistics(*tensors(b, dev))
    check_stats(st, E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"]), "A_blue")


@pytest.mark.parametrize("zform", ["factored", "zabs"])
def test_resident_form_is_bit_equal_to_the_gathered_batch(dev, zform):
    import torch
    from qfa_amd.resident import ResidentBatch
    npix, nh, N, B, stride = 333, 8, 300, 130, 352
    m, p, b, zfac, _ = setup(dev, npix, nh, N, seed=21)
    def pad(a, dt, fill):
        out = torch.full((N, stride), fill, dtype=dt, device=dev)
        out[:, :npix] = a
        return out
    d, e, z, mk = tensors(b, dev)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:B].to(torch.int32).to(dev)
    rb = ResidentBatch(None, pad(d, torch.float32, 0.0), pad(e, torch.float32, 0.0), pad(mk, torch.bool, False),
                       zfac[0] if zform == "factored" else None, zfac[1] if zform == "factored" else None, rows, npix, m.Nb,
                       zabs=z if zform == "zabs" else None)
    st = m.em_statistics(batch=rb)
    (gd, ge, gz, gm), gzf = rb.materialize()
    st2 = m.em_statistics(gd, ge, gz, gm, zfac=gzf)
    assert torch.equal(st.buf, st2.buf)
    idx = rows.long().cpu().numpy()
    zf = b["zabs"][idx] if zform == "zabs" else np.outer(zfac[0].double().cpu().numpy()[idx], zfac[1].double().cpu().numpy()) - 1.0
    check_stats(st, E.em_statistics(p, b["delta"][idx], b["error"][idx], zf, b["mask"][idx]), ("resident", zform))


@pytest.mark.parametrize("npix,nh,B", [(203, 4, 70), (333, 8, 257), (501, 16, 130), (211, 17, 33), (130, 32, 300)])
def test_identity_with_exact_gradient_on_the_device(dev, npix, nh, B):
    """oracle-free: S2 f - S1 from em_statistics against accumulate in exact mode (gF sums = -accF), random-init F"""
    m, p, b, zfac, _ = setup(dev, npix, nh, B, seed=npix + nh)
    bt = tensors(b, dev)
    st = m.em_statistics(*bt)
    m.exact_gradients = True
    acc = m.accumulate(*bt)
    gF = -acc[:npix * nh].view(npix, nh).double()
    S2f = torch_einsum(st.S2.double(), m.F.double())
    diff = (S2f - st.S1.double() - gF).norm().item()
    scale = S2f.norm().item() + st.S1.double().norm().item()
    print("identity", (npix, nh, B), diff / scale)
    assert diff <= 2e-5 * scale, (diff, scale)


def torch_einsum(S2, F):
    import torch
    return torch.einsum("iab,ib->ia", S2, F)


@pytest.mark.parametrize("npix,nh,B", [(37, 1, 9), (203, 4, 70), (333, 8, 257), (501, 16, 130), (211, 17, 60), (130, 32, 300)])
def test_update_matches_float64(dev, npix, nh, B):
    import torch
    m, p, b, zfac, dead = setup(dev, npix, nh, B, seed=2 * npix + nh)
    bt = tensors(b, dev)
    ref = E.em_statistics(p, b["delta"], b["error"], b["zabs"], b["mask"])
    cond = max(np.linalg.cond(ref["S2"][i]) for i in range(npix) if ref["cnt"][i] > 0)
    st = m.em_statistics(*bt)
    F0 = m.F.clone()
    want, wskip = E.em_update(p["F"], ref)
    for ridge, damping in ((0.0, 1.0), (0.3, 1.0), (0.0, 0.4), (2.0, 0.7)):
        m.F = F0.clone()
        n = m.em_update_F(st, ridge=ridge, damping=damping)           # in place: F_out aliases F
        wantrd, wskip = E.em_update(p["F"], ref, ridge, damping)
        err = rel_l2(m.F.double().cpu().numpy(), wantrd)
        print("update", (npix, nh, B, ridge, damping), err, "cond", cond)
        assert err <= TOL_F, (ridge, damping, err)
        assert n == wskip == int((ref["cnt"] == 0).sum())
        skipped = torch.tensor(ref["cnt"] == 0, device=dev)
        assert torch.equal(m.F[skipped], F0[skipped])                 # bit-equal to the old F
    # out of place through the C-ABI: F untouched
    import ctypes as C
    from qfa_amd import _lib
    m.F = F0.clone()
    out = torch.full_like(F0, 7.0)
    _lib.check(_lib.lib().qfa_em_update_f_f32(C.c_void_p(st.buf.data_ptr()), C.c_void_p(m.F.data_ptr()), npix, nh, 0.0, 1.0,
                                              C.c_void_p(out.data_ptr()), None, _lib.current_stream(dev)), "update")
    assert torch.equal(m.F, F0) and rel_l2(out.double().cpu().numpy(), want) <= TOL_F


def test_non_positive_pivot_rows_are_kept_and_counted(dev):
    import torch
    m, p, b, zfac, _ = setup(dev, 64, 4, 40, seed=5)
    st = m.em_statistics(*tensors(b, dev))
    base = int((st.cnt == 0).sum().item())
    st.S2[7] = -st.S2[7]
    st.S2[9, 2, 2] = float("nan")
    F0 = m.F.clone()
    assert m.em_update_F(st) == base + 2
    assert torch.equal(m.F[7], F0[7]) and torch.equal(m.F[9], F0[9]) and torch.isfinite(m.F).all()
    assert not torch.equal(m.F[8], F0[8])


@pytest.mark.parametrize("shape", ["c2", "c3"])
def test_monotone_descent_on_one_batch(dev, shape):
    """four em_steps from random_init_func values on one fixed batch: the loss never rises, and the first step delivers at
    least half of the fall the float64 closed form predicts for it"""
    import torch
    from qfa_amd import QFA, synthetic
    npix, nh = (2000, 8) if shape == "c2" else (4000, 16)
    B = 2000
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=31)
    d, e, z, mk = synthetic.make_batch_torch(p, mu, wav, nb, B, 32, dev)
    torch.manual_seed(7)
    m = QFA(nb, nr, nh, dev)
    p0 = {k: v.double().cpu().numpy() for k, v in m.parameters.items()}
    losses = [m.em_step(d, e, z, mk).item() for _ in range(4)]
    losses.append(m.em_statistics(d, e, z, mk).loss.item())
    # float64 prediction of the first step on a subset of the spectra is not the same batch: use the whole batch, in chunks
    dn, en, zn, mn = (t.cpu().numpy() for t in (d, e, z, mk))
    ref = E.em_statistics(p0, dn, en, zn, mn)
    newF, _ = E.em_update(p0["F"], ref)
    q = dict(p0); q["F"] = newF
    l0, l1 = ref["nll_sum"] / B, E.em_statistics(q, dn, en, zn, mn)["nll_sum"] / B
    print("descent", shape, losses, "float64", l0, l1)
    assert all(losses[k + 1] <= losses[k] for k in range(4)), losses
    assert abs(losses[0] - l0) <= TOL_LOSS * abs(l0)
    assert losses[0] - losses[1] >= 0.5 * (l0 - l1) > 0
