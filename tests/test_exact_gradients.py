"""The exact gradient mode on the GPU (QFA.exact_gradients, include/qfa_hip.h QFA_F_EXACT_GRAD): every pass-2 form against
the float64 closed form of tests/_exact_ref.py, its consistency with the reference mode, a directional derivative of the
float64 NLL, the fused finalize + Adam call, graph capture and the mode the packed buffer carries."""
import numpy as np
import pytest

import _exact_ref as X
from conftest import rel_l2
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")
TOL = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5}
TOL_SCAL = 1.5e-7          # of the sum of |terms| (the scalars are sums of terms that cancel)
TOL_LOSS = 5e-6
FULL_BARS = {"F": 8e-5, "Psi": 1e-5, "omega": 1e-5}      # reference mode's bars for one c3 launch (test_full_size_parity.py)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    return torch.tensor(x, dtype=torch.bool if x.dtype == bool else torch.float32, device=dev)


def setup(dev, npix, nh, B, seed, **kw):
    from qfa_amd import QFA, synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1, **kw)
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    zfac = (T((1.0 + b["zqso"].astype(np.float64)).astype(np.float32), dev),
            T((wav[:nb] / synthetic.LYA).astype(np.float32), dev))
    return m, p, b, zfac


def tensors(b, dev):
    return T(b["delta"], dev), T(b["error"], dev), T(b["zabs"], dev), T(b["mask"], dev)


def check_against_helper(loss, g, p, b, tag="", zabs=None):
    ol, og, ab = X.exact_forward(p, b["delta"], b["error"], b["zabs"] if zabs is None else zabs, b["mask"])
    assert abs(float(loss) - ol) <= TOL_LOSS * abs(ol), (tag, float(loss), ol)
    got = {k: np.asarray(g[k].cpu().numpy(), dtype=np.float64) for k in KEYS}
    for k in ("F", "Psi", "omega"):
        assert np.isfinite(got[k]).all(), (tag, k)
        assert rel_l2(got[k], og[k]) < TOL[k], (tag, k, rel_l2(got[k], og[k]))
    for k in ("tau0", "c0", "beta"):
        err = abs(float(got[k]) - float(og[k]))
        assert err <= TOL_SCAL * ab[k], (tag, k, float(got[k]), float(og[k]), err / ab[k])
    return og


FORMS = [  # (npix, nh, B, flags): every kernel that sums tau0 / c0 / beta, both input forms, both accumulation modes
    (200, 1, 40, 0), (300, 3, 70, _lib.F_PASS2_XDL), (400, 8, 96, _lib.F_PASS2_F32), (400, 8, 130, _lib.F_PASS2_PIXRES),
    (300, 12, 70, 0), (500, 12, 130, _lib.F_PASS2_XDL), (640, 16, 48, _lib.F_PASS2_F32), (600, 16, 200, _lib.F_PASS2_PIXRES),
    (97, 9, 33, _lib.F_PASS2_PIXRES), (450, 17, 70, 0), (300, 24, 40, _lib.F_S3_FAST), (450, 32, 70, 0), (31, 17, 5, 0),
]


@pytest.mark.parametrize("npix,nh,B,flags", FORMS)
@pytest.mark.parametrize("form", ["zabs", "factored"])
@pytest.mark.parametrize("det", [False, True])
def test_gpu_matches_closed_form(dev, npix, nh, B, flags, form, det):
    m, p, b, zfac = setup(dev, npix, nh, B, seed=npix + 3 * nh, dead_range=(npix // 4, npix // 4 + 3))
    m.exact_gradients, m.flags, m.deterministic = True, flags, det
    d, e, z, mk = tensors(b, dev)
    zf = None
    if form == "zabs":
        loss, g = m.forward(d, e, z, mk)
    else:
        loss, g = m.forward(d, e, None, mk, zfac=zfac)
        # the factored form's redshifts: 1 + z = zq1 x pix_ratio exactly (float64 products of the float32 factors)
        zf = np.outer(zfac[0].double().cpu().numpy(), zfac[1].double().cpu().numpy()) - 1.0
    og = check_against_helper(loss.item(), g, p, b, (npix, nh, B, flags, form, det), zabs=zf)
    # a pixel no spectrum observes: 0, where the reference mode gives 0/0 = NaN
    assert (g["F"][npix // 4].cpu().numpy() == 0).all() and g["Psi"][npix // 4].item() == 0
    assert (og["F"][npix // 4] == 0).all()


def test_auto_factored_zabs(dev):
    """the zabs tensor that comes back a second time is served by the factored-z kernels (QFA.auto_factor_zabs)"""
    m, p, b, _ = setup(dev, 600, 16, 200, seed=5)
    m.exact_gradients, m.auto_factor_zabs = True, True
    bt = tensors(b, dev)
    for call in range(3):
        loss, g = m.forward(*bt)
        check_against_helper(loss.item(), g, p, b, call)


def test_modes_agree_where_they_should(dev, shipped, grid):
    """same loss and raw gPsi / gOmega bits in both modes; tau0 moves the other way; the mode is a pure
    switch: on, then off again, reproduces a model that never turned it on, bit for bit"""
    import torch
    from qfa_amd import QFA, Adam, synthetic
    p, mu = shipped
    wav, nb, nr = grid
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 64, seed=17)
    bt = tensors(b, dev)

    def raw(exact):
        m = QFA(nb, nr, 8, dev, model_params=p)
        m.deterministic, m.exact_gradients = True, exact
        nll = torch.empty(64, device=dev)
        acc = m.accumulate(*bt, nll=nll).clone()
        return m, acc, nll, m._finalize(acc, False)

    mr, accr, nllr, (lr, gr) = raw(False)
    mx, accx, nllx, (lx, gx) = raw(True)
    assert torch.equal(nllr, nllx) and torch.equal(lr, lx)
    assert torch.equal(gr["Psi"], gx["Psi"]) and torch.equal(gr["omega"], gx["omega"])
    assert gr["tau0"].item() * gx["tau0"].item() < 0
    _, og, _ = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"], normalize=False)
    assert np.sign(gx["tau0"].item()) == np.sign(og["tau0"])
    # slot 5 and 6 of the packed buffer: the spectra of the launch, and of its exact-mode launches
    assert accr[-2].item() == 0 and accx[-2].item() == 64 and accx[-3].item() == 64 and accr[-3].item() == 64

    # a step in exact mode moves the parameters differently from a reference step; turning the mode off again gives
    # the reference step's update from there on, bit for bit (the mode lives in the buffer, nothing else is kept)
    def run(first):
        m = QFA(nb, nr, 8, dev, model_params=p)
        m.deterministic = True
        opt = Adam(m.parameters, dev, learning_rate=1e-3)
        m.exact_gradients = first
        m.step(opt, *bt)
        after1 = {k: getattr(m, k).clone() for k in KEYS}
        m.exact_gradients = False
        q = QFA(nb, nr, 8, dev, model_params={k: v.cpu().numpy() for k, v in after1.items()})
        q.deterministic = True
        qopt = Adam(q.parameters, dev, learning_rate=1e-3)
        for k in KEYS:
            qopt.m[k].copy_(opt.m[k])
            qopt.v[k].copy_(opt.v[k])
        m.step(opt, *bt)
        q.step(qopt, *bt)
        return after1, {k: getattr(m, k) for k in KEYS}, {k: getattr(q, k) for k in KEYS}
    r1, _, _ = run(False)
    x1, x2, fresh2 = run(True)
    assert not torch.equal(r1["F"], x1["F"]) and not torch.equal(r1["tau0"], x1["tau0"])
    for k in KEYS:
        assert torch.equal(x2[k], fresh2[k]), k

    # a model that turned the mode on for a forward call and off again computes what a fresh model computes
    m = QFA(nb, nr, 8, dev, model_params=p)
    m.deterministic = True
    m.exact_gradients = True
    m.forward(*bt)
    m.exact_gradients = False
    l1, g1 = m.forward(*bt)
    l0, g0 = mr.forward(*bt)
    assert torch.equal(l1, l0)
    for k in KEYS:
        assert torch.equal(torch.nan_to_num(g1[k], nan=7.0), torch.nan_to_num(g0[k], nan=7.0)), k


def test_never_observed_pixel_stays_finite_through_a_step(dev):
    import torch
    from qfa_amd import Adam
    m, p, b, _ = setup(dev, 300, 8, 50, seed=9)
    mk = b["mask"].copy()
    mk[:, 40] = False
    mk[:, 250] = False
    d, e, z, _ = tensors(b, dev)
    m.exact_gradients = True
    opt = Adam(m.parameters, dev, learning_rate=1e-3)
    for _ in range(2):
        loss = m.step(opt, d, e, z, T(mk, dev))
    assert torch.isfinite(loss).all()
    for k in KEYS:
        assert torch.isfinite(getattr(m, k)).all(), k


def test_mixed_modes_in_one_buffer_give_nan(dev):
    """two launches of different modes added into one buffer (ranks that disagree): NaN, in both finalize calls"""
    import torch
    from qfa_amd import Adam
    m, p, b, _ = setup(dev, 200, 8, 40, seed=4)
    bt = tensors(b, dev)
    acc = m._accum()
    m.exact_gradients = True
    m.accumulate(*bt, accum=acc)
    m.exact_gradients = False
    m.accumulate(*bt, accum=acc)
    loss, g = m._finalize(acc, True)
    assert torch.isnan(loss).all()
    for k in KEYS:
        assert torch.isnan(g[k]).all(), k
    opt = Adam(m.parameters, dev, learning_rate=1e-3)
    loss, new = opt.update_from_accum(m, acc, clip=m._clip_table())
    assert torch.isnan(loss).all()
    for k in KEYS:
        assert torch.isnan(new[k]).all(), k
    # two exact launches into one buffer: the sums of both, normalised by both
    acc2 = m._accum()
    m.exact_gradients = True
    m.accumulate(*bt, accum=acc2)
    m.accumulate(*bt, accum=acc2)
    l2, g2 = m._finalize(acc2, True)
    l1, g1 = m.forward(*bt)
    assert abs(l2.item() - l1.item()) <= 1e-6 * abs(l1.item())
    assert rel_l2(g2["F"].cpu().numpy(), g1["F"].cpu().numpy()) < 1e-6


def test_directional_derivative(dev):
    """<g_gpu, v> against the central difference of the float64 NLL, random directions v"""
    m, p, b, _ = setup(dev, 300, 6, 60, seed=31)
    m.exact_gradients = True
    _, g = m.forward(*tensors(b, dev))
    g = {k: g[k].double().cpu().numpy() for k in KEYS}
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    rng = np.random.default_rng(3)

    def loss(q):
        return X.exact_forward(q, b["delta"], b["error"], b["zabs"], b["mask"])[0]
    for trial in range(3):
        v = {k: rng.standard_normal(np.shape(p64[k])) * (np.abs(p64[k]).mean() + 1e-3) for k in KEYS}
        h = 1e-5
        qp = {k: p64[k] + h * v[k] for k in KEYS}
        qm = {k: p64[k] - h * v[k] for k in KEYS}
        fd = (loss(qp) - loss(qm)) / (2 * h)
        dot = sum(float(np.sum(g[k] * v[k])) for k in KEYS)
        assert abs(dot - fd) <= 1e-4 * abs(fd) + 1e-6, (trial, dot, fd)


def test_fused_finalize_adam_and_graph(dev):
    """exact mode: the fused finalize + Adam launch is bit-identical to finalize then Adam; a StepGraph replay equals the
    eager step, and turning the mode on re-captures"""
    import torch
    from qfa_amd import Adam, QFA
    from qfa_amd.model import StepGraph
    _, p, b, _ = setup(dev, 400, 12, 32, seed=8)
    bt = tensors(b, dev)
    nb = len(p["omega"])

    def model():
        m = QFA(nb, 400 - nb, 12, dev, model_params=p)
        m.deterministic, m.exact_gradients = True, True
        return m, Adam(m.parameters, dev, learning_rate=1e-3)
    m1, o1 = model()
    m1.step(o1, *bt)
    m2, o2 = model()
    loss, g = m2.forward(*bt)
    new = o2.update(m2.parameters, g, clip=m2._clip_table())
    for k in KEYS:
        assert torch.equal(getattr(m1, k), new[k]), k

    class Loader:
        def __init__(self):
            self.n = 0

        def next_batch(self):
            return bt

    m3, o3 = model()
    m4, o4 = model()
    sg = StepGraph(m3, o3, 32)
    m3.exact_gradients = False
    sg.run_next(Loader())                                     # reference mode: eager, then captured on the next call
    m4.exact_gradients = False
    m4.step(o4, *bt)
    key_ref = sg._key()
    m3.exact_gradients = m4.exact_gradients = True
    assert sg._key() != key_ref
    for _ in range(3):
        sg.run_next(Loader())
        m4.step(o4, *bt)
    torch.cuda.synchronize()
    assert sg.replays >= 1
    for k in KEYS:
        assert torch.equal(getattr(m3, k), getattr(m4, k)), k


def test_three_epochs_match_float64_adam(dev):
    """three epochs of one batch each (step, then the per-epoch Adam.step of QFA.train) against a float64 Adam loop on the
    closed form's gradients"""
    from oracle import qfa_oracle as O
    from qfa_amd import Adam
    m, p, b, _ = setup(dev, 300, 6, 40, seed=12)
    m.exact_gradients = True
    opt = Adam(m.parameters, dev, learning_rate=1e-3, weight_decay=1e-1)
    bt = tensors(b, dev)
    q = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    mm = {k: np.zeros_like(v) for k, v in q.items()}
    vv = {k: np.zeros_like(v) for k, v in q.items()}
    for epoch in range(3):
        i, lr = opt.i, float(opt.scheduled_lr)
        m.step(opt, *bt)
        _, g, _ = X.exact_forward(q, b["delta"], b["error"], b["zabs"], b["mask"])
        q, mm, vv = O.adam_update(mm, vv, i, q, g, lr, weight_decay=1e-1)
        q = O.clip_params(q)
        opt.step()
    for k in KEYS:
        assert rel_l2(getattr(m, k).cpu().numpy(), q[k]) < 2e-5, k


def test_full_size_c3(dev):
    """one launch of 25 000 spectra at c3's shape (4 000 pixels, N_h = 16) against the closed form"""
    from qfa_amd import QFA, synthetic
    npix, nh, B = 4000, 16, 25000
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=100)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=101)
    m = QFA(nb, nr, nh, dev, model_params=p)
    m.exact_gradients = True
    loss, g = m.forward(*tensors(b, dev))
    ol, og, ab = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"])
    got = {k: np.asarray(g[k].cpu().numpy(), dtype=np.float64) for k in KEYS}
    err = {"loss": abs(loss.item() - ol) / abs(ol)}
    err.update({k: rel_l2(got[k], og[k]) for k in ("F", "Psi", "omega")})
    err.update({k: abs(float(got[k]) - float(og[k])) / ab[k] for k in ("tau0", "c0", "beta")})
    print("exact full-size c3 errors:", err)
    # about 1.5x what this launch achieves, and no looser than the reference-mode full-size bars
    # (achieved: loss 9.6e-8, F 2.4e-6, Psi 3.0e-6, omega 6.9e-6, scalars 6.7-6.8e-8 of sum |terms|)
    bars = {"loss": 1.5e-7, "F": 4e-6, "Psi": 5e-6, "omega": 1e-5, "tau0": 1e-7, "c0": 1e-7, "beta": 1e-7}
    assert all(bars[k] <= FULL_BARS[k] for k in FULL_BARS)
    for k, v in err.items():
        assert v < bars[k], (k, v, bars[k])
