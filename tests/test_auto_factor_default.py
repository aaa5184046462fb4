"""The shipped default QFA.auto_factor_zabs = True (tests/conftest.py turns it off for the rest of the suite).

A plain zabs tensor handed to the model a second time, unchanged, is tested once for the reference loader's structure
(qfa_zabs_factor_f32) and from then on served by the factored-z kernels.  These tests run that default on the paths users get
with it -- repeated calls on one batch, graph capture, inference tensors, batches past the 65 535-block grid.y limit, training --
against the float64 oracle with the suite's bars (NLL 5e-6, TOL_G, predict 1e-4, sections 2e-5 against the zabs form).  Where
the factored kernels are meant to serve, the test shows that they did: the model's entry for the tensor holds the factors."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_l2
from qfa_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")
TOL_NLL = 5e-6
TOL_G = {"F": 1e-4, "Psi": 2e-5, "omega": 2e-5, "tau0": 1e-4, "c0": 1e-4, "beta": 1e-4}
GRID_Y = 65536                                   # past the grid.y limit whether it is 65 535 or 65 536 blocks


@pytest.fixture(autouse=True)
def default_on(monkeypatch):
    import qfa_amd.model as M
    monkeypatch.setattr(M, "AUTO_FACTOR_ZABS", True)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    return torch.tensor(x, dtype=torch.bool if x.dtype == bool else torch.float32, device=dev)


def setup(npix, nh, B, seed, dev):
    from qfa_amd import QFA, synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1)
    m = QFA(nb, nr, nh, dev, model_params=p)
    m.mu = T(mu, dev)
    assert m.auto_factor_zabs
    return m, p, mu, wav, b


def tensors(b, dev, key="delta"):
    return T(b[key], dev), T(b["error"], dev), T(b["zabs"], dev), T(b["mask"], dev)


def factored(m, zabs):
    ent = m._zf_seen.get(id(zabs))
    return ent is not None and isinstance(ent[2], tuple)


def check_forward(loss, g, p, b):
    from oracle import qfa_oracle as O
    ol, og = O.forward(p, b["delta"], b["error"], b["zabs"], b["mask"])
    assert abs(loss.item() - ol) <= TOL_NLL * abs(ol), (loss.item(), ol)
    for k in KEYS:
        ref = np.asarray(og[k], dtype=np.float64)
        ours = g[k].cpu().numpy()
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(ours), ~ok), k
        assert rel_l2(ours[ok], ref[ok]) < TOL_G[k], (k, rel_l2(ours[ok], ref[ok]))


def check_predict(out, p, mu, b, rows):
    from oracle import qfa_oracle as O
    ll, hm, hc, cont, unc = [x.cpu().numpy() for x in out]
    for s in rows:
        o = O.predict_single(p, mu, b["flux"][s], b["error"][s], b["zabs"][s], b["mask"][s])
        assert abs(ll[s] - o[0]) <= TOL_NLL * abs(o[0]), s
        assert rel_l2(hm[s], o[1]) < 1e-4, s
        assert rel_l2(hc[s], o[2]) < 1e-4, s
        assert np.max(np.abs(cont[s] - o[3])) / np.max(np.abs(o[3])) < 1e-4, s
        assert rel_l2(unc[s], o[4]) < 1e-4, s


def check_sections(m, acc, ref):
    from tools import parity_sections as PS
    for name, sl in PS.sections(m).items():
        a, r = acc[sl].double().cpu().numpy(), ref[sl].double().cpu().numpy()
        if name in ("cnt", "n_blue", "n_spectra"):
            assert np.array_equal(a, r), name
        elif a.size == 1:
            assert abs(a[0] - r[0]) <= 2e-4 * abs(r[0]) + 1e-6, (name, a, r)
        else:
            assert rel_l2(a, r) < 2e-5, (name, rel_l2(a, r))


# ------------------------------------------------------------------ A. graph capture of a plain zabs
@pytest.mark.parametrize("call", ["forward", "predict"])
def test_captured_call_reads_the_batch_copied_into_its_static_zabs(dev, call):
    """The usual torch capture pattern: eager warm-ups on static tensors (the second one factors them), capture, copy_ the next
    batch in, replay.  The replay must compute batch 2 (its own z_qso), not batch 1's cached factors."""
    import torch
    m, p, mu, wav, b1 = setup(640, 12, 130, 31, dev)
    from qfa_amd import synthetic
    b2 = synthetic.make_batch_numpy(p, mu, wav, m.Nb, 130, seed=77)
    assert not np.allclose(b1["zqso"], b2["zqso"])
    key = "delta" if call == "forward" else "flux"
    static = tensors(b1, dev, key)
    fn = m.forward if call == "forward" else m.predict
    for _ in range(3):
        fn(*static)
    assert factored(m, static[2]), "the eager warm-ups must have run the factored kernels"
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(*static)
    for dst, src in zip(static, tensors(b2, dev, key)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    if call == "forward":
        check_forward(out[0], out[1], p, b2)
    else:
        check_predict(out, p, mu, b2, range(0, 130, 13))
    # eager again on the refilled tensors: a new version, read as zabs, then factored from batch 2 itself
    for _ in range(2):
        res = fn(*static)
    assert factored(m, static[2])
    if call == "forward":
        check_forward(res[0], res[1], p, b2)
    else:
        check_predict(res, p, mu, b2, (0, 64, 129))


# ------------------------------------------------------------------ C. inference tensors
def test_inference_mode_tensors_are_read_as_zabs(dev):
    """A batch made under torch.inference_mode() has no version counter: it is never factored, and a second call must not
    fail.  accumulate, forward and predict twice each, against the oracle."""
    import torch
    m, p, mu, wav, b = setup(640, 12, 70, 41, dev)
    with torch.inference_mode():
        bt = tensors(b, dev)
        ft = tensors(b, dev, "flux")
        assert bt[2].is_inference()
        accs = [m.accumulate(*bt).clone() for _ in range(2)]
        for _ in range(2):
            loss, g = m.forward(*bt)
            check_forward(loss, g, p, b)
        for _ in range(2):
            check_predict(m.predict(*ft), p, mu, b, (0, 35, 69))
    assert id(bt[2]) not in m._zf_seen
    check_sections(m, accs[1], accs[0])
    loss, g = m._finalize(accs[1], True)
    check_forward(loss, g, p, b)
    # the default is live in this model: an ordinary tensor with the same values is factored on its second call
    z = bt[2].clone()
    for _ in range(2):
        loss, g = m.forward(bt[0].clone(), bt[1].clone(), z, bt[3].clone())
    assert factored(m, z)
    check_forward(loss, g, p, b)


# ------------------------------------------------------------------ D. batches past the grid.y limit
def _zabs_exact(zq1, ratio):
    return (zq1.double()[:, None] * ratio.double()[None, :] - 1.0).float().contiguous()


def test_zabs_factor_entry_point_past_the_grid_y_limit(dev):
    """qfa_zabs_factor_f32 on 8 x 65 536 + 43 rows (k_zfactor_check: 8 rows per block along grid.y): an exact zabs has no bad
    element; elements moved in the last rows -- past what 65 535 blocks of 8 rows reach, row B - 1 among them -- and a NaN are
    counted exactly."""
    import torch
    B, nb = 8 * GRID_Y + 43, 16
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    zq1 = 3.0 + 1.5 * torch.rand(B, generator=g, device=dev, dtype=torch.float64)
    ratio = torch.linspace(0.85, 0.999, nb, device=dev, dtype=torch.float64)
    z = _zabs_exact(zq1, ratio)
    out_zq1, out_ratio = torch.empty(B, device=dev), torch.empty(nb, device=dev)
    nbad = torch.full((1,), 12345, dtype=torch.int32, device=dev)

    def run(zz):
        rc = _lib.lib().qfa_zabs_factor_f32(C.c_void_p(zz.data_ptr()), B, nb, 4e-7, C.c_void_p(out_zq1.data_ptr()),
                                            C.c_void_p(out_ratio.data_ptr()), C.c_void_p(nbad.data_ptr()), _lib.current_stream(dev))
        assert rc == 0
        return int(nbad.item())

    assert run(z) == 0
    assert torch.equal(out_zq1, 1.0 + z[:, 0])
    moved = [(B - 1, 5), (B - 1, 15), (B - 20, 11), (8 * GRID_Y + 3, 2), (8 * (GRID_Y - 1) + 1, 7)]
    for r, c in moved:
        z[r, c] = (1.0 + z[r, c]) * (1.0 + 2e-6) - 1.0
    z[8 * GRID_Y + 40, 9] = float("nan")
    assert run(z) == len(moved) + 1


def test_repeated_batch_past_the_grid_y_limit_is_factored(dev):
    """accumulate twice on 8 x 65 536 + 43 spectra (N_pix 96, N_h 4): the second call runs the structure test over every row and
    then the factored kernels; against the zabs-kernel call section by section, and the per-spectrum NLL against the oracle on
    200 rows: every row past 8 x 65 535 (51) and 149 spread over the rest."""
    import torch
    from oracle import qfa_oracle as O
    from qfa_amd import QFA, synthetic
    npix, nh, B = 96, 4, 8 * GRID_Y + 43
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=61)
    d, e, _, mk, zq = synthetic.make_batch_torch(p, mu, wav, nb, B, 62, dev, masks=True, return_zq=True)
    z = ((1.0 + zq.double())[:, None] * torch.tensor(wav[:nb] / synthetic.LYA, device=dev)[None, :] - 1.0).float()
    torch.cuda.empty_cache()
    m = QFA(nb, nr, nh, dev, model_params=p)
    nll1, nll2 = torch.empty(B, device=dev), torch.empty(B, device=dev)
    acc1 = m.accumulate(d, e, z, mk, nll=nll1).clone()
    acc2 = m.accumulate(d, e, z, mk, nll=nll2).clone()
    assert factored(m, z)
    check_sections(m, acc2, acc1)
    # (per spectrum the float32 error scales with the summed terms, not with their sum: among half a million spectra some NLL
    # lies close to zero, so the relative bar is taken against the larger of |NLL| and the batch's median |NLL|)
    scale = float(nll1.abs().median())
    assert ((nll1 - nll2).abs() <= TOL_NLL * torch.clamp(nll1.abs(), min=scale)).all()
    past = 8 * (GRID_Y - 1)
    rows = np.unique(np.r_[np.linspace(0, past - 1, 149).astype(np.int64), np.arange(past, B)])
    assert len(rows) == 200 and (rows >= past).sum() == 51 and rows[-1] == B - 1
    idx = torch.tensor(rows, device=dev)
    dh, eh, zh, mh = (x.index_select(0, idx).cpu().numpy() for x in (d, e, z, mk))
    ours = nll2.index_select(0, idx).cpu().numpy()
    for j in range(len(rows)):
        ref, _ = O.nll_and_grads_single(p, dh[j], eh[j], zh[j], mh[j])
        assert abs(ours[j] - ref) <= TOL_NLL * max(abs(ref), scale), (int(rows[j]), ours[j], ref)


def test_mu_sums_past_the_grid_y_limit(dev):
    """qfa_mu_sums_f64 + qfa_mu_finish_f64 (k_mu_accumulate: 64 spectra per block along grid.y) on 64 x 65 536 + 197 spectra,
    a grid that starts below Ly-beta (two Lyman series), and pixels whose flux is valid while the error is -999 (masked in the
    numerator, counted in the denominator): raw and smoothed mean continuum against the float64 oracle."""
    import torch
    from oracle import qfa_oracle as O
    B, npix, window = 64 * GRID_Y + 197, 24, 16
    wav = np.linspace(1000.0, 1300.0, npix)
    nb = int(np.sum(wav < 1215.67))
    assert int(np.sum(wav[0] < O._LYMAN_LAM)) == 2                 # Ly-alpha and Ly-beta
    g = torch.Generator(device=dev)
    g.manual_seed(71)
    zq = 2.0 + 1.5 * torch.rand(B, generator=g, device=dev, dtype=torch.float64)
    flux = (0.5 + torch.rand(B, npix, generator=g, device=dev)).contiguous()
    err = (0.05 + 0.1 * torch.rand(B, npix, generator=g, device=dev)).contiguous()
    u = torch.rand(B, npix, generator=g, device=dev)
    flux[u < 0.03] = -999.0
    err[u < 0.03] = -999.0
    err[(u >= 0.03) & (u < 0.05)] = -999.0                         # valid flux, error -999
    flux[B - 1, 3] = -999.0                                          # the last row, past the old grid
    err[B - 2, 4] = -999.0
    wav_d = torch.tensor(wav, dtype=torch.float64, device=dev)
    scratch = torch.zeros(2 * npix, dtype=torch.float64, device=dev)
    raw = torch.empty(npix, dtype=torch.float64, device=dev)
    sm = torch.empty(npix, dtype=torch.float64, device=dev)
    h, st = _lib.lib(), _lib.current_stream(dev)
    assert h.qfa_mu_sums_f64(C.c_void_p(flux.data_ptr()), C.c_void_p(err.data_ptr()), C.c_void_p(zq.data_ptr()),
                             C.c_void_p(wav_d.data_ptr()), float(wav[0]), _lib.TAU_IDS["becker"], B, npix, nb, 0,
                             C.c_void_p(scratch.data_ptr()), st) == 0
    assert h.qfa_mu_finish_f64(C.c_void_p(scratch.data_ptr()), npix, window, C.c_void_p(raw.data_ptr()), C.c_void_p(sm.data_ptr()),
                               st) == 0
    raw, sm = raw.cpu().numpy(), sm.cpu().numpy()
    fh, eh, zh = flux.cpu().numpy(), err.cpu().numpy(), zq.cpu().numpy()
    del flux, err, u
    oraw, osm = O.mu_estimate(wav, fh, (fh != -999.0) & (eh != -999.0), zh, nb, window_len=window)
    assert np.max(np.abs(raw - oraw) / np.abs(oraw)) < 1e-10
    assert np.max(np.abs(sm - osm) / np.abs(osm)) < 1e-10


# ------------------------------------------------------------------ E. the default on the product paths
@pytest.mark.parametrize("npix,nh,B,flags", [(640, 12, 90, 0), (450, 24, 70, 0), (640, 16, 130, _lib.F_PASS2_PIXRES),
                                            (1100, 12, 200, 0)])          # (N_pix >= 1024, 128+ spectra: k_grads_t by default)
def test_forward_twice_on_one_batch(dev, npix, nh, B, flags):
    """forward on the same tensors twice: the second call is factored, both agree with the oracle"""
    m, p, mu, wav, b = setup(npix, nh, B, npix + nh, dev)
    m.flags = flags
    bt = tensors(b, dev)
    for i in range(2):
        loss, g = m.forward(*bt)
        check_forward(loss, g, p, b)
    assert factored(m, bt[2])


@pytest.mark.parametrize("npix,nh,B", [(640, 12, 70), (450, 24, 70)])
def test_predict_twice_on_one_batch(dev, npix, nh, B):
    m, p, mu, wav, b = setup(npix, nh, B, 3 * npix + nh, dev)
    ft = tensors(b, dev, "flux")
    for i in range(2):
        out = m.predict(*ft)
        check_predict(out, p, mu, b, (0, B // 3, B // 2, B - 1))
    assert factored(m, ft[2])


def test_forward_then_steps_on_one_batch_follow_the_oracle_adam_loop(dev):
    """the golden step's shape (shipped parameters, 128 spectra): forward, then four fused steps on the same tensors (factored
    from the second call on); parameters against the float64 oracle's Adam loop after every step"""
    import os
    from conftest import GOLDEN
    from oracle import qfa_oracle as O
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    p, mu = O.load_params_npz(os.path.join(GOLDEN, "model_parameters.npz"))
    wav, nb, nr = synthetic.wavelength_grid()
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 128, seed=91)
    m = QFA(nb, nr, p["F"].shape[1], dev, model_params=p)
    opt = Adam(params=m.parameters, device=dev, scheduler=step_scheduler(0.9, 10), learning_rate=1e-3, weight_decay=1e-1)
    bt = tensors(b, dev)
    loss, g = m.forward(*bt)
    check_forward(loss, g, p, b)
    ref = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    mo = {k: np.zeros_like(v) for k, v in ref.items()}
    vo = {k: np.zeros_like(v) for k, v in ref.items()}
    for it in range(4):
        loss = m.step(opt, *bt)
        assert factored(m, bt[2])
        ol, og = O.forward(ref, b["delta"], b["error"], b["zabs"], b["mask"])
        assert abs(loss.item() - ol) <= TOL_NLL * abs(ol), it
        ref, mo, vo = O.adam_update(mo, vo, 0, ref, og, O.step_lr(0, 1e-3, 0.9, 10), weight_decay=1e-1)
        ref = O.clip_params(ref)
        for k in KEYS:
            assert rel_l2(m.parameters[k].cpu().numpy(), ref[k]) < 1e-5, (it, k)


class CopyLoader:
    """A foreign loader that copy_s each batch into fixed buffers (and skips the copy when the buffers already hold it)"""

    def __init__(self, b, mu, batch_size, device):
        import torch
        self.t = {k: torch.tensor(b[k], device=device) for k in ("delta", "error", "zabs", "mask")}
        self.buf = {k: torch.empty_like(v[:batch_size]) for k, v in self.t.items()}
        self.mu, self.data_size, self.batch_size = mu, b["delta"].shape[0], batch_size
        self.cur, self.held = 0, None

    def rewind(self):
        self.cur = 0

    def have_next_batch(self):
        return self.cur < self.data_size

    def next_batch(self):
        s = self.cur
        self.cur = s + self.batch_size
        if self.held != s:
            for k in self.buf:
                self.buf[k].copy_(self.t[k][s:s + self.batch_size])
            self.held = s
        return tuple(self.buf[k] for k in ("delta", "error", "zabs", "mask"))


@pytest.mark.parametrize("n_batches", [1, 3])
def test_train_with_a_loader_that_copies_into_fixed_buffers(dev, tmp_path, n_batches):
    """QFA.train over CopyLoader for two epochs against the oracle loop: with one batch the buffers come back unchanged and are
    factored from the second step on; with three every step refills them (a new version: never the previous batch's factors)."""
    from test_train_loop import _oracle_train
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    wav, nb, nr = synthetic.wavelength_grid(320)
    p, mu = synthetic.mock_parameters(320, nb, 4, seed=23)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 8 * n_batches, seed=231)
    model = QFA(nb, nr, 4, dev, model_params=p)
    opt = Adam(model.parameters, dev, scheduler=step_scheduler(0.9, 1), learning_rate=1e-3, weight_decay=1e-1)
    dl = CopyLoader(b, mu, 8, dev)
    model.train(opt, dl, 2, str(tmp_path), save_interval=5, smooth_interval=5, quiet=True)
    ent = model._zf_seen[id(dl.buf["zabs"])]
    assert isinstance(ent[2], tuple) if n_batches == 1 else ent[2] == "seen"
    ref, _ = _oracle_train(p, b, 8, 2, 1e-3, 0.9, 1, 1e-1, 5)
    for k in KEYS:
        assert rel_l2(model.parameters[k].cpu().numpy(), ref[k]) < 2e-5, k


class SameTensorsLoader:
    """A foreign loader that hands out the same batch tensor objects every epoch"""

    def __init__(self, b, mu, batch_size, device):
        import torch
        n = b["delta"].shape[0]
        self.batches = [tuple(torch.tensor(b[k][s:s + batch_size], device=device) for k in ("delta", "error", "zabs", "mask"))
                        for s in range(0, n, batch_size)]
        self.mu, self.data_size, self.batch_size = mu, n, batch_size
        self.cur = 0

    def rewind(self):
        self.cur = 0

    def have_next_batch(self):
        return self.cur < len(self.batches)

    def next_batch(self):
        self.cur += 1
        return self.batches[self.cur - 1]


def test_step_graph_with_a_foreign_loader_matches_eager(dev, tmp_path):
    """test_train_with_step_graph_matches_eager's foreign loader with the default on and batch tensors that come back every
    epoch: the eager run serves them factored from epoch 2, StepGraph copies them into its buffers and replays; the same
    parameters, and the oracle loop's"""
    from test_train_loop import _oracle_train
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    wav, nb, nr = synthetic.wavelength_grid(320)
    p, mu0 = synthetic.mock_parameters(320, nb, 4, seed=5)
    b = synthetic.make_batch_numpy(p, mu0, wav, nb, 27, seed=51, masks=False)

    def run(use_graph):
        dl = SameTensorsLoader(b, mu0, 6, dev)
        model = QFA(nb, nr, 4, dev, model_params=p)
        opt = Adam(model.parameters, dev, scheduler=step_scheduler(0.5, 1), learning_rate=1e-3, weight_decay=1e-1)
        model.train(opt, dl, 3, str(tmp_path / ("g" if use_graph else "e")), quiet=True, smooth_interval=2, use_graph=use_graph)
        return model, dl, {k: model.parameters[k].cpu().numpy() for k in KEYS}

    me, dle, eager = run(False)
    assert all(factored(me, z) for _, _, z, _ in dle.batches)
    mg, dlg, graph = run(True)
    assert factored(mg, dlg.batches[-1][2])                          # (the short last batch runs eagerly)
    for k in KEYS:
        assert rel_l2(graph[k], eager[k]) < 1e-6, k
    ref, _ = _oracle_train(p, b, 6, 3, 1e-3, 0.5, 1, 1e-1, 2)
    for k in KEYS:
        assert rel_l2(eager[k], ref[k]) < 2e-5, k
