"""The exact gradient mode on the paths a user trains on: the resident, indexed input form (DeviceDataloader, QFA.train,
StepGraph), a 3-epoch QFA.train run and two data-parallel ranks on one GPU, against the float64 closed form of
tests/_exact_ref.py."""
import os
import sys

import numpy as np
import pytest

import _exact_ref as X
from conftest import REPO, rel_l2
from qfa_amd import _lib

pytestmark = pytest.mark.gpu
KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


RESIDENT = [
    # npix, nh, N, B, flags, zabs form
    (200, 16, 150, 70, 0, False),                                     # k_grads_x<16>
    (1913, 12, 900, 700, _lib.F_PASS2_PIXRES, False),                 # k_grads_t<16, .., ZF, IDX, EXACT>
    (1000, 8, 300, 130, _lib.F_PASS2_PIXRES, True),                   # k_grads_t<8, .., zabs, IDX, EXACT>
    (4000, 16, 2000, 1100, 0, False),                                 # the default pixel-resident path of a large batch
    (450, 32, 120, 70, 0, False),                                     # k_s12_x
]


@pytest.mark.parametrize("npix,nh,N,B,flags,zform", RESIDENT)
@pytest.mark.parametrize("det", [False, True])
def test_resident_form_matches_closed_form(dev, npix, nh, N, B, flags, zform, det):
    from test_exact_gradients import check_against_helper
    from test_resident_form import perm_rows, resident_set
    m, rb0, b, p, mu = resident_set(dev, npix, nh, N, seed=3 * npix + nh, with_zabs=zform)
    rb = rb0.with_rows(perm_rows(dev, N, B, seed=npix + B))
    m.flags, m.deterministic, m.exact_gradients = flags, det, True
    loss, g = m.forward(batch=rb)
    rows = rb.rows.cpu().numpy()
    if zform:
        z = b["zabs"][rows]
    else:
        z = np.outer(rb.zq1.double().cpu().numpy()[rows], rb.pix_ratio.double().cpu().numpy()) - 1.0
    sub = {k: b[k][rows] for k in ("delta", "error", "mask")}
    sub["zabs"] = b["zabs"][rows]
    check_against_helper(loss.item(), g, p, sub, (npix, nh, B, flags, zform, det), zabs=z)


def _oracle_train_exact(p, batches, N, batch_size, n_epochs, lr, alpha, step, wd, smooth_interval):
    """the reference's loop (QFA/model.py:183-231, as tests/test_train_loop.py plays it) on the closed form's gradients"""
    from oracle import qfa_oracle as O
    params = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    m = {k: np.zeros_like(v) for k, v in params.items()}
    v = {k: np.zeros_like(vv) for k, vv in params.items()}
    niter = N // batch_size
    i = 0
    for epoch in range(n_epochs):
        tot = 0.0
        for d, e, z, mk in batches:
            loss, g, _ = X.exact_forward(params, d, e, z, mk)
            tot += loss / niter
            params, m, v = O.adam_update(m, v, i, params, g, O.step_lr(i, lr, alpha, step), weight_decay=wd)
            params = O.clip_params(params)
        i += 1
        if tot < 0:
            params = O.smooth_params(params)
            break
        if (epoch + 1) % smooth_interval == 0:
            params = O.smooth_params(params)
    return params


def test_train_three_epochs_with_device_dataloader(dev, tmp_path):
    """QFA.train on a DeviceDataloader (resident batches, factored z) with exact gradients: the float64 trajectory"""
    from qfa_amd import QFA, Adam, step_scheduler, synthetic
    from qfa_amd.dataloader import DeviceDataloader
    npix, nh, N, bs = 320, 4, 22, 8
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=23)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, N, seed=231)
    b["error"] = b["error"] * 8.0                         # (noisier spectra: a positive epoch loss, no early stop)
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, batch_size=bs, device=dev, shuffle=False)
    dl.rewind()
    batches = []
    while dl.have_next_batch():
        d, e, z, mk = (x.cpu().numpy() for x in dl.next_batch())
        rows = np.arange(len(batches) * bs, len(batches) * bs + len(d))
        zq1 = (1.0 + b["zqso"][rows].astype(np.float64)).astype(np.float32).astype(np.float64)
        zf = np.outer(zq1, (wav[:nb] / synthetic.LYA).astype(np.float32).astype(np.float64)) - 1.0
        batches.append((d, e, zf, mk))
    dl.rewind()
    model = QFA(nb, nr, nh, dev, model_params=p)
    model.exact_gradients = True
    opt = Adam(model.parameters, dev, scheduler=step_scheduler(0.9, 1), learning_rate=1e-3, weight_decay=1e-1)
    model.train(opt, dl, 3, str(tmp_path), save_interval=10, smooth_interval=2, quiet=True)
    assert opt.i == 3
    ref = _oracle_train_exact(p, batches, N, bs, 3, 1e-3, 0.9, 1, 1e-1, 2)
    for k in KEYS:
        assert rel_l2(model.parameters[k].cpu().numpy(), ref[k]) < 2e-5, k


def _dp_case():
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(220)
    p, mu = synthetic.mock_parameters(220, nb, 4, seed=8)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, 7, seed=81, red_only=(5,), dead_range=(100, 104))
    return p, nb, b


def _worker(rank, world, port, q, modes):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from qfa_amd import QFA, Adam
    from qfa_amd.distributed import shard_bounds
    dev = torch.device("cuda:0")
    p, nb, b = _dp_case()
    m = QFA(nb, 220 - nb, 4, dev, model_params=p)
    m.enable_data_parallel()
    m.exact_gradients = modes[rank]
    lo, hi = shard_bounds(7, rank, world)
    t = [torch.tensor(b[k][lo:hi], device=dev) for k in ("delta", "error", "zabs", "mask")]
    opt = Adam(m.parameters, dev, learning_rate=1e-3, weight_decay=1e-1)
    try:
        m.check_replicas(opt)
        checked = "ok"
    except _lib.QFAHipError as exc:
        checked = str(exc)
    loss, g = m.forward(*t)
    m.step(opt, *t)
    out = (checked, loss.item(), {k: v.cpu().numpy() for k, v in g.items()},
           {k: v.cpu().numpy() for k, v in m.parameters.items()})
    gathered = [None, None]
    dist.all_gather_object(gathered, out)
    if rank == 0:
        q.put(gathered)
    dist.destroy_process_group()


def _run_dp(modes):
    import torch.multiprocessing as mp
    from test_data_parallel import _collect
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 7 * int(modes[1])) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, modes)) for r in range(2)]
    [pr.start() for pr in procs]
    gathered = _collect(procs, q, 300)
    [pr.join(60) for pr in procs]
    assert all(pr.exitcode == 0 for pr in procs)
    return gathered


def test_dp_two_ranks_exact_matches_single_process(dev):
    """two ranks on one GPU, both in exact mode: the all-reduced step equals the single process at the same global batch"""
    import torch
    from qfa_amd import QFA, Adam
    gathered = _run_dp((True, True))
    p, nb, b = _dp_case()
    assert gathered[0][0] == "ok" and gathered[1][0] == "ok"
    ol, og, ab = X.exact_forward(p, b["delta"], b["error"], b["zabs"], b["mask"])
    _, loss, g, newp = gathered[0]
    assert abs(loss - ol) <= 5e-6 * abs(ol)
    for k in ("F", "Psi", "omega"):
        assert np.isfinite(g[k]).all() and rel_l2(g[k], og[k]) < 1e-4, k
    for k in ("tau0", "c0", "beta"):
        assert abs(float(g[k]) - og[k]) <= 1.5e-7 * ab[k], k
    m = QFA(nb, 220 - nb, 4, dev, model_params=p)
    m.exact_gradients = True
    opt = Adam(m.parameters, dev, learning_rate=1e-3, weight_decay=1e-1)
    m.step(opt, *(torch.tensor(b[k], device=dev) for k in ("delta", "error", "zabs", "mask")))
    for k in KEYS:
        assert np.array_equal(gathered[0][3][k], gathered[1][3][k]), k          # the replicas stay identical
        assert rel_l2(gathered[0][3][k], m.parameters[k].cpu().numpy()) < 1e-6, k


def test_dp_mixed_modes_are_refused_and_give_nan():
    """ranks that disagree about the mode: check_replicas raises on both, and the all-reduced buffer finalises to NaN"""
    gathered = _run_dp((True, False))
    for r in range(2):
        checked, loss, g, newp = gathered[r]
        assert "exact_gradients" in checked, checked
        assert np.isnan(loss)
        for k in KEYS:
            assert np.isnan(g[k]).all(), (r, k)
