"""The EM update of F through the paths around the kernels: graph capture and replay of em_step, train(f_update="em") on a
DeviceDataloader against a float64 loop, two data-parallel ranks on one GPU, one large launch against float64 sums, and the
default training loop, which the feature must leave bit for bit as it was."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import _em_ref as E
from conftest import REPO, rel_l2

pytestmark = pytest.mark.gpu

KEYS = ("F", "Psi", "omega", "tau0", "c0", "beta")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    return torch.tensor(x, dtype=torch.bool if x.dtype == bool else torch.float32, device=dev)


def case(npix, nh, B, seed, **kw):
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=seed + 1, **kw)
    p = dict(p)
    p["F"] = np.random.default_rng(seed + 2).uniform(-0.5, 0.5, size=(npix, nh)).astype(np.float32)
    return wav, nb, p, mu, b


def test_graph_capture_and_replay_of_em_step(dev):
    import torch
    from qfa_amd import QFA
    npix, nh, B = 333, 8, 96
    wav, nb, p, mu, b1 = case(npix, nh, B, seed=3)
    b2 = case(npix, nh, B, seed=40)[4]
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    eager = QFA(nb, npix - nb, nh, dev, model_params=p)
    static = [T(b1[k], dev) for k in ("delta", "error", "zabs", "mask")]
    m.em_step(*static)                                                  # warm-up: buffers allocated outside the capture
    m.F = T(p["F"], dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            loss = m.em_step(*static)
    torch.cuda.current_stream().wait_stream(side)
    for b in (b1, b2, b1):
        for t, k in zip(static, ("delta", "error", "zabs", "mask")):
            t.copy_(T(b[k], dev))
        g.replay()
        want = eager.em_step(*[T(b[k], dev) for k in ("delta", "error", "zabs", "mask")])
        torch.cuda.synchronize()
        assert torch.equal(loss, want) and torch.equal(m.F, eager.F)


def test_three_epochs_of_em_training_match_a_float64_loop(dev, tmp_path):
    import torch
    from oracle import qfa_oracle as O
    from qfa_amd import QFA, Adam
    from qfa_amd.dataloader import DeviceDataloader
    npix, nh, N, bs = 300, 6, 80, 40
    wav, nb, p, mu, b = case(npix, nh, N, seed=12)
    dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, bs, dev, shuffle=False)
    batches = []
    dl.rewind()
    while dl.have_next_batch():
        batches.append([t.cpu().numpy() for t in dl.next_batch()])
    m = QFA(nb, npix - nb, nh, dev, model_params=p)
    opt = Adam(m.parameters, dev, learning_rate=1e-3, weight_decay=1e-1)
    m.train(opt, dl, 3, output_dir=str(tmp_path), quiet=True, smooth_interval=100, save_interval=100, f_update="em")
    assert m.em_running is not None
    q = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    rest = [k for k in KEYS if k != "F"]
    mm = {k: np.zeros_like(q[k]) for k in rest}
    vv = {k: np.zeros_like(q[k]) for k in rest}
    for epoch in range(3):
        for d, e, z, mk in batches:
            _, g = O.forward(q, d, e, z, mk)
            new, mm, vv = O.adam_update(mm, vv, epoch, {k: q[k] for k in rest}, {k: g[k] for k in rest}, 1e-3, weight_decay=1e-1)
            q.update(O.clip_params(dict(q, **new)))
            q["F"], _ = E.em_update(q["F"], E.em_statistics(q, d, e, z, mk))
    for k in KEYS:
        err = rel_l2(getattr(m, k).cpu().numpy(), q[k])
        print("train", k, err)
        assert err < (1e-4 if k == "F" else 2e-5), (k, err)
    # the running statistics travel with the checkpoint
    path = os.path.join(str(tmp_path), "ck.npz")
    m.save_checkpoint(path, opt)
    m2 = QFA(nb, npix - nb, nh, dev)
    m2.load_checkpoint(path)
    assert torch.equal(m2.em_running.buf, m.em_running.buf) and torch.equal(m2.F, m.F)


def test_default_training_is_untouched_by_the_feature(dev, tmp_path):
    """the default loop twice -- once on a model that has had em_statistics called and discarded: the same bits"""
    import torch
    from qfa_amd import QFA, Adam
    from qfa_amd.dataloader import DeviceDataloader
    npix, nh, N, bs = 333, 8, 96, 32
    wav, nb, p, mu, b = case(npix, nh, N, seed=21)

    def run(touch):
        dl = DeviceDataloader(b["flux"], b["error"], b["zqso"], wav, bs, dev, shuffle=False)
        m = QFA(nb, npix - nb, nh, dev, model_params=p)
        if touch:
            dl.rewind()
            m.em_statistics(batch=dl.next_batch_rows())
            m.em_statistics(*[T(b[k], dev) for k in ("delta", "error", "zabs", "mask")])
        opt = Adam(m.parameters, dev, learning_rate=1e-3, weight_decay=1e-1)
        m.train(opt, dl, 2, output_dir=str(tmp_path), quiet=True, smooth_interval=100, save_interval=100)
        assert m.em_running is None
        return m
    a, c = run(False), run(True)
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(c, k)), k


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from qfa_amd import QFA
    from qfa_amd.distributed import shard_bounds
    dev = torch.device("cuda:0")
    wav, nb, p, mu, b = case(220, 4, 37, seed=8, dead_range=(100, 104))
    m = QFA(nb, 220 - nb, 4, dev, model_params=p)
    m.enable_data_parallel()
    lo, hi = shard_bounds(37, rank, world)
    loss = m.em_step(*[torch.tensor(b[k][lo:hi], device=dev) for k in ("delta", "error", "zabs", "mask")])
    out = (loss.item(), m.F.cpu().numpy())
    gathered = [None, None]
    dist.all_gather_object(gathered, out)
    if rank == 0:
        q.put(gathered)
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu(dev):
    from qfa_amd import QFA
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [pr.start() for pr in procs]
    gathered = q.get(timeout=300)
    [pr.join(60) for pr in procs]
    assert all(pr.exitcode == 0 for pr in procs)
    (l0, F0), (l1, F1) = gathered
    assert l0 == l1 and np.array_equal(F0, F1)                          # both replicas bit-equal
    wav, nb, p, mu, b = case(220, 4, 37, seed=8, dead_range=(100, 104))
    m = QFA(nb, 220 - nb, 4, dev, model_params=p)
    loss = m.em_step(*[T(b[k], dev) for k in ("delta", "error", "zabs", "mask")])
    assert abs(loss.item() - l0) <= 1e-6 * abs(l0)
    assert rel_l2(F0, m.F.cpu().numpy()) <= 1e-5                        # the one-process result, to rounding
    assert np.array_equal(F0[100:104], p["F"][100:104])


# S2 / S1 of one launch of 25 000 c3-shape spectra against float64 sums, rel-L2: measured 4.53e-8 / 4.29e-8 on one MI355X
# (DESIGN.md section 14); the bars are 50 % above that, the margin of deterministic arithmetic
LARGE_BAR = {"S2": 6.8e-8, "S1": 6.5e-8}


def _large_chunk(args):
    pfile, path, a, c = args
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _em_ref as E2
    p = dict(np.load(pfile))
    arr = {k: np.load(os.path.join(path, k + ".npy"), mmap_mode="r") for k in ("delta", "error", "zabs", "mask")}
    st = E2.em_statistics(p, arr["delta"][a:c], arr["error"][a:c], arr["zabs"][a:c], arr["mask"][a:c])
    return st["S2"], st["S1"], st["cnt"], st["nll_sum"]


def test_one_large_launch(dev, tmp_path):
    """25 000 spectra at c3's shape in one launch against float64 sums over the same spectra (worker processes on the host
    cores, as tools/oracle_pool.py runs its sums).  Measured: S2 4.53e-8, S1 4.29e-8, F after the update 6.0e-8."""
    import torch
    from qfa_amd import QFA, synthetic
    npix, nh, B = 4000, 16, 25000
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=3)
    p = dict(p)
    p["F"] = np.random.default_rng(5).uniform(-0.5, 0.5, size=(npix, nh)).astype(np.float32)
    d, e, z, mk = synthetic.make_batch_torch(p, mu, wav, nb, B, 33, dev)
    m = QFA(nb, nr, nh, dev, model_params=p)
    st = m.em_statistics(d, e, z, mk)
    F0 = m.F.clone()
    m.em_update_F(st)
    scratch = str(tmp_path)
    for k, t in (("delta", d), ("error", e), ("zabs", z), ("mask", mk)):
        np.save(os.path.join(scratch, k + ".npy"), t.cpu().numpy())
    pfile = os.path.join(scratch, "params.npz")
    np.savez(pfile, **{k: np.asarray(v) for k, v in p.items()})
    jobs = [(pfile, scratch, a, min(a + 250, B)) for a in range(0, B, 250)]
    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 1))
    with mp.get_context("spawn").Pool(workers) as pool:
        res = pool.map(_large_chunk, jobs)
    ref = {"S2": sum(r[0] for r in res), "S1": sum(r[1] for r in res), "cnt": sum(r[2] for r in res)}
    e2, e1 = rel_l2(st.S2.double().cpu().numpy(), ref["S2"]), rel_l2(st.S1.double().cpu().numpy(), ref["S1"])
    want, _ = E.em_update(p["F"], ref)
    ef = rel_l2(m.F.double().cpu().numpy(), want)
    print("large launch: S2", e2, "S1", e1, "F", ef)
    assert np.array_equal(st.cnt.cpu().numpy().astype(np.float64), ref["cnt"])
    assert ef <= 1e-4
    assert max(LARGE_BAR.values()) <= 1e-4
    assert e2 <= LARGE_BAR["S2"] and e1 <= LARGE_BAR["S1"], (e2, e1)
