"""What the GPU tests of the forest statistics share (tests/test_forest.py, test_p1d.py, test_p1d_band.py, test_xi.py, test_flux_pdf.py,
test_variance.py): the device fixture, the inputs, one call of a segment statistic's C entry point by hand, the redshift forms on
identical z, the loop of the refusal tests, and the loader / two-rank / command-line scaffolds.  A plain module: the test modules
import what they use by name (the `dev` fixture too).  The comparisons and their bars stay with the tests and the `_*_ref` ports."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import _forest_ref
import _p1d_ref

TB_BINS = (1.5, 0.125, 17)                                    # z of `geometry` lies in [1.54, 3.5]
F_ZERO, F_SYNC = 0x80, 0x20                                   # QFA_F_ZERO_ACCUM, QFA_F_SYNC
OUT_FILL, STACK_FILL = -7, 3.0                                # what a fresh output of `call_segment` holds


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dev):
    import torch
    x = np.asarray(x)
    if x.dtype == bool:
        return torch.tensor(x, dtype=torch.bool, device=dev)
    if x.dtype == np.int32:
        return torch.tensor(x, dtype=torch.int32, device=dev)
    return torch.tensor(x, dtype=torch.float32, device=dev)


def geometry(npix, nb, nh, B, S, seed, masks=True):
    """mu ~ 1, small F, h ~ N(0, 1): c stays in [0.5, 2]; z = zq1 ratio - 1 with zq1 in [3, 4.5], ratio log-spaced 1030 .. 1215 A"""
    rng = np.random.default_rng(seed)
    p = {"F": (rng.uniform(-1, 1, (npix, nh)) * 0.1 / np.sqrt(nh)).astype(np.float32),
         "Psi": np.full(npix, 0.01, np.float32), "omega": np.full(nb, 0.1, np.float32),
         "tau0": np.float32(0.02), "c0": np.float32(0.3), "beta": np.float32(2.0)}
    mu = (1.0 + 0.1 * np.sin(np.arange(npix) / 7.0)).astype(np.float32)
    ratio = (10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32)
    zq1 = rng.uniform(3.0, 4.5, B).astype(np.float32)
    zfac = _forest_ref.z_factored(zq1, ratio)                        # what the factored form bins with
    zabs = (zq1.astype(np.float64)[:, None] * ratio.astype(np.float64)[None, :] - 1.0 + rng.normal(0, 1e-4, (B, nb))).astype(np.float32)
    h = np.clip(rng.normal(0, 1, (B, S, nh)), -3, 3).astype(np.float32)
    error = rng.uniform(0.01, 0.1, (B, npix)).astype(np.float32)
    flux = (rng.uniform(0.0, 1.0, (B, npix)) * mu[None, :] + error * rng.normal(0, 1, (B, npix))).astype(np.float32)
    unc = rng.uniform(0.01, 0.05, (B, npix)).astype(np.float32)
    mask = rng.random((B, npix)) > 0.2 if masks else None
    return {"p": p, "mu": mu, "ratio": ratio, "zq1": zq1, "zfac": zfac, "zabs": zabs, "h": h, "error": error, "flux": flux,
            "unc": unc, "mask": mask}


def make_model(dev, g, nb, nr, nh):
    from qfa_amd import QFA
    m = QFA(nb, nr, nh, dev, model_params=g["p"])
    m.mu = T(g["mu"], dev)
    return m


def forest_case(dev, B, S, nb, seed, nh=4):
    """trans / ivar (B, S, nb) as qfa_forest_f32 writes them, on the device and as numpy, with the geometry they came from"""
    npix = nb + 20
    g = geometry(npix, nb, nh, B, S, seed)
    m = make_model(dev, g, nb, npix - nb, nh)
    tr, iv, _ = m.forest(T(g["flux"], dev), T(g["error"], dev), T(g["zabs"], dev), T(g["mask"], dev), h=T(g["h"], dev), cont_min=0.05)
    tbar = np.random.default_rng(seed + 1).uniform(0.3, 0.9, (S, TB_BINS[2])).astype(np.float32)
    return g, m, tr, iv, tbar


def case_shape(rows, L, nseg, p_lo):
    """B, S, nb, min_used and the seed of a (rows, L, nseg, p_lo) row of a module's CASES"""
    S = 3 if rows % 3 == 0 and rows > 3 else 1
    return rows // S, S, p_lo + nseg * L + 3, max(1, int(np.ceil(0.78 * L))), 1000 + L


def call_segment(name, dev, trans, ivar, tbar, prm, own=None, outputs=(), *, size=(), stack_width, zabs=None, zq1=None, ratio=None,
                 rows=None, flags=F_ZERO, outs=None, stack=None, expect=0, ws_bytes=None, nrows=None):
    """``name``_f32 by hand on device tensors, its workspace sized by ``name``_workspace_bytes(..., *size).  prm = (p_lo, L, nseg,
    min_used, (z0, dz, nz)); ``own``: the statistic's parameter struct (None: the call has none); ``outputs``: (letter, the shape behind
    (B, S, nseg), the name of its torch dtype) of every per-segment output in the call's order; ``outs``: the letters of the outputs to
    pass, "s" = the stack (S, nz, ``stack_width``), default all -- the others go in as NULL.  Fresh outputs hold OUT_FILL, a fresh stack STACK_FILL.
    ``ws_bytes``: the workspace size to report instead of the computed one; ``nrows``: B instead of trans' own.  Asserts the status
    ``expect`` and returns the outputs and the stack as numpy (None where NULL went in)."""
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    B, S, Nb = trans.shape
    B = B if nrows is None else nrows
    p_lo, L, nseg, min_used, bins = prm
    outs = "".join(o[0] for o in outputs) + "s" if outs is None else outs
    tb = T(tbar, dev).reshape(-1, TB_BINS[2]).contiguous()
    addr = lambda t: None if t is None else t.data_ptr()
    bs = _lib.Batch()
    bs.zabs, bs.zq1, bs.pix_ratio, bs.rows, bs.row_stride = addr(zabs), addr(zq1), addr(ratio), addr(rows), 0
    pp = _lib.P1DParams(TB_BINS[0], TB_BINS[1], TB_BINS[2], int(tb.shape[0]), p_lo, L, nseg, min_used, bins[0], bins[1], bins[2])
    made = [torch.full((B, S, nseg) + tuple(tail), OUT_FILL, dtype=getattr(torch, dtype), device=dev) if k in outs else None
            for k, tail, dtype in outputs]
    if stack is None and "s" in outs:
        stack = torch.full((S, bins[2], stack_width), STACK_FILL, dtype=torch.float64, device=dev)
    need = getattr(lib, name + "_workspace_bytes")(B * S, S, Nb, L, nseg, bins[2], *size)
    if expect == 0:
        assert need > 0
    nbytes = ws_bytes if ws_bytes is not None else (need or 1 << 16)   # (a refused shape has no size: the check under test comes first)
    ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    st = getattr(lib, name + "_f32")(
        C.c_void_p(trans.data_ptr()), C.c_void_p(ivar.data_ptr()), C.byref(bs), C.c_void_p(tb.data_ptr()), B, S, Nb, C.byref(pp),
        *(() if own is None else (C.byref(own),)), flags, *(C.c_void_p(addr(o)) for o in made), C.c_void_p(addr(stack)),
        C.c_void_p(ws.data_ptr()), nbytes, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert st == expect, st
    return tuple(None if x is None else x.cpu().numpy() for x in made + [stack])


def call_p1d(dev, trans, ivar, tbar, prm, *, flags=F_ZERO, **kw):
    """qfa_p1d_f32 by hand on device tensors; prm = (p_lo, L, nseg, min_used, (z0, dz, nz)).  Returns power, noise, stack (numpy)"""
    M = prm[1] // 2
    return call_segment("qfa_p1d", dev, trans, ivar, tbar, prm, outputs=(("p", (M,), "float32"), ("n", (), "float32")),
                        stack_width=2 + 2 * M, flags=flags, **kw)


def redshift_forms(dev, g, B, nb):
    """(zf, forms): the float32 z the factored form computes, and the keywords of `call_segment` for zabs = zf, the factored pair, and
    the resident `rows` form of both (B rows of B + 4 in another order, NaN in the rows not named)"""
    zf = _p1d_ref.z_factored(g["zq1"], g["ratio"])
    N = B + 4
    rows = np.random.default_rng(3).permutation(N)[:B].astype(np.int32)
    zres, zq = np.full((N, nb), np.nan, np.float32), np.full(N, np.nan, np.float32)
    zres[rows], zq[rows] = zf, g["zq1"]
    return zf, (dict(zabs=T(zf, dev)), dict(zq1=T(g["zq1"], dev), ratio=T(g["ratio"], dev)), dict(zabs=T(zres, dev), rows=T(rows, dev)),
                dict(zq1=T(zq, dev), ratio=T(g["ratio"], dev), rows=T(rows, dev)))


def refusals(call, **valid):
    """refused(code, **bad) of a refusal test: ``call`` -- a module's wrapper of `call_segment` -- with the ``valid`` keywords, ``bad``
    over them, must return ``code`` and leave every output it was given as it was: the outputs OUT_FILL, the stack (last) STACK_FILL"""
    def refused(code, **bad):
        *got, stack = call(expect=code, **{**valid, **bad})
        for x in got:
            assert x is None or (x == OUT_FILL).all(), bad
        assert stack is None or (stack == STACK_FILL).all(), bad
    return refused


# ------------------------------------------------------------------------------------------------------------ end to end
def loader_case(dev, **dl_kw):
    """(model, mk(batch_size) -> a fresh DeviceDataloader of the same 96 spectra with 10 % dead pixels, wav)"""
    from qfa_amd import synthetic
    from qfa_amd.dataloader import DeviceDataloader
    npix, nb, nh, B = 96, 48, 4, 96
    wav = 10 ** (np.log10(synthetic.LYA) + (np.arange(npix) - nb + 0.5) * 1.2e-3)
    assert int(np.sum(wav < synthetic.LYA)) == nb
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=3)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, B, seed=33, masks=False)
    dead = np.random.default_rng(4).random((B, npix)) < 0.1
    flux, err = np.where(dead, np.float32(-999.0), b["flux"]), np.where(dead, np.float32(-999.0), b["error"])
    m = make_model(dev, {"p": p, "mu": mu}, nb, npix - nb, nh)
    mk = lambda bs: DeviceDataloader(flux, err, b["zqso"], wav, batch_size=bs, device=dev, shuffle=False, **dl_kw)
    return m, mk, wav


def tbar_range(dv):
    """the range of the mean transmission the loader calls make for bins [1.8, 3.4) and segments of 24 pixels: half a segment more"""
    half = float(np.exp(0.5 * 25 * dv / 299792.458))
    return (1.0 + 1.8) / half - 1.0, (1.0 + 3.4) * half - 1.0


def two_ranks(worker, port):
    """``worker(rank, 2, port, queue)`` in two spawned processes; returns what rank 0 put on the queue"""
    import torch.multiprocessing as mp
    from test_data_parallel import _collect
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, port + os.getpid() % 2000, q)) for r in range(2)]
    [pr.start() for pr in procs]
    got = _collect(procs, q, 300)
    [pr.join(60) for pr in procs]
    assert all(pr.exitcode == 0 for pr in procs)
    return got


def cli_predict_case(dev, tmp_path):
    """24 spectra and a model on disk for `cli.main` in predict mode.  Returns a namespace: argv(out, *opts) -- the command line that
    writes mean_transmission.npz (10 bins of [1.6, 3.6)) and the statistics of 2 segments in 3 z-bins (min_used_frac 0.6) into ``out``,
    ``opts`` appended --, and wav, npix, nb, b (the batch), names, p, mu"""
    from qfa_amd import io, synthetic
    wav = io.wavelength_grid(1030.0, 1600.0, 2e-3)
    npix, nb, n = len(wav), int(np.sum(wav < 1215.67)), 24
    p, mu = synthetic.mock_parameters(npix, nb, 4, seed=9)
    b = synthetic.make_batch_numpy(p, mu, wav, nb, n, seed=91, masks=False)
    data = tmp_path / "data"
    data.mkdir()
    names = [f"spec-{i:02d}.npz" for i in range(n)]
    for i, name in enumerate(names):
        np.savez(data / name, flux=b["flux"][i].astype(np.float64), error=b["error"][i].astype(np.float64), z=b["zqso"][i])
    (tmp_path / "pred.csv").write_text("file\n" + "\n".join(names) + "\n")
    make_model(dev, {"p": p, "mu": mu}, nb, npix - nb, 4).save_to_npz(str(tmp_path), "model.npz")
    argv = lambda out, *opts: [
        "--type", "predict", "--data_dir", str(data), "--catalog", str(tmp_path / "pred.csv"), "--output_dir", str(out),
        "--opts", "MODEL.NH", "4", "MODEL.RESUME", str(tmp_path / "model.npz"), "MODEL.REFERENCE_C0_QUIRK", "False",
        "DATA.LOGLAM_DELTA", "2e-3", "MODEL.FOREST_ZMIN", "1.6", "MODEL.FOREST_ZMAX", "3.6", "MODEL.FOREST_NBINS", "10",
        "MODEL.P1D_SEGMENTS", "2", "MODEL.P1D_NZBINS", "3", "MODEL.P1D_MIN_USED_FRAC", "0.6", *opts]
    return types.SimpleNamespace(argv=argv, wav=wav, npix=npix, nb=nb, b=b, names=names, p=p, mu=mu)
