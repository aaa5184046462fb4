"""The flux PDF without a GPU: the numpy port (tests/_flux_pdf_ref.py) against an independent count, the inputs of the GPU tests'
shapes, PDFStack's arithmetic on CPU tensors, the boundary (header, exports, size functions, argument checks) and the config keys
and command line."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _flux_pdf_ref as R
import _forest_ref as RF
from conftest import REPO

NAMES = ("qfa_flux_pdf_stack_doubles", "qfa_flux_pdf_workspace_bytes", "qfa_flux_pdf_f32")
TB_BINS = (1.5, 0.125, 17)


def _counts(rng, B, S, nseg, nt, nz):
    """integer histograms of B S nseg segments of 30 pixels, their validity and z-bins"""
    hist = rng.multinomial(30, rng.dirichlet(np.ones(nt) * 2.0), (B, S, nseg)).astype(np.int64)
    drop = rng.integers(0, 4, (B, S, nseg))                                            # pixels no bin holds
    ok = rng.random((B, S, nseg)) < 0.9
    hist = np.where(ok[..., None], hist, 0)
    n_cnt = np.where(ok, hist.sum(-1) + drop, 0)
    kz = rng.integers(-1, nz, (B, nseg))
    return hist, n_cnt, ok, kz


def test_port_against_an_independent_count():
    """x at bin centres, where float32 and float64 binning cannot differ: np.histogram on float64 per segment"""
    rng = np.random.default_rng(1)
    B, S, L, nseg, p_lo, nt = 5, 2, 23, 2, 1, 12
    t0, dt = 0.25, 0.125                                                              # (exact in float32)
    nb = p_lo + nseg * L + 2
    a = rng.integers(-3, nt + 3, (B, S, nb))
    trans = (t0 + (a + 0.5) * dt).astype(np.float32)
    ivar = rng.uniform(10.0, 100.0, (B, S, nb)).astype(np.float32)
    ivar[rng.random((B, S, nb)) < 0.2] = 0
    z = (rng.uniform(1.7, 2.0, (B, 1)) + np.linspace(0.0, 1.2, nb)[None, :]).astype(np.float32)
    tbar = np.ones((S, TB_BINS[2]), np.float32)
    bins = (1.6, 0.45, 4)
    for clamp, imin in ((False, 0.0), (True, 0.0), (False, 50.0)):
        r = R.flux_pdf(trans, ivar, z, tbar, TB_BINS, p_lo, L, nseg, 18, bins, t0, dt, nt, False, clamp, imin)
        assert r["valid"].any() and not r["valid"].all()
        for b in range(B):
            for s in range(S):
                for g in range(nseg):
                    sl = slice(p_lo + g * L, p_lo + (g + 1) * L)
                    cnt = (ivar[b, s, sl] > 0) & (ivar[b, s, sl] >= imin)
                    x = trans[b, s, sl][cnt].astype(np.float64)
                    x = np.clip(x, t0 + 0.5 * dt, t0 + (nt - 0.5) * dt) if clamp else x
                    h, _ = np.histogram(x, bins=nt, range=(t0, t0 + nt * dt))
                    ok = (ivar[b, s, sl] > 0).sum() >= 18
                    assert np.array_equal(r["hist"][b, s, g], h if ok else 0 * h) and r["n_cnt"][b, s, g] == (cnt.sum() if ok else 0)
        sel = r["valid"] & (r["kz"][:, None, :] >= 0)
        assert r["stack"][:, :, 0].sum() == sel.sum() > 0 and r["stack"][:, :, 1].sum() == r["n_cnt"][sel].sum()
        assert np.array_equal(r["stack"][:, :, 2:2 + nt].sum((0, 1)), r["hist"][sel].sum(0))
        assert np.array_equal(r["stack"][:, :, 2 + nt:].sum((0, 1)).reshape(nt, nt), np.einsum("ia,ib->ab", r["hist"][sel], r["hist"][sel]))
    # relative: one division by the draw's tbar, and a NaN x (0 / 0 cannot occur under `used`; a NaN T can) is counted but in no bin
    tb2 = np.full((S, TB_BINS[2]), 0.5, np.float32)
    r1 = R.flux_pdf(trans, ivar, z, tb2, TB_BINS, p_lo, L, nseg, 18, bins, 2 * t0, 2 * dt, nt, True, False)
    r0 = R.flux_pdf(trans, ivar, z, tb2, TB_BINS, p_lo, L, nseg, 18, bins, t0, dt, nt, False, False)
    assert np.array_equal(r1["hist"], r0["hist"])                                     # T / 0.5 on doubled bins: exact either way
    bad = trans.copy()
    j = p_lo + np.argmax(ivar[0, 0, p_lo:p_lo + L] > 0)
    bad[0, 0, j] = np.nan
    for clamp in (False, True):
        rn = R.flux_pdf(bad, ivar, z, tbar, TB_BINS, p_lo, L, nseg, 1, bins, t0, dt, nt, False, clamp)
        rc = R.flux_pdf(trans, ivar, z, tbar, TB_BINS, p_lo, L, nseg, 1, bins, t0, dt, nt, False, clamp)
        assert rn["n_cnt"][0, 0, 0] == rc["n_cnt"][0, 0, 0] and rn["hist"][0, 0, 0].sum() == rc["hist"][0, 0, 0].sum() - (1 if clamp or 0 <= a[0, 0, j] < nt else 0)


def test_inputs_of_the_gpu_shapes_exercise_what_they_are_there_for():
    """the GPU test asserts, on the port's output, valid and invalid segments, three occupied bins, pixels outside [0.2, 1.4) and
    pixels below the median ivar: confirmed here with the forest port's float64 transmission in the place of the kernel's"""
    from test_flux_pdf import BINS, CASES, T_HI, T_LO, assert_not_vacuous, case_shape, median_ivar
    from test_forest import geometry
    for rows, L, nseg, p_lo, nt in CASES:
        if L < 37:
            continue
        B, S, nb, min_used, seed = case_shape(rows, L, nseg, p_lo)
        g = geometry(nb + 20, nb, 4, B, S, seed)
        f = RF.forest(g["p"]["F"], g["mu"], g["flux"], g["error"], g["zabs"], g["mask"], g["h"], None, (1.5, 0.5, 4), 0.05)
        tbar = np.random.default_rng(seed + 1).uniform(0.3, 0.9, (S, TB_BINS[2])).astype(np.float32)
        tr, iv = np.where(f["use"], f["T"], 0).astype(np.float32), np.where(f["use"], f["iv"], 0).astype(np.float32)
        t0, dt = np.float32(T_LO), np.float32((T_HI - T_LO) / nt)
        for clamp in (False, True):
            for rel in (False, True):
                for imin in (0.0, median_ivar(iv)):
                    r = R.flux_pdf(tr, iv, g["zabs"], tbar, TB_BINS, p_lo, L, nseg, min_used, BINS, t0, dt, nt, rel, clamp, imin)
                    assert_not_vacuous(r, rows, L, nt, clamp, imin > 0, (rows, L, clamp, rel, imin))


def test_pdf_stack_arithmetic():
    import torch
    import qfa_amd
    from qfa_amd._lib import QFAHipError
    from qfa_amd.model import PDFStack
    assert qfa_amd.PDFStack is PDFStack
    rng = np.random.default_rng(3)
    B, S, nseg, nt, nz, L = 40, 3, 2, 7, 3, 30
    t0, dt = 0.2, 0.15
    hist, n_cnt, ok, kz = _counts(rng, B, S, nseg, nt, nz)
    kz[0, 0], ok[0, :, 0] = 2, True
    kz[1:, :] = np.minimum(kz[1:, :], 1)                                              # z-bin 2 holds one segment
    hist[0, :, 0], n_cnt[0, :, 0] = rng.multinomial(30, np.ones(nt) / nt, S), 31
    whole = R.stack_of(hist, n_cnt, ok, kz, nz)
    mk = lambda buf=None, **kw: PDFStack(**{**dict(buf=torch.tensor(whole, dtype=torch.float64) if buf is None else buf, z0=2.0, dz=0.5,
                                                    nz=nz, L=L, t0=t0, dt=dt, n_tbins=nt, relative=False, clamp=True, ivar_min=0.0), **kw})
    st = mk()
    assert st.S == S and st.nt == nt and st.bins == (2.0, 0.5, 3) and st.L == L and st.flux_bins == (float(np.float32(t0)), float(np.float32(dt)), nt)
    assert np.allclose(st.t_edges.numpy(), np.float32(t0) + np.float64(np.float32(dt)) * np.arange(nt + 1), rtol=0, atol=0)
    assert np.allclose(st.t_centres.numpy(), 0.5 * (st.t_edges[1:] + st.t_edges[:-1]).numpy(), rtol=1e-15)
    assert torch.equal(st.z_centres, st.z_centers) and st.n_segments[:, 2].tolist() == [1.0, 1.0, 1.0]
    sel = ok & (kz >= 0)[:, None, :]
    assert st.n_segments.sum() == sel.sum() and st.n_pixels.sum() == n_cnt[sel].sum() and st.counts.sum() == hist[sel].sum()
    # pdf integrates to 1 over the range; out_of_range is what no bin holds
    p = st.pdf()
    assert torch.allclose((p * st.dt).sum(-1), torch.ones(S, nz, dtype=torch.float64), rtol=1e-14)
    for s in range(S):
        for k in range(nz):
            pick = ok[:, s, :] & (kz == k)
            H, Nc = hist[:, s][pick].sum(0), n_cnt[:, s][pick].sum()
            assert np.allclose(p[s, k].numpy(), H / (H.sum() * np.float64(np.float32(dt))), rtol=1e-14)
            assert np.isclose(st.out_of_range()[s, k].item(), 1.0 - H.sum() / Nc, rtol=0, atol=1e-15)
    assert (st.out_of_range() > 0).any()
    # cov against the segment-by-segment sum, within the bar derived in the port; rows sum to zero within the same bar
    got, want = st.cov().numpy(), R.cov_bruteforce(hist, ok, kz, nz, dt)
    bar, scaled = R.cov_bar(whole, nt, dt)
    fin = np.isfinite(want)
    assert fin[:, :2].all() and not fin[:, 2].any() and np.array_equal(fin, np.isfinite(got))        # one segment: NaN, no division error
    assert (np.abs(got - want)[fin] <= bar[fin]).all(), (np.abs(got - want)[fin] / bar[fin]).max()
    rows_bar = ((st.n_segments.numpy()[:, :, None, None] + 32.0 + nt) * R.U64 * scaled)[:, :2].sum(-1)
    assert (np.abs(got[:, :2].sum(-1)) <= rows_bar).all() and (np.abs(got[:, :2]).sum(-1) > 1e6 * rows_bar).all()
    assert np.allclose(got[:, :2], np.swapaxes(got[:, :2], 2, 3), rtol=1e-12, atol=1e-300)
    # err and corr
    assert np.allclose(st.err().numpy()[:, :2] ** 2, np.diagonal(got[:, :2], axis1=2, axis2=3), rtol=1e-13)
    c = st.corr().numpy()[:, :2]
    assert np.allclose(np.diagonal(c, axis1=2, axis2=3), 1.0, rtol=0, atol=1e-14) and (np.abs(c) <= 1.0 + 1e-12).all()
    assert torch.isnan(st.err()[:, 2]).all() and torch.isfinite(st.pdf()[:, 2]).all()
    empty = PDFStack.zeros(2, 2.0, 0.5, nz, L, t0, dt, nt, False, True, 0.0, "cpu")
    assert empty.buf.shape == (2, 3, 2 + nt + nt * nt) and torch.isnan(empty.pdf()).all() and torch.isnan(empty.cov()).all()
    assert torch.isnan(empty.out_of_range()).all()
    # over the draws
    assert st.mean_over_draws.shape == (nz, nt) and torch.allclose(st.mean_over_draws, st.pdf().mean(0))
    assert torch.allclose(st.std_over_draws, st.pdf().std(0, unbiased=True))
    d = st.pdf() - st.pdf().mean(0, keepdim=True)
    cod = torch.einsum("sza,szb->zab", d, d) / (S - 1.0)
    assert torch.allclose(st.cov_over_draws, cod) and torch.allclose(torch.diagonal(cod, dim1=1, dim2=2), st.std_over_draws ** 2)
    assert torch.allclose(st.total_cov[:2], st.cov()[:, :2].mean(0) + cod[:2])
    with pytest.raises(QFAHipError):
        st.draws(0, 1).std_over_draws
    # two halves of the segments, added, are the whole, exactly; draws is a view; layouts are checked
    h1, h2 = R.stack_of(hist[:17], n_cnt[:17], ok[:17], kz[:17], nz), R.stack_of(hist[17:], n_cnt[17:], ok[17:], kz[17:], nz)
    a = mk(torch.tensor(h1, dtype=torch.float64))
    both = a.clone().add_(mk(torch.tensor(h2, dtype=torch.float64)))
    assert torch.equal(both.buf, st.buf) and np.array_equal(a.buf.numpy(), h1)
    assert st.draws(1, 2).S == 1 and st.draws(1, 2).buf.data_ptr() == st.buf[1:].data_ptr() and st.draws(1, 3).clamp
    for other in (st.draws(0, 1), mk(dz=0.25), mk(L=31), mk(dt=0.1), mk(t0=0.0), mk(clamp=False), mk(relative=True), mk(ivar_min=1.0)):
        with pytest.raises(QFAHipError):
            st.add_(other)
    for bad in (dict(buf=st.buf.float()), dict(buf=st.buf[:, :, :5].contiguous()), dict(n_tbins=6), dict(n_tbins=0), dict(n_tbins=65),
                dict(dt=0.0), dict(dt=float("nan")), dict(t0=float("inf")), dict(ivar_min=-1.0), dict(L=0), dict(dz=0.0)):
        with pytest.raises(QFAHipError):
            mk(**bad)
    assert PDFStack._round_bins(0.1, 0.2, 3) == (float(np.float32(0.1)), float(np.float32(0.2)), 3)


def test_boundary_declares_and_exports_the_entry_points():
    from qfa_amd import _lib
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and name + "(" in txt
    assert "qfa_pdf_t" in txt and "#define QFA_F_PDF_RELATIVE 0x800u" in txt and "#define QFA_F_PDF_CLAMP    0x1000u" in txt
    assert "#define QFA_ABI_VERSION 4" in txt
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert [f[0] for f in _lib.PDFParams._fields_] == ["t0", "dt", "nt", "ivar_min"] and C.sizeof(_lib.PDFParams) == 16
    assert _lib.F_PDF_RELATIVE == 0x800 and _lib.F_PDF_CLAMP == 0x1000


def test_size_functions():
    from qfa_amd import _lib
    h = _lib.lib()
    assert h.qfa_flux_pdf_stack_doubles(3, 7, 5) == 3 * 7 * (2 + 5 + 25) and h.qfa_flux_pdf_stack_doubles(1, 4096, 64) == 4096 * (2 + 64 + 4096)
    for a in ((0, 7, 5), (3, 0, 5), (3, 4097, 5), (3, 7, 0), (3, 7, 65), (3, 7, -1)):
        assert h.qfa_flux_pdf_stack_doubles(*a) == 0, a
    ok = (12, 3, 100, 37, 2, 7, 20)                                                # R = B S, S, Nb, L, nseg, nz, nt
    row = 3 * 7 * (2 + 20 + 210) * 4                                               # one chunk's int32 partials per (draw, z-bin)
    assert row <= h.qfa_flux_pdf_workspace_bytes(*ok) <= row + 16
    for i, bad in ((0, -3), (0, 13), (1, 0), (2, 73), (3, 0), (3, 4097), (3, 51), (4, 0), (4, 3), (5, 0), (5, 4097), (6, 0), (6, 65)):
        a = list(ok)
        a[i] = bad
        assert h.qfa_flux_pdf_workspace_bytes(*a) == 0, a
    assert h.qfa_flux_pdf_workspace_bytes(12, 3, 100, 37, 2, 7, 64) > 0
    assert h.qfa_flux_pdf_workspace_bytes(0, 1, 1, 1, 1, 1, 1) > 0                   # B = 0 is a shape the call accepts
    assert h.qfa_flux_pdf_workspace_bytes(4096 * 100, 100, 720, 240, 3, 8, 20) < (80 << 20)
    # a chunk's partials beyond the cap of a launch: one chunk all the same
    assert h.qfa_flux_pdf_workspace_bytes(4096, 1, 720, 240, 3, 4096, 64) == 16 + 4096 * (2 + 64 + 2080) * 4 * 1


def test_every_argument_check_returns_its_code_before_device_work():
    """device pointers are never dereferenced by the checks: stand-in addresses reach every code without a GPU"""
    from qfa_amd import _lib
    h = _lib.lib()
    P = C.c_void_p(4096)                                                           # a stand-in device address

    def call(B=2, S=3, Nb=40, prm=None, pdf=None, flags=0, ws_bytes=None, null=(), batch=None, outs="hs"):
        bs = _lib.Batch()
        bs.zabs = 4096
        bs.row_stride = 0
        for k, v in (batch or {}).items():
            setattr(bs, k, v)
        d = dict(zT0=2.0, dzT=0.1, nT=5, St=1, p_lo=1, seg_len=13, nseg=3, min_used=2, z0=2.0, dz=0.25, nz=4)
        d.update(prm or {})
        pp = _lib.P1DParams(**d)
        q = dict(t0=0.0, dt=0.05, nt=20, ivar_min=0.0)
        q.update(pdf or {})
        qq = _lib.PDFParams(**q)
        need = h.qfa_flux_pdf_workspace_bytes(2 * 3, 3, 40, 13, 3, 4, 20)
        a = lambda name, v: None if name in null else v
        return h.qfa_flux_pdf_f32(a("trans", P), a("ivar", P), a("b", C.byref(bs)), a("tbar", P), B, S, Nb, a("p", C.byref(pp)),
                                  a("q", C.byref(qq)), flags, P if "h" in outs else None, P if "s" in outs else None,
                                  a("workspace", P), need if ws_bytes is None else ws_bytes, None)

    for name in ("trans", "ivar", "b", "tbar", "p", "q", "workspace"):
        assert call(null=(name,)) == -1, name
    assert call(outs="") == -1 and call(batch={"zabs": None}) == -1
    assert call(batch={"zabs": None, "zq1": 4096}) == -1 and call(batch={"pix_ratio": 4096}) == -1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(S=0), dict(Nb=0), dict(prm={"seg_len": 0}), dict(prm={"seg_len": 4097}), dict(prm={"nseg": 0}),
               dict(prm={"p_lo": -1}), dict(prm={"p_lo": 2}), dict(prm={"nseg": 4}), dict(Nb=39), dict(prm={"min_used": 0}),
               dict(prm={"dz": 0.0}), dict(prm={"dz": nan}), dict(prm={"z0": inf}), dict(prm={"nz": 0}), dict(prm={"nz": 4097}),
               dict(prm={"dzT": 0.0}), dict(prm={"zT0": inf}), dict(prm={"nT": 0}), dict(prm={"St": 2}), dict(batch={"row_stride": 39}),
               dict(pdf={"nt": 0}), dict(pdf={"nt": -1}), dict(pdf={"nt": 65}), dict(pdf={"dt": 0.0}), dict(pdf={"dt": -0.1}),
               dict(pdf={"dt": nan}), dict(pdf={"dt": inf}), dict(pdf={"t0": nan}), dict(pdf={"t0": -inf}), dict(pdf={"ivar_min": -1e-3}),
               dict(pdf={"ivar_min": nan}), dict(pdf={"ivar_min": inf})):
        assert call(**kw) == -2, kw
    # the accepted values of the same arguments, on a call with nothing to do (B = 0: no device work is reached)
    assert call(B=0, prm={"St": 3}) == 0 and call(B=0, pdf={"nt": 64}, ws_bytes=1 << 30) == 0 and call(B=0, pdf={"nt": 1}) == 0
    assert call(B=0, pdf={"t0": -3.0, "ivar_min": 7.5}) == 0
    for outs in ("h", "s"):
        assert call(B=0, outs=outs) == 0, outs
    for flags in (0x800, 0x1000, 0x1800, 0x1800 | 0x20):
        assert call(B=0, flags=flags) == 0, flags
    for flags in (0x1, 0x100, 0x200, 0x400, 0x80 | 0x8, 0x2000):
        assert call(flags=flags) == -5, flags
    need = h.qfa_flux_pdf_workspace_bytes(6, 3, 40, 13, 3, 4, 20)
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3


def test_config_keys_and_python_surface():
    from qfa_amd import config as Cf
    from qfa_amd import model
    from qfa_amd.cli import build_parser
    cfg = Cf.get_config()
    M = cfg.MODEL
    assert (M.PDF_NBINS, M.PDF_TMIN, M.PDF_TMAX, M.PDF_CLAMP, M.PDF_RELATIVE, M.PDF_IVAR_MIN) == (0, 0.0, 1.0, True, False, 0.0)
    assert {"MODEL.PDF_NBINS", "MODEL.PDF_TMIN", "MODEL.PDF_TMAX", "MODEL.PDF_CLAMP", "MODEL.PDF_RELATIVE", "MODEL.PDF_IVAR_MIN"} <= set(Cf.EXTRA_KEYS)
    args = build_parser().parse_args(["--type", "predict", "--opts", "MODEL.PDF_NBINS", "24", "MODEL.PDF_TMIN", "-0.1", "MODEL.PDF_TMAX", "1.5",
                                      "MODEL.PDF_CLAMP", "False", "MODEL.PDF_RELATIVE", "True", "MODEL.PDF_IVAR_MIN", "2"])
    got = Cf.get_config(args).MODEL
    assert (got.PDF_NBINS, got.PDF_TMIN, got.PDF_TMAX, got.PDF_CLAMP, got.PDF_RELATIVE, got.PDF_IVAR_MIN) == (24, -0.1, 1.5, False, True, 2.0)
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(model.QFA.flux_pdf_segments)
    assert list(sig.parameters)[1:3] == ["trans", "ivar"]
    want = {"zabs": None, "zfac": None, "batch": None, "tbar": empty, "tbar_bins": None, "seg_len": empty, "n_segments": empty,
            "pixel_start": 0, "min_used": empty, "t_min": empty, "t_max": empty, "n_tbins": empty, "relative": False, "clamp": False,
            "ivar_min": 0.0, "bins": None, "stack": None, "return_segments": True}
    assert list(sig.parameters)[3:] == list(want)
    for k, d in want.items():
        assert sig.parameters[k].kind is KW and sig.parameters[k].default == d, k
    sig = inspect.signature(model.QFA.flux_pdf)
    assert list(sig.parameters)[1:6] == ["dataloader", "z_min", "z_max", "n_zbins", "n_tbins"] and sig.parameters["n_tbins"].default == 20
    want = {"t_min": 0.0, "t_max": 1.0, "relative": False, "clamp": True, "ivar_min": 0.0, "n_segments": 3, "seg_len": None,
            "min_used_frac": 0.75, "tbar": None, "tbar_nbins": 64, "n_samples": 0, "seed": 0, "batch_size": 4096, "cont_min": 0.0}
    assert list(sig.parameters)[6:] == list(want)
    for k, d in want.items():
        assert sig.parameters[k].kind is KW and sig.parameters[k].default == d, k


def test_cli_refuses_a_bad_pdf_request_before_any_work(tmp_path):
    from qfa_amd import cli
    out = tmp_path / "out"
    base = ["--type", "predict", "--output_dir", str(out), "--catalog", str(tmp_path / "none.csv")]
    with pytest.raises(ValueError, match="PDF_NBINS.*P1D_SEGMENTS"):
        cli.main(base + ["--opts", "MODEL.PDF_NBINS", "8", "MODEL.FOREST_NBINS", "10"])
    opts = ["MODEL.FOREST_NBINS", "10", "MODEL.P1D_SEGMENTS", "2"]
    for bad in ("65", "-1"):
        with pytest.raises(ValueError, match="PDF_NBINS"):
            cli.main(base + ["--opts"] + opts + ["MODEL.PDF_NBINS", bad])
    with pytest.raises(ValueError, match="PDF_TMAX"):
        cli.main(base + ["--opts"] + opts + ["MODEL.PDF_NBINS", "8", "MODEL.PDF_TMIN", "1.0"])
    with pytest.raises(ValueError, match="PDF_TMAX"):
        cli.main(base + ["--opts"] + opts + ["MODEL.PDF_NBINS", "8", "MODEL.PDF_TMIN", "0.5", "MODEL.PDF_TMAX", "0.25"])
    with pytest.raises(ValueError, match="PDF_IVAR_MIN"):
        cli.main(base + ["--opts"] + opts + ["MODEL.PDF_NBINS", "8", "MODEL.PDF_IVAR_MIN", "-1.0"])
    assert not out.exists()
