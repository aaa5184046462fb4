"""The observed-frame residual stack and the calibration on the GPU against their numpy port (tests/_obs_ref.py): qfa_obs_stack_f32
over the shapes, bin widths, modes and edge cases at which the kernel takes another path, qfa_calibrate_f32, and the chain
observed_stack -> find_lines + calibration -> calibrate + mask_absorbers on spectra with an injected calibration and sky line.

Bars, derived and not tuned: the counts equal the port's exactly (the inputs keep every |c - cont_min| above the fma chain's bound,
asserted on the port); every other entry is within sum |term| (rel + n 2^-53), rel the row's pixel bound from `trans_bound` /
`ivar_bound` (`_obs_ref.stack_bars`).  The achieved fractions of the bar are printed; profiles/obs_stack_accuracy.txt records them."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _obs_ref as R
from _segment_harness import F_SYNC, F_ZERO, STACK_FILL, T, dev, geometry, make_model   # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

CONT_MIN = 0.05
F_UNIT = 0x2000
U = 2.0 ** -24


def coords(npix, B, mode, width, seed):
    """(pix_u, spec_u, u0, du): `width` = "coarse" (many pixels per bin), "fine" (empty bins inside a spectrum's run) or "edge" (the
    grid's own step, every number a multiple of a power of two: coordinates fall exactly on bin edges).  With B >= 3 spectrum 0 has a
    NaN 1 + z and spectrum 1 a non-positive one."""
    rng = np.random.default_rng(seed)
    if width == "edge":
        if mode == R.LOG:
            pix_u, du = 3.0 + np.arange(npix) * 2.0 ** -13, 2.0 ** -13
            spec_u = rng.integers(4096, 5500, B).astype(np.float64) * 2.0 ** -13
        else:
            pix_u, du = 1000.0 + 0.5 * np.arange(npix), 0.25
            spec_u = rng.choice([3.0, 3.25, 3.5, 4.0], B)
    else:
        wav = 10 ** (np.log10(1040.0) + 1e-4 * np.arange(npix))
        z1 = rng.uniform(3.0, 4.5, B)
        if mode == R.LOG:
            pix_u, spec_u, du = np.log10(wav), np.log10(z1), 8e-4 if width == "coarse" else 0.3e-4
        else:
            pix_u, spec_u, du = wav, z1, 8.0 if width == "coarse" else 0.3
    # the bins start at pixel npix // 3 of the first good spectrum -- exactly on it ("edge"), or a quarter of a bin below --: that
    # spectrum lies partly inside the range, the others partly or wholly outside
    good = 2 if B >= 3 else 0
    at = pix_u[npix // 3] * spec_u[good] if mode == R.LINEAR else pix_u[npix // 3] + spec_u[good]
    u0 = at if width == "edge" else at - 0.25 * du
    if B >= 3:
        spec_u[0], spec_u[1] = np.nan, np.nan if mode == R.LOG else -0.5
    return pix_u, spec_u, float(u0), float(du)


def call_obs(dev, g, nh, pix_u, spec_u, bins, *, mask, unc=None, h=None, flags=F_ZERO, stack=None, sel=None, resident=False, expect=0, nrows=None):
    """qfa_obs_stack_f32 by hand.  bins = (u0, du, nbin, p_lo, p_hi, mode); ``sel``: the spectra of the call (default all);
    ``nrows``: B instead of the selection's own (0: the arrays stay, none of them is read); ``resident``: the resident form -- rows of B + 4 in another order, a stride of Npix + 7, NaN in what is not named.  A fresh stack
    holds STACK_FILL.  Returns the stack as numpy."""
    import torch
    from qfa_amd import _lib
    lib = _lib.lib()
    sel = np.arange(g["flux"].shape[0]) if sel is None else np.asarray(sel)
    B, npix = len(sel), g["flux"].shape[1]
    h = g["h"] if h is None else h
    S = h.shape[1]
    flux, error = g["flux"][sel], g["error"][sel]
    mk = None if mask is None else np.asarray(mask, bool)[sel]
    bs = _lib.Batch()
    keep = []
    if resident:
        N, stride = B + 4, npix + 7
        rows = np.random.default_rng(3).permutation(N)[:B].astype(np.int32)
        fr, er = np.full((N, stride), np.nan, np.float32), np.full((N, stride), np.nan, np.float32)
        mr = np.ones((N, stride), bool)
        fr[rows, :npix], er[rows, :npix] = flux, error
        if mk is not None:
            mr[rows, :npix] = mk
        tf, te, tm, tr = T(fr, dev), T(er, dev), T(mr, dev), T(rows, dev)
        bs.rows, bs.row_stride = tr.data_ptr(), stride
        if mk is None:
            tm = None
        keep += [tr]
    else:
        tf, te, tm = T(flux, dev), T(error, dev), None if mk is None else T(mk, dev)
        bs.row_stride = 0
    bs.delta, bs.error, bs.mask = tf.data_ptr(), te.data_ptr(), None if tm is None else tm.data_ptr()
    tF, tmu, th = T(g["p"]["F"], dev), T(g["mu"], dev), T(np.ascontiguousarray(h[sel]), dev)
    tu = None if unc is None else T(unc[sel], dev)
    tp = torch.tensor(np.asarray(pix_u, np.float64), device=dev)
    ts = torch.tensor(np.asarray(spec_u, np.float64)[sel], device=dev)
    u0, du, nbin, p_lo, p_hi, mode = bins
    ob = _lib.ObsBins(u0, du, nbin, p_lo, p_hi, mode)
    if stack is None:
        stack = torch.full((S, 4, nbin), STACK_FILL, dtype=torch.float64, device=dev)
    B = B if nrows is None else nrows
    need = lib.qfa_obs_stack_workspace_bytes(B, S, npix, nh, nbin)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = lib.qfa_obs_stack_f32(C.c_void_p(tF.data_ptr()), C.c_void_p(tmu.data_ptr()), C.byref(bs), C.c_void_p(th.data_ptr()),
                               None if tu is None else C.c_void_p(tu.data_ptr()), C.c_void_p(tp.data_ptr()), C.c_void_p(ts.data_ptr()),
                               B, S, npix, nh, C.byref(ob), CONT_MIN, flags, C.c_void_p(stack.data_ptr()), C.c_void_p(ws.data_ptr()),
                               need, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert st == expect, st
    return stack.cpu().numpy()


def port_of(g, nh, pix_u, spec_u, bins, *, mask, unc=None, unit_w=False, sel=None):
    sel = np.arange(g["flux"].shape[0]) if sel is None else np.asarray(sel)
    r = R.obs_stack(g["p"]["F"], g["mu"], g["flux"][sel], g["error"][sel], None if mask is None else mask[sel], g["h"][sel],
                    None if unc is None else unc[sel], pix_u, np.asarray(spec_u)[sel], bins, CONT_MIN, unit_w)
    # no pixel is excused: every continuum is further from cont_min than the float32 chain can move it
    assert np.all(np.abs(r["c"] - CONT_MIN) > (nh + 2) * U * r["cabs"])
    return r


def judge(got, r, nh, unit_w, what):
    """counts exact, sums within the bar; returns the largest achieved fraction of the bar"""
    assert np.array_equal(got[:, 3], r["stack"][:, 3]), what
    bars = R.stack_bars(r, nh, unit_w)
    err = np.abs(got[:, :3] - r["stack"][:, :3])
    assert np.all(err <= bars[:, :3]), (what, float(np.max(err / np.maximum(bars[:, :3], 1e-300))))
    on = bars[:, :3] > 0
    frac = float(np.max(err[on] / bars[:, :3][on])) if on.any() else 0.0
    print(f"obs_stack {what}: n = {int(got[:, 3].sum())}, worst fraction of the bar {frac:.3f}")
    return frac


def make_case(nh, npix, B, S, seed, maskkind):
    g = geometry(npix, npix // 2, nh, B, S, seed, masks=True)
    mask = {"none": None, "random": g["mask"], "zero": np.zeros_like(g["mask"])}[maskkind]
    if maskkind == "random":                                              # what lies under the mask reaches nothing
        rng = np.random.default_rng(seed + 1)
        junk = np.array([np.nan, np.inf, -np.inf, -999.0], np.float32)
        g["flux"] = np.where(mask, g["flux"], junk[rng.integers(0, 4, mask.shape)])
        g["error"] = np.where(mask, g["error"], junk[rng.integers(0, 4, mask.shape)])
    return g, mask


def ranges(npix):
    nb = npix // 2
    return {"full": (0, npix), "inside": (min(npix // 5, npix - 1), max(npix - npix // 7, min(npix // 5, npix - 1))),
            "across": (max(nb - 3, 0), min(nb + 40, npix)), "empty": (npix // 3, npix // 3)}


# N_h x Npix in full; B, S, nbin, the mode, the bin width, the mask, the pixel range, unit weights and unc walk their values
_NH, _NPIX = (1, 8, 9, 16, 17, 32), (1, 5, 257, 1027)
_B, _S, _NBIN = (1, 3, 65, 130), (1, 3), (1, 7, 300, 5000, 32768)
_WIDTH, _MASK, _RANGE = ("coarse", "fine", "edge"), ("random", "none", "zero", "random"), ("full", "inside", "across", "full", "empty")
_WALK = np.random.default_rng(12)


def _walk(vals, n):
    """n values: every one of ``vals`` the same number of times (as far as n allows), in a fixed shuffled order"""
    out = [vals[i % len(vals)] for i in range(n)]
    return [out[i] for i in _WALK.permutation(n)]


_N = len(_NH) * len(_NPIX)
CASES = [tuple(c[0]) + tuple(c[1:]) for c in zip(itertools.product(_NH, _NPIX), _walk(_B, _N), _walk(_S, _N), _walk(_NBIN, _N),
                                                   _walk((0, 1), _N), _walk(_WIDTH, _N), _walk(_MASK, _N), _walk(_RANGE, _N),
                                                   _walk((False, False, True), _N), _walk((True, False), _N))]


def test_the_walk_covers_every_value():
    for col, vals in ((2, _B), (3, _S), (4, _NBIN), (5, (0, 1)), (6, _WIDTH), (7, _MASK), (8, _RANGE), (9, (False, True))):
        assert {c[col] for c in CASES} == set(vals), col
    assert {(c[5], c[6]) for c in CASES} == set(itertools.product((0, 1), _WIDTH))      # both modes at the three widths
    assert any(c[3] == 1 and c[10] for c in CASES)                                      # unc at S = 1
    assert any(c[2] >= 65 and c[4] >= 300 and c[1] >= 257 and c[7] != "zero" and c[8] != "empty" for c in CASES)
    assert any(c[0] == 32 and c[3] == 3 and c[1] >= 257 for c in CASES) or any(c[0] == 32 and c[1] >= 257 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "nh{}-npix{}-B{}-S{}-nbin{}-{}-{}-{}-{}-{}".format(
    c[0], c[1], c[2], c[3], c[4], "lin" if c[5] else "log", c[6], c[7], c[8], "unit" if c[9] else "ivar"))
def test_stack_against_the_port(dev, case):
    nh, npix, B, S, nbin, mode, width, maskkind, rangekind, unit_w, with_unc = case
    g, mask = make_case(nh, npix, B, S, 100 + nh + npix, maskkind)
    pix_u, spec_u, u0, du = coords(npix, B, mode, width, 7 + nh)
    p_lo, p_hi = ranges(npix)[rangekind]
    bins = (u0, du, nbin, p_lo, p_hi, mode)
    unc = g["unc"] if (with_unc and S == 1) else None
    r = port_of(g, nh, pix_u, spec_u, bins, mask=mask, unc=unc, unit_w=unit_w)
    flags = F_ZERO | (F_UNIT if unit_w else 0)
    got = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, unc=unc, flags=flags)
    judge(got, r, nh, unit_w, "case")
    if maskkind == "zero" or rangekind == "empty":
        assert not got.any()                                              # overwritten with zeros, STACK_FILL gone
    again = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, unc=unc, flags=flags)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))       # two calls, the same bits
    if B >= 3:
        res = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, unc=unc, flags=flags, resident=True)
        assert np.array_equal(got.view(np.int64), res.view(np.int64))     # the resident form: shuffled rows, a padded stride


@pytest.mark.parametrize("nh,mode", [(8, R.LOG), (17, R.LINEAR), (32, R.LOG)])
def test_add_against_zero_accum_and_half_batches(dev, nh, mode):
    import torch
    npix, B, S, nbin = 257, 130, 3, 300
    g, mask = make_case(nh, npix, B, S, 41, "random")
    pix_u, spec_u, u0, du = coords(npix, B, mode, "coarse", 9)
    bins = (u0, du, nbin, 0, npix, mode)
    r = port_of(g, nh, pix_u, spec_u, bins, mask=mask)
    whole = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask)
    assert whole[:, 3].sum() > 1000
    judge(whole, r, nh, False, "whole")
    # ADD: onto what the stack holds
    base = torch.full((S, 4, nbin), 2.0, dtype=torch.float64, device=dev)
    added = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, flags=0, stack=base)
    assert np.array_equal(added, 2.0 + whole)
    # two half-batch ADD calls against the whole call: counts exactly, sums within the bar
    acc = torch.zeros((S, 4, nbin), dtype=torch.float64, device=dev)
    call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, flags=0, stack=acc, sel=np.arange(0, 61))
    halves = call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask, flags=0, stack=acc, sel=np.arange(61, B))
    assert np.array_equal(halves[:, 3], whole[:, 3])
    judge(halves, r, nh, False, "two halves")
    # B = 0 and an empty range add nothing, and zero under QFA_F_ZERO_ACCUM
    for kw in (dict(nrows=0), dict()):
        b2 = bins if "nrows" in kw else (u0, du, nbin, 9, 9, mode)
        keep = torch.full((S, 4, nbin), 5.0, dtype=torch.float64, device=dev)
        assert (call_obs(dev, g, nh, pix_u, spec_u, b2, mask=mask, flags=0, stack=keep, **kw) == 5.0).all()
        assert not call_obs(dev, g, nh, pix_u, spec_u, b2, mask=mask, flags=F_ZERO, stack=keep, **kw).any()


def test_a_falling_coordinate(dev):
    """a negative linear spec_u is a coordinate like any other: x falls with p, and with u0 below it the pixels are stacked"""
    nh, npix, B, S, nbin = 8, 257, 5, 1, 300
    g, mask = make_case(nh, npix, B, S, 43, "random")
    pix_u = 1000.0 + 0.5 * np.arange(npix)
    spec_u = np.array([-2.0, -2.5, 0.0, -3.0, 2.0])
    bins = (-2700.0, 2.0, nbin, 0, npix, R.LINEAR)
    r = port_of(g, nh, pix_u, spec_u, bins, mask=mask)
    assert (r["k"][0] >= 0).sum() > 100 and (r["k"][2] >= 0).sum() == 0
    judge(call_obs(dev, g, nh, pix_u, spec_u, bins, mask=mask), r, nh, False, "falling")


def test_model_entry_point_and_input_forms(dev):
    import torch
    from qfa_amd._lib import QFAHipError
    from qfa_amd.calibration import ObservedStack
    from qfa_amd.resident import ResidentBatch
    nh, npix, B, S = 8, 257, 65, 3
    nb = npix // 2
    g, mask = make_case(nh, npix, B, S, 47, "random")
    m = make_model(dev, g, nb, npix - nb, nh)
    wav = 10 ** (np.log10(1040.0) + 1e-4 * np.arange(npix))
    zq = np.random.default_rng(2).uniform(2.0, 3.5, B)
    kw = dict(zqso=zq, wav_grid=wav, lam_min=wav[npix // 3] * 3.6, nbin=300, dloglam=8e-4, cont_min=CONT_MIN)
    pix_u, spec_u = np.log10(wav), np.log10(1.0 + zq)
    r = R.obs_stack(g["p"]["F"], g["mu"], g["flux"], g["error"], mask, g["h"], None, pix_u, spec_u,
                    (float(np.log10(kw["lam_min"])), 8e-4, 300, int(np.searchsorted(wav, 1060.0)), npix, R.LOG), CONT_MIN)
    st = m.observed_residuals(T(g["flux"], dev), T(g["error"], dev), T(mask, dev), h=T(g["h"], dev), rest_range=(1060.0, np.inf), **kw)
    assert isinstance(st, ObservedStack) and st.S == S and st.bins == (float(np.log10(kw["lam_min"])), 8e-4, 300, "log")
    assert r["stack"][:, 3].sum() > 1000
    judge(st.buf.cpu().numpy(), r, nh, False, "QFA.observed_residuals")
    # stack=: the call adds; the resident form gives the same bits
    m.observed_residuals(T(g["flux"], dev), T(g["error"], dev), T(mask, dev), h=T(g["h"], dev), rest_range=(1060.0, np.inf), stack=st,
                         zqso=zq, wav_grid=wav, cont_min=CONT_MIN)
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    rb = ResidentBatch(T(g["flux"], dev), None, T(g["error"], dev), T(mask, dev), T(g["zq1"], dev), T(g["ratio"], dev), rows, npix, nb)
    st2 = m.observed_residuals(batch=rb, h=T(g["h"], dev), rest_range=(1060.0, np.inf), **kw)
    assert torch.equal(st.buf, 2 * st2.buf)
    with pytest.raises(QFAHipError):
        m.observed_residuals(T(g["flux"], dev), T(g["error"], dev), T(mask, dev), h=T(g["h"], dev), zqso=zq, wav_grid=wav)
    with pytest.raises(QFAHipError):
        m.observed_residuals(T(g["flux"], dev), T(g["error"], dev), T(mask, dev), h=T(g["h"], dev), stack=st.draws(0, 1), zqso=zq, wav_grid=wav)


@pytest.mark.parametrize("mode", [R.LOG, R.LINEAR])
def test_calibrate_against_the_port(dev, mode):
    import torch
    from qfa_amd.calibration import calibrate
    rng = np.random.default_rng(11)
    N, npix, ncal = 37, 1027, 400
    wav = 10 ** (np.log10(1040.0) + 1e-4 * np.arange(npix))
    zq = rng.uniform(2.0, 3.5, N)
    zq[3] = np.nan
    flux = rng.normal(1.0, 0.3, (N, npix)).astype(np.float32)
    err = rng.uniform(0.01, 0.1, (N, npix)).astype(np.float32)
    dead = rng.random((N, npix)) < 0.1
    flux[dead], err[dead] = -999.0, -999.0
    flux[5, 7] = -999.0                                                   # (one of the pair alone)
    cal = 1.0 + 0.2 * np.sin(np.arange(ncal) / 9.0)
    cal[50], cal[120:123], cal[200] = np.nan, 0.01, np.inf
    u0, du = (np.log10(3500.0), 4e-4) if mode == R.LOG else (3500.0, 3.0)
    table = {"u0": u0, "du": du, "mode": "log" if mode == R.LOG else "linear", "cal": cal}
    with np.errstate(invalid="ignore"):
        pix_u, spec_u = (np.log10(wav), np.log10(1.0 + zq)) if mode == R.LOG else (wav, 1.0 + zq)
    fo_r, eo_r, nu_r, j, done, qf, qe = R.calibrate(flux, err, pix_u, spec_u, cal, u0, du, mode, 0.1)
    assert done.any() and (~done & ~dead).any() and (j == -1).any() and (j == ncal - 2).any() and nu_r[3] == (~dead[3]).sum()
    fo, eo, nu = calibrate(flux, err, zq, wav, table, c_min=0.1, device=dev)
    fo, eo, nu = fo.cpu().numpy(), eo.cpu().numpy(), nu.cpu().numpy()
    assert np.array_equal(nu, nu_r)
    # the pixels left alone keep their input bits; the calibrated set is the port's (a quotient that equals its input is allowed)
    assert np.array_equal(fo[~done].view(np.int32), flux[~done].view(np.int32)) and np.array_equal(eo[~done].view(np.int32), err[~done].view(np.int32))
    changed = (fo.view(np.int32) != flux.view(np.int32)) | (eo.view(np.int32) != err.view(np.int32))
    assert not changed[~done].any() and changed[done].mean() > 0.99
    # one float32 rounding of the float64 quotient (the port's c carries the extended format's rounding of the fma: one ulp of float64)
    for got, q in ((fo, qf), (eo, qe)):
        assert np.all(np.abs(got[done].astype(np.float64) - q[done]) <= 0.5 * np.spacing(np.abs(q[done]).astype(np.float32)) * (1 + 1e-6))
    # in place equals out of place, bit for bit
    tf, te = T(flux, dev), T(err, dev)
    f2, e2, n2 = calibrate(tf, te, zq, wav, table, c_min=0.1, out=(tf, te), device=dev)
    assert f2 is tf and np.array_equal(tf.cpu().numpy().view(np.int32), fo.view(np.int32))
    assert np.array_equal(te.cpu().numpy().view(np.int32), eo.view(np.int32)) and np.array_equal(n2.cpu().numpy(), nu)
    assert torch.cuda.is_available()


def test_end_to_end_calibration_and_sky_line(dev, tmp_path):
    """spectra drawn from the model, a known smooth calibration multiplied in, the noise inflated in one observed interval: the chain
    finds the interval and nothing else, and recovers the calibration within 5 of the stack's own error per bin.  The port is held
    to both conditions on the same data before the GPU is judged."""
    import torch
    from qfa_amd import io
    from qfa_amd.absorbers import mask_absorbers
    from qfa_amd.calibration import ObservedStack, calibrate
    from qfa_amd.dataloader import DeviceDataloader
    from qfa_amd.synthetic import LYA
    nh, npix, B, nb = 4, 257, 64, 100
    step = 1.2e-3
    rng = np.random.default_rng(2024)
    g = geometry(npix, nb, nh, B, 1, 5, masks=False)
    g["p"]["Psi"] = np.full(npix, 1e-4, np.float32)
    m = make_model(dev, g, nb, npix - nb, nh)
    wav = 10 ** (np.log10(LYA) + (np.arange(npix) - nb + 0.5) * step)
    zq = rng.uniform(2.2, 3.4, B)
    error = rng.uniform(0.02, 0.05, (B, npix)).astype(np.float32)
    zabs = ((1.0 + zq)[:, None] * wav[None, :nb] / LYA - 1.0).astype(np.float32)
    flux = m.sample_spectra(T(error, dev), T(zabs, dev), None, n_samples=1, seed=7)[:, 0].cpu().numpy()
    lam_obs = wav[None, :] * (1.0 + zq)[:, None]
    cal_true = lambda lam: 1.0 + 0.08 * np.sin(2.0 * np.pi * (lam - 4000.0) / 900.0)
    line = (6056.0, 6069.0)                                               # inside bin 150 of the stack below
    flux = flux * cal_true(lam_obs)
    error = (error * cal_true(lam_obs)).astype(np.float32)
    hit = (lam_obs >= line[0]) & (lam_obs < line[1])
    flux = (flux + np.where(hit, 8.0 * error * rng.normal(0, 1, hit.shape), 0.0)).astype(np.float32)
    loader = DeviceDataloader(flux, error, zq, wav, batch_size=B, device=dev, shuffle=False)
    lam_min, nbin = 4000.0, 270                                           # bins of the grid's own step: bin 150 = [6054.2, 6071.0) A
    red = (1230.0, np.inf)
    kw = dict(min_count=20, chi2_ratio=5.0, max_dev=0.15, grow=0, half_width=2)

    def conditions(st, who):
        found = st.find_lines(**kw)
        assert len(found) == 1 and found[0, 0] <= line[0] and found[0, 1] >= line[1], (who, found)
        n, err, mean = st.n[0].cpu().numpy(), st.err()[0].cpu().numpy(), st.calibration(0)
        ok = n >= kw["min_count"]
        assert ok.sum() > 60
        dev_sig = np.abs(mean[ok] - cal_true(st.wave_centers[ok])) / err[ok]
        print(f"{who}: {int(ok.sum())} bins, calibration within {dev_sig.max():.2f} sigma, line {found[0]}")
        assert np.all(dev_sig <= 5.0), (who, float(dev_sig.max()))
        return found

    st = m.observed_stack(loader, lam_min, nbin, dloglam=step, rest_range=red)
    # the port on the same data and the same posterior mean, first
    rb, _ = loader.rows_batch(0, B)
    _, hmean, _, _, unc = m.predict(batch=rb)
    u0 = float(np.log10(lam_min))
    p_lo = int(np.searchsorted(wav, red[0]))
    gp = dict(g, flux=flux, error=error, h=hmean.cpu().numpy()[:, None, :])
    r = R.obs_stack(g["p"]["F"], g["mu"], flux, error, None, gp["h"], unc.cpu().numpy(), np.log10(wav), np.log10(1.0 + zq),
                    (u0, step, nbin, p_lo, npix, R.LOG), 0.0)
    conditions(ObservedStack(torch.tensor(r["stack"]), u0, step, nbin, "log"), "port")
    judge(st.buf.cpu().numpy(), r, nh, False, "end to end")
    found = conditions(st, "gpu")
    # the products on disk, and the chain's second half: calibrate, then mask the found interval
    io.write_intervals(str(tmp_path / "sky_lines.txt"), found)
    io.write_calibration(str(tmp_path / "calibration.npz"), st, half_width=2)
    table = io.read_calibration(str(tmp_path / "calibration.npz"))
    fc, ec, nu = calibrate(flux, error, zq, wav, table, c_min=0.5, device=dev)
    fr, er, nur, _, done, _, _ = R.calibrate(flux, error, np.log10(wav), np.log10(1.0 + zq), table["cal"], u0, step, R.LOG, 0.5)
    assert np.array_equal(nu.cpu().numpy(), nur) and done.mean() > 0.3
    assert np.array_equal(fc.cpu().numpy()[~done].view(np.int32), flux[~done].view(np.int32))
    assert np.allclose(fc.cpu().numpy()[done], fr[done], rtol=2e-7, atol=0)
    fm, em, rec = mask_absorbers(fc, ec, zq, wav, sky=io.read_intervals(str(tmp_path / "sky_lines.txt")), device=dev)
    inside = (lam_obs >= found[0, 0]) & (lam_obs < found[0, 1])
    assert hit[inside].sum() == hit.sum() and (fm.cpu().numpy()[inside] == -999.0).all() and (fm.cpu().numpy()[~inside] != -999.0).all()
    assert int(rec["n_interval_masked"].sum()) == int(inside.sum())
