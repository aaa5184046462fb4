"""The mean-optical-depth models and Lyman series that the kernels are judged at (tests/test_tau_models.py on the GPU,
tests/test_tau_models_cpu.py on the judges themselves) -- plain numpy.

Ten C-ABI entry points take ``qfa_tau_t {amp, scale, expo, offset}``; the library ships four models x series 1..30 and the rest
of the suite runs ``becker``, series 1.  The kernels' tau arithmetic (qfa_amd/csrc/qfa_common.h: ``load_consts``,
``blue_terms``, ``zfac_spec`` / ``k_zfac_pix`` / ``blue_terms_zf``) was tuned on that one model, where the exponent handed to
exp2 is about 1 (about 8 for the other three), and three of the four have scale = 1 and offset = 0, so that the split of
log2(scale), ``offp`` and the per-blue-pixel offset image take their trivial values.  The table:

* ``MODELS``: fg, kamble, mock at series 1; becker at series 2 (the only combination where offset x series coefficient is not
  trivial); kamble at series 5; becker at series 30 (tau of order 1e-4: A within a few float32 ulps of 1).
* redshifts: "std" = z_qso ~ U(2, 3.5) as every other case of the suite draws them (tau <= 0.65); "hiz" = z_qso ~ U(4.5, 5.5)
  for fg, kamble, mock at series 1: tau reaches 2 to 3 and A 0.1 to 0.05 -- the relative error of A is tau x that of tau.
* shapes: one per N_h arm from the tables of tests/_elementwise_ref.py (``STEP_SHAPES`` of GRADIENT_CASES, ``PREDICT_SHAPES`` of
  PREDICT_CASES): they cross a 16-pixel tile edge, hold the blue / red boundary inside a tile and end in a ragged tile.

The spectra are DRAWN from the model under test (``draw``: synthetic.make_batch_numpy line by line with the model and the
redshift range as arguments -- at becker, series 1, "std" it returns that function's arrays bit for bit, which
tests/test_tau_models_cpu.py asserts), then masked as ``_elementwise_ref.gradient_case`` / ``predict_case`` mask theirs.

``emulate_A`` restates ``blue_terms`` and the factored form in float32 with correctly rounded log2 / exp2: what the float32
constants and the float32 chain cost WITHOUT the hardware transcendentals (tests/test_tau_models_cpu.py prints the table).
"""
import math
import os

import numpy as np

import _elementwise_ref as E
from oracle import qfa_oracle as O
from qfa_amd import synthetic

MODELS = [("fg", 1), ("kamble", 1), ("mock", 1), ("becker", 2), ("kamble", 5), ("becker", 30)]
HIGH_Z = [("fg", 1), ("kamble", 1), ("mock", 1)]
Z_RANGE = {"std": (2.0, 3.5), "hiz": (4.5, 5.5)}
VARIANTS = [(w, s, "std") for w, s in MODELS] + [(w, s, "hiz") for w, s in HIGH_Z]

STEP_SHAPES = [(333, None, 5, 17), (200, None, 16, 70), (260, None, 24, 35)]       # N_h <= 8 | 9..16 | 17..32
PREDICT_SHAPES = [(97, 8, 17), (333, 13, 16), (97, 17, 129)]
assert set(STEP_SHAPES) <= set(E.GRADIENT_CASES) and set(PREDICT_SHAPES[1:]) <= set(E.PREDICT_CASES)   # ((97, 8, 129) is its neighbour)

STEP_CASES = [v + (c,) for v in VARIANTS for c in STEP_SHAPES]
PREDICT_CASES = [v + (c,) for v in VARIANTS for c in PREDICT_SHAPES]

SKEYS = ("tau0", "c0", "beta")
TOL_SCAL = 1.5e-7               # of the sum of |terms| (tests/test_exact_gradients.py)
# The variants whose scalar gradients are judged against the float64 oracle on the FLOAT32 constants of the struct (read back
# through _lib.tau_model, promoted to float64) instead of the double constants.  kamble, series 1, z_qso ~ U(4.5, 5.5): measured on
# MI355X against the double constants 1.50e-7 .. 1.56e-7 in the factored and the resident form (exact mode; 1.29e-7 .. 1.44e-7 in
# reference mode, 1.11e-7 .. 1.28e-7 in the zabs form), against the struct's constants 0.96e-7 .. 1.07e-7 (zabs form 0.65e-7 ..
# 0.86e-7): the excess is the rounding of expo = 3.182 and amp = 5.54e-3 to float32 (a coherent +2.1e-7 in A at tau = 2 to 3,
# 5e-8 of the sum of |terms|: tests/test_tau_models_cpu.py prints it), which qfa_tau_t {four floats} fixes, not the kernels'
# arithmetic.  Every field is within half a float32 ulp of the double product (test_struct_fields_are_float32_of_the_double_
# products).  profiles/tau_model_accuracy.txt holds both columns for every run.
SCALARS_ON_STRUCT_CONSTANTS = {("kamble", 1, "hiz")}


def case_id(c):
    which, series, zr, shape = c
    return f"{which}{series}-{zr}-" + "x".join("b" if v is None else str(v) for v in shape)


def tau_constants(which, series):
    """(amp, scale, expo, offset) in float64 with the series coefficient in amp and offset: what ``qfa_tau_model`` rounds to
    float32 field by field"""
    amp, scale, expo, off = O.TAU_MODELS[which]
    c = float(O.LYMAN_COEFF[series - 1])
    return amp * c, scale, expo, off * c


def struct_constants(t):
    """the float32 fields of a ``_lib.TauModel`` promoted to float64: the 4-tuple the oracle takes for ``tau_which``"""
    return float(t.amp), float(t.scale), float(t.expo), float(t.offset)


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def draw(params, mu, wav, nb, batch, seed, which="becker", series=1, zrange=(2.0, 3.5), masks=True):
    """synthetic.make_batch_numpy with the tau model and the range of z_qso as arguments: the same draws in the same order"""
    rng = np.random.default_rng(seed)
    n_pix = len(wav)
    F = np.asarray(params["F"], dtype=np.float64)
    Psi = np.asarray(params["Psi"], dtype=np.float64)
    om = np.asarray(params["omega"], dtype=np.float64)
    tau0, beta, c0 = float(params["tau0"]), float(params["beta"]), float(params["c0"])
    mu = np.asarray(mu, dtype=np.float64)
    zq = rng.uniform(zrange[0], zrange[1], size=batch)
    zabs = (1.0 + zq)[:, None] * wav[None, :nb] / synthetic.LYA - 1.0
    A = np.ones((batch, n_pix))
    A[:, :nb] = np.exp(-O.tau_eff(zabs, which, series))
    h = rng.standard_normal((batch, F.shape[1]))
    snr = np.exp(rng.uniform(math.log(2.0), math.log(100.0), size=batch))
    sigma = mu[None, :] / snr[:, None] * (0.8 + 0.4 * rng.random((batch, n_pix)))
    zdep = (1.0 - c0 - np.exp(-tau0 * (1.0 + zabs) ** beta)) ** 2
    flux = A * (mu[None, :] + h @ F.T + np.sqrt(Psi)[None, :] * rng.standard_normal((batch, n_pix)))
    flux[:, :nb] += np.sqrt(om[None, :] * zdep) * rng.standard_normal((batch, nb))
    flux += sigma * rng.standard_normal((batch, n_pix))
    mask = np.ones((batch, n_pix), dtype=bool)
    if masks:
        for s in range(batch):
            for _ in range(rng.poisson(2.0)):
                ln = int(rng.integers(10, 101))
                st = int(rng.integers(0, n_pix))
                mask[s, st:st + ln] = False
        mask &= rng.random((batch, n_pix)) >= 0.01
    flux = np.where(mask, flux, -999.0)
    sigma = np.where(mask, sigma, -999.0)
    delta = flux - mu[None, :] * A
    return {"delta": delta.astype(np.float32), "error": sigma.astype(np.float32), "zabs": zabs.astype(np.float32), "mask": mask,
            "flux": flux.astype(np.float32), "zqso": zq.astype(np.float32)}


def _draw(npix, nb, nh, N, seed, wav, which, series, zr):
    """``_elementwise_ref._draw`` from the model under test"""
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=seed)
    full = draw(p, mu, wav, nb, N, 1000 + seed, which, series, Z_RANGE[zr], masks=False)
    mask = draw(p, mu, wav, nb, N, 1000 + seed, which, series, Z_RANGE[zr], masks=True)["mask"].copy()
    mu_a = (full["flux"].astype(np.float64) - full["delta"].astype(np.float64)).astype(np.float32)
    return p, mu, full, mask, mu_a


def gradient_case(which, series, zr, shape):
    """(p, mu, wav, nb, batch of N >= B resident rows, rows): ``_elementwise_ref.gradient_case`` of ``shape`` -- its seeds, its
    masks with runs, its thin coverage -- with spectra drawn from the model (which, series) at the redshifts ``zr``"""
    npix, nb, nh, B = shape
    seed = 5 * npix + 17 * nh + B
    if nb is None:
        wav, nb, nr = synthetic.wavelength_grid(npix)
    else:
        wav = np.linspace(1100.0, 1300.0, npix)
    N = B + 5
    p, mu, full, mask, mu_a = _draw(npix, nb, nh, N, seed, wav, which, series, zr)
    rows = E._rows_of(N, B, seed)
    (a, e), none, last = E.thin_pixels(npix)
    mask[:, a:e] = False
    mask[rows[B - 1], a:e] = True
    mask[:, none] = False
    mask[:, last] = False
    mask[rows[0], last] = True
    return p, mu, wav, nb, E._remask(full, mask, mu_a), rows


def predict_case(which, series, zr, shape):
    """``_elementwise_ref.predict_case`` of ``shape`` likewise: a pixel masked everywhere, a fully masked spectrum (B // 2), a
    red-only one (row 1) and one with errors of 1e-4 of its flux (row 3 B // 4)"""
    npix, nh, B = shape
    seed = 7 * npix + 131 * nh + B
    wav, nb, nr = synthetic.wavelength_grid(npix)
    N = B + 7
    p, mu, full, mask, mu_a = _draw(npix, nb, nh, N, seed, wav, which, series, zr)
    rows = E._rows_of(N, B, seed)
    mask[:, npix // 3] = False
    if B >= 5:
        mask[rows[B // 2], :] = False
        mask[rows[1], :nb] = False
        hi = rows[(3 * B) // 4]
        full["error"][hi] = (np.abs(full["flux"][hi]) * 1e-4 + 1e-12).astype(np.float32)
    return p, mu, wav, nb, E._remask(full, mask, mu_a), rows


LOADER_SHAPE = (200, 4, 24)            # (N_pix, N_h, spectra of the data set = one batch)


def loader_case(which):
    """(p, mu as drawn, wav, nb, data set) of the loader test: flux / error / z_qso as a loader is given them (-999 under the
    masks), drawn from ``which`` at series 1"""
    npix, nh, N = LOADER_SHAPE
    wav, nb, nr = synthetic.wavelength_grid(npix)
    p, mu = synthetic.mock_parameters(npix, nb, nh, seed=77)
    return p, mu, wav, nb, draw(p, mu, wav, nb, N, 770, which, 1)


def loader_batch(which):
    """the batch that the loader's resident form must hold, by the float64 port of the reference's host preprocessing
    (oracle.qfa_oracle: mu_estimate, delta_from_flux -- tau_total over the Lyman series), rounded to float32"""
    p, mu0, wav, nb, b = loader_case(which)
    raw, mu = O.mu_estimate(wav, b["flux"].astype(np.float64), b["mask"], b["zqso"], nb, which=which)
    delta = O.delta_from_flux(wav, b["flux"].astype(np.float64), b["zqso"], mu, nb, which=which)
    return p, wav, nb, {"delta": delta.astype(np.float32), "error": b["error"], "mask": b["mask"], "zqso": b["zqso"],
                        "zabs": O.zabs_from_zqso(wav, b["zqso"], nb).astype(np.float32)}


# ----------------------------------------------------------------------------------------------------------------------
# the references of the training step
# ----------------------------------------------------------------------------------------------------------------------
def step_sums(p, b, rows, tau_which, tau_series=1, dtype=np.float64, A_blue=None):
    """One oracle pass over the spectra ``rows``: (what ``E.gradient_units`` gives for F, Psi, omega and the NLL;
    {tau0 | c0 | beta: (sum of the terms, sum of |terms|, number of non-zero terms)}).  ``A_blue``: (len(rows), N_b) or None."""
    out, sc = None, {k: [0.0, 0.0, 0] for k in SKEYS}
    nll = np.empty(len(rows))
    for j, r in enumerate(rows):
        nll[j], g, ab = O.nll_and_grads_single(p, b["delta"][r], b["error"][r], b["zabs"][r], b["mask"][r], tau_which, tau_series,
                                               dtype=dtype, A_blue=None if A_blue is None else A_blue[j], return_abs=True)
        if out is None:
            out = {k: {"sum": np.zeros_like(g[k]), "count": np.zeros(g[k].shape), "abssum": np.zeros_like(g[k])} for k in E.GKEYS}
        for k in E.GKEYS:
            out[k]["sum"] = out[k]["sum"] + g[k]
            out[k]["count"] = out[k]["count"] + (g[k] != 0.0)
            out[k]["abssum"] = out[k]["abssum"] + np.abs(g[k])
        for k in SKEYS:
            sc[k][0] += float(g[k])
            sc[k][1] += float(ab[k])
            sc[k][2] += int(g[k] != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in E.GKEYS:
            out[k]["grad"] = out[k]["sum"] / out[k]["count"]
    out["nll"] = nll
    return out, {k: tuple(v) for k, v in sc.items()}


def scalar_units(ours, sc):
    """|ours - sum / n| n / sum|terms| of a NORMALISED scalar gradient of the reference mode (sum / number of non-zero terms)"""
    total, absum, n = sc
    if n == 0:                                           # no term: 0 / 0 = NaN on both sides
        return 0.0 if np.isnan(ours) else np.inf
    if not np.isfinite(ours):
        return np.inf
    return abs(float(ours) - total / n) * n / absum if absum > 0 else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# blue_terms and the factored form in float32 with correctly rounded transcendentals
# ----------------------------------------------------------------------------------------------------------------------
_f32 = np.float32
LOG2E32 = _f32(1.4426950408889634)


def _r(x):
    return np.asarray(x, dtype=np.float64).astype(_f32)


def struct_f32(which, series):
    """the four fields as ``qfa_tau_model`` forms them: float32 of the double product"""
    return tuple(_f32(c) for c in tau_constants(which, series))


def emulate_consts(t32):
    """``load_consts``: the float32 part of log2(scale) in the exponent, its remainder in the amplitude, both from float64"""
    amp, scale, expo, off = t32
    l2s = math.log2(float(scale))
    lscale = _f32(l2s)
    t_amp = _f32(float(amp) * 2.0 ** (float(expo) * (l2s - float(lscale))))
    return {"t_amp": t_amp, "t_lscale": lscale, "t_expo": _f32(expo), "t_off": _f32(off), "offp": _f32(-LOG2E32 * _f32(off))}


def emulate_A(zabs32, t32):
    """A of ``blue_terms`` (the zabs form), every operation rounded to float32, log2 and exp2 correctly rounded"""
    k = emulate_consts(t32)
    one_z = (_f32(1.0) + np.asarray(zabs32, dtype=_f32)).astype(_f32)
    l2 = _r(np.log2(one_z.astype(np.float64)))
    arg = (k["t_expo"] * (l2 + k["t_lscale"]).astype(_f32)).astype(_f32)
    ex = _r(np.exp2(arg.astype(np.float64)))
    tau = ((k["t_amp"] * ex).astype(_f32) + k["t_off"]).astype(_f32)
    return _r(np.exp2(((-tau).astype(_f32) * LOG2E32).astype(_f32).astype(np.float64)))


def emulate_A_factored(zq1_32, ratio32, t32):
    """A of ``zfac_spec`` / ``k_zfac_pix`` / ``blue_terms_zf``: the two factors from float64, rounded once; one fused
    multiply-add and one exp2 per element"""
    amp, scale, expo, off = (float(c) for c in t32)
    k = emulate_consts(t32)
    l2s = np.log2(np.asarray(zq1_32, dtype=np.float64))
    ts = _r(-1.4426950408889634 * amp * np.exp2(expo * (l2s + math.log2(scale))))
    ti = _r(np.exp2(expo * np.log2(np.asarray(ratio32, dtype=np.float64))))
    arg = _r(ts.astype(np.float64)[:, None] * ti.astype(np.float64)[None, :] + float(k["offp"]))
    return _r(np.exp2(arg.astype(np.float64)))


def record(line):
    """QFA_TAU_MODEL_LOG=<file>: the GPU tests append their achieved maxima there (profiles/tau_model_accuracy.txt)"""
    print(line)
    path = os.environ.get("QFA_TAU_MODEL_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
