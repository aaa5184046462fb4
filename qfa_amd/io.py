"""On-disk spectrum reader and catalogue selection.

Host-side ingestion only: per-spectrum ``.npz`` files (``flux``, ``error``, ``z``; missing pixels are
``-999.``) and the catalogue filter of the reference (reference QFA/dataloader.py:18-55,72-90).  What the
reference does with the arrays afterwards (``zabs``, ``delta``, masks, ``mu``) runs on the device in
``qfa_amd.dataloader.DeviceDataloader``; this module only gets the bytes off the disk.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MISSING = -999.0


def wavelength_grid(lam_min, lam_max, loglam_delta):
    """the common rest-frame grid (reference QFA/dataloader.py:59)"""
    return 10 ** np.arange(np.log10(lam_min), np.log10(lam_max), loglam_delta)


def read_npz_spectrum(path):
    """flux, error, z, path of one spectrum file (reference QFA/dataloader.py:18-30; the mask
    ``(flux != -999) & (error != -999)`` is derived on the device from the same sentinels)."""
    with np.load(path) as f:
        return np.asarray(f["flux"]), np.asarray(f["error"]), float(f["z"]), path


def read_spectra(paths, nprocs=1):
    """(flux (N, Npix) f32, error (N, Npix) f32, zqso (N,) f64, paths) in the order of ``paths``
    (reference QFA/dataloader.py:33-45; threads instead of a process pool: the work is file I/O and
    zip inflation, both release the GIL)."""
    paths = list(paths)
    if not paths:
        raise ValueError("no spectrum files given")
    if nprocs and nprocs > 1:
        with ThreadPoolExecutor(max_workers=int(nprocs)) as ex:
            data = list(ex.map(read_npz_spectrum, paths))
    else:
        data = [read_npz_spectrum(p) for p in paths]
    npix = {d[0].shape[-1] for d in data} | {d[1].shape[-1] for d in data}
    if len(npix) != 1:
        raise ValueError(f"all spectra must share one wavelength grid, got lengths {sorted(npix)}")
    flux = np.stack([d[0] for d in data]).astype(np.float32, copy=False)
    error = np.stack([d[1] for d in data]).astype(np.float32, copy=False)
    zqso = np.array([d[2] for d in data], dtype=np.float64)
    return flux, error, zqso, np.array([d[3] for d in data])


def read_observed_spectrum(path):
    """wave, flux, ivar, bad, z of one observed-frame file: keys ``wave`` (Angstrom) or ``loglam`` (log10 Angstrom, the SDSS
    column), ``flux``, ``ivar``, optional ``and_mask`` (non-zero = a flagged pixel), ``z``"""
    with np.load(path) as f:
        wave = np.asarray(f["wave"], dtype=np.float64) if "wave" in f.files else 10.0 ** np.asarray(f["loglam"], dtype=np.float64)
        flux, ivar = np.asarray(f["flux"], dtype=np.float32), np.asarray(f["ivar"], dtype=np.float32)
        bad = (np.asarray(f["and_mask"]) != 0) if "and_mask" in f.files else np.zeros(len(wave), dtype=bool)
        z = float(f["z"])
    if not (wave.ndim == 1 and wave.shape == flux.shape == ivar.shape == bad.shape):
        raise ValueError(f"{path}: wave / flux / ivar / and_mask must be 1-d arrays of one length")
    return wave, flux, ivar, bad.view(np.uint8), z


def read_observed_npz(paths, nprocs=1):
    """Observed-frame spectra as ``qfa_amd.preprocess.preprocess`` takes them: the ragged, concatenated form
    (wave f64, flux f32, ivar f32, bad u8, offsets i64 (N + 1), zqso f64 (N)) of the per-spectrum files, in the order of ``paths``.
    (No FITS reader: the survey's tables are converted to .npz by whoever has astropy.)"""
    paths = list(paths)
    if not paths:
        raise ValueError("no spectrum files given")
    if nprocs and nprocs > 1:
        with ThreadPoolExecutor(max_workers=int(nprocs)) as ex:
            data = list(ex.map(read_observed_spectrum, paths))
    else:
        data = [read_observed_spectrum(p) for p in paths]
    offsets = np.concatenate([[0], np.cumsum([len(d[0]) for d in data])]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([d[i] for d in data]).astype(dt, copy=False)
    return cat(0, np.float64), cat(1, np.float32), cat(2, np.float32), cat(3, np.uint8), offsets, \
        np.array([d[4] for d in data], dtype=np.float64)


def read_absorber_csv(path):
    """An absorber catalogue (columns ``file``, ``z_abs``, ``log_nhi``; any number of rows per file) as the table
    ``qfa_amd.absorbers.AbsorberCatalog.from_table`` takes"""
    import pandas as pd
    t = pd.read_csv(path)
    missing = [c for c in ("file", "z_abs", "log_nhi") if c not in t.columns]
    if missing:
        raise ValueError(f"{path}: missing column(s) {missing}")
    return {"file": t["file"].astype(str).values, "z_abs": t["z_abs"].values.astype(np.float64),
            "log_nhi": t["log_nhi"].values.astype(np.float64)}


BAL_COLUMNS = ("file", "line", "v_min", "v_max", "bi", "ai")


def write_bal_csv(path, table):
    """A BAL catalogue, one row per trough: columns ``file``, ``line`` (Angstrom), ``v_min``, ``v_max`` (km/s of outflow velocity),
    ``bi``, ``ai`` (km/s, of the spectrum and line the trough belongs to) -- ``BALScan.to_table``; floats with 17 significant digits"""
    cols = [np.asarray(table[c]).reshape(-1) for c in BAL_COLUMNS]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("write_bal_csv: the columns must have one length")
    with open(path, "w") as f:
        f.write(",".join(BAL_COLUMNS) + "\n")
        for row in zip(*cols):
            f.write(str(row[0]) + "," + ",".join(repr(float(x)) for x in row[1:]) + "\n")
    return path


def read_bal_csv(path):
    """The table ``write_bal_csv`` wrote, bit for bit: a dict of ``file`` (str) and float64 ``line``, ``v_min``, ``v_max``, ``bi``,
    ``ai``; ``bi`` / ``ai`` may be missing from a catalogue brought from elsewhere (NaN then)"""
    import pandas as pd
    t = pd.read_csv(path, float_precision="round_trip")
    missing = [c for c in ("file", "v_min", "v_max") if c not in t.columns]
    if missing:
        raise ValueError(f"{path}: missing column(s) {missing}")
    out = {"file": t["file"].astype(str).values}
    for c in BAL_COLUMNS[1:]:
        out[c] = t[c].values.astype(np.float64) if c in t.columns else np.full(len(t), np.nan)
    return out


REDSHIFT_COLUMNS = ("file", "z_cat", "z", "sigma_z", "dv_kms", "sigma_kms", "best_s", "offset", "best_llr", "at_edge")


def write_redshift_csv(path, table):
    """A redshift catalogue, one row per spectrum: ``file``, the catalogue redshift ``z_cat``, the refined ``z`` and ``sigma_z``,
    the velocity offset ``dv_kms`` and ``sigma_kms``, the best pixel shift ``best_s`` (int), the parabola's ``offset`` in pixels, the
    log-likelihood gain ``best_llr`` and ``at_edge`` (0 / 1) -- ``RedshiftScan.to_table``; floats with 17 significant digits"""
    cols = [np.asarray(table[c]).reshape(-1) for c in REDSHIFT_COLUMNS]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("write_redshift_csv: the columns must have one length")
    ints = {REDSHIFT_COLUMNS.index("best_s"), REDSHIFT_COLUMNS.index("at_edge")}
    with open(path, "w") as f:
        f.write(",".join(REDSHIFT_COLUMNS) + "\n")
        for row in zip(*cols):
            f.write(str(row[0]) + "," + ",".join(str(int(x)) if k in ints else repr(float(x)) for k, x in enumerate(row) if k > 0) + "\n")
    return path


def read_redshift_csv(path):
    """The table ``write_redshift_csv`` wrote, bit for bit: a dict of ``file`` (str), int64 ``best_s`` and ``at_edge`` and float64
    for the rest (NaN stays NaN)"""
    import pandas as pd
    t = pd.read_csv(path, float_precision="round_trip")
    missing = [c for c in REDSHIFT_COLUMNS if c not in t.columns]
    if missing:
        raise ValueError(f"{path}: missing column(s) {missing}")
    out = {"file": t["file"].astype(str).values}
    for c in REDSHIFT_COLUMNS[1:]:
        out[c] = t[c].values.astype(np.int64 if c in ("best_s", "at_edge") else np.float64)
    return out


def bal_rest_intervals(names, table, pad_kms=0.0, lines=None):
    """The per-spectrum ``rest=`` list of ``mask_absorbers`` from a BAL table: for the spectra ``names`` (a trailing ``.npz`` is
    ignored on both sides) the intervals ``bal_intervals(v_min - pad_kms, v_max + pad_kms, lines)`` of every row of the file"""
    from .absorbers import BAL_LINES, bal_intervals
    key = lambda n: str(n)[:-4] if str(n).endswith(".npz") else str(n)
    by_file = {}
    for f, a, b in zip(table["file"], table["v_min"], table["v_max"]):
        by_file.setdefault(key(f), []).append((float(a) - float(pad_kms), float(b) + float(pad_kms)))
    out = []
    for n in names:
        v = np.asarray(by_file.get(key(n), []), dtype=np.float64).reshape(-1, 2)
        out.append(bal_intervals(v[:, 0], v[:, 1], BAL_LINES if lines is None else lines) if len(v) else np.zeros((0, 2)))
    return out


def read_intervals(path):
    """Intervals ``[lo, hi)`` in Angstrom, one per line, two columns separated by blanks or a comma (``#`` starts a comment):
    float64 (n, 2)"""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].replace(",", " ").split()
            if not line:
                continue
            if len(line) != 2:
                raise ValueError(f"{path}: a line with {len(line)} columns, expected 2")
            rows.append((float(line[0]), float(line[1])))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 2)


def write_intervals(path, intervals, header=None):
    """Intervals ``[lo, hi)`` in Angstrom as ``read_intervals`` reads them back bit for bit: one per line, two columns, 17
    significant digits; ``header``: a comment line"""
    iv = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    with open(path, "w") as f:
        if header:
            f.write("# " + str(header).replace("\n", " ") + "\n")
        for lo, hi in iv:
            f.write(f"{float(lo)!r} {float(hi)!r}\n")
    return path


def write_calibration(path, table, half_width=10):
    """A calibration vector as an npz holding ``u0``, ``du``, ``mode`` ('log' or 'linear') and ``cal`` (float64, at the bin centres
    u0 + (j + 0.5) du).  ``table``: that dict, or an ``ObservedStack`` (its ``table(half_width)``)."""
    t = table.table(half_width) if hasattr(table, "table") else table
    np.savez(path, u0=np.float64(t["u0"]), du=np.float64(t["du"]), mode=np.asarray(str(t["mode"])),
             cal=np.asarray(t["cal"], dtype=np.float64).reshape(-1))
    return path


def read_calibration(path):
    """The dict u0, du, mode, cal of ``write_calibration`` (what ``qfa_amd.calibration.calibrate`` takes)"""
    with np.load(path) as z:
        missing = [k for k in ("u0", "du", "mode", "cal") if k not in z.files]
        if missing:
            raise ValueError(f"{path}: missing {missing}")
        return {"u0": float(z["u0"]), "du": float(z["du"]), "mode": str(z["mode"]), "cal": z["cal"].astype(np.float64).reshape(-1)}


def select_from_catalog(catalog, num, snr_min, snr_max, z_min, z_max, num_mask, output_dir=None, prefix="train"):
    """File names drawn from a catalogue csv with columns file, snr, z, num_mask
    (reference QFA/dataloader.py:48-55): the rows inside the S/N, redshift and masked-pixel limits,
    ``num`` of them drawn with ``np.random.choice`` (with replacement only when fewer than ``num``
    qualify -- the global numpy RNG, as the reference), and the draw written to
    ``<output_dir>/<prefix>-catalog.csv``."""
    import pandas as pd
    cat = pd.read_csv(catalog)
    ok = ((cat["snr"] >= snr_min) & (cat["snr"] <= snr_max) & (cat["z"] >= z_min) & (cat["z"] <= z_max)
          & (cat["num_mask"] <= num_mask))
    pool = cat["file"][ok].values
    if len(pool) == 0:
        raise ValueError("no catalogue row passes the selection")
    files = np.random.choice(pool, size=(num,), replace=(int(np.sum(ok)) < num))
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        pd.Series(files).to_csv(os.path.join(output_dir, f"{prefix}-catalog.csv"), header=False, index=False)
    return files


def read_prediction_catalog(catalog):
    """the file list of ``--type predict`` (reference QFA/dataloader.py:86-87): every value of the csv"""
    import pandas as pd
    return list(np.atleast_1d(pd.read_csv(catalog).values.squeeze()))


def load_from_catalog(catalog, data_dir, num, snr_min, snr_max, z_min, z_max, num_mask, nprocs=1, output_dir=None,
                      prefix="train"):
    """select + read (reference QFA/dataloader.py:48-55)"""
    files = select_from_catalog(catalog, num, snr_min, snr_max, z_min, z_max, num_mask, output_dir, prefix)
    return read_spectra([os.path.join(data_dir, x) for x in files], nprocs)
