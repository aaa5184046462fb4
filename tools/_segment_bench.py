"""What tools/bench_p1d.py, bench_p1d_band.py, bench_xi.py, bench_pdf.py and bench_variance.py share: the synthetic inputs of a
B:Nb:nseg:S shape with the z-bins of the eager compositions, the timing, the HBM floor and the record writer.  Each tool keeps its own
fused calls, eager composition, asserts and command line."""
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 4.0e12                                     # what the project's streaming kernels reach


def time_ms(fn, iters):
    """(median, min, max) ms of ``iters`` calls after a warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return {"median": t[0], "min": t[1], "max": t[2]}


def floor_ms(nsegs, L):
    """the time the 8 bytes per pixel-draw of the segments take at HBM_BYTES_PER_S"""
    return nsegs * L * 8 / HBM_BYTES_PER_S * 1e3


def inputs(spec, nz, dev, trans_lo=0.0, ivar_of=lambda u: 10.0 + 90.0 * u):
    """The inputs of shape ``spec`` = "B:Nb:nseg:S" under seed 0: trans uniform in [trans_lo, trans_lo + 1.2), ivar = ``ivar_of`` of a
    uniform number with 20 % of the pixels unused (segments on both sides of min_used), z = zq1 ratio - 1, tbar (S, 64) over
    [1.5, 3.6), ``nz`` z-bins over [1.6, 3.4).  ``kw``: the keywords every segment method takes.  For the eager forms: kT / okT, the
    tbar bin of a pixel and whether it has one; okz, whether a segment's central pixel has a z-bin; row (B, S, nseg), its row in a
    (S nz, ...) view of the stack."""
    import numpy as np
    import torch
    B, nb, nseg, S = (int(x) for x in spec.split(":"))
    L, nT = nb // nseg, 64
    min_used = int(np.ceil(0.75 * L))
    torch.manual_seed(0)
    trans = torch.rand((B, S, nb), device=dev) * 1.2 + trans_lo
    ivar = ivar_of(torch.rand((B, S, nb), device=dev))
    ivar.mul_(torch.rand((B, S, nb), device=dev) > 0.2)
    zq1 = (3.0 + 1.5 * torch.rand(B, device=dev)).contiguous()
    ratio = torch.tensor((10 ** np.linspace(np.log10(1030.0), np.log10(1215.0), nb) / 1215.67).astype(np.float32), device=dev)
    zabs = (zq1[:, None] * ratio[None, :] - 1.0).contiguous()
    zT0, dzT = np.float32(1.5), np.float32(2.1 / nT)
    z0, dz = np.float32(1.6), np.float32(1.8 / nz)
    tbar = (0.3 + 0.6 * torch.rand((S, nT), device=dev)).contiguous()
    kT = torch.floor((zabs - zT0) * (np.float32(1.0) / dzT)).long()
    okT = (kT >= 0) & (kT < nT)
    kT.clamp_(0, nT - 1)
    zc = zabs[:, torch.arange(nseg, device=dev) * L + L // 2]
    kz = torch.floor((zc - z0) * (np.float32(1.0) / dz)).long()
    okz = (kz >= 0) & (kz < nz)
    row = torch.arange(S, device=dev)[None, :, None] * nz + kz.clamp(0, nz - 1)[:, None, :]
    kw = dict(zabs=zabs, tbar=tbar, tbar_bins=(zT0, dzT, nT), seg_len=L, n_segments=nseg, min_used=min_used)
    return types.SimpleNamespace(B=B, nb=nb, nseg=nseg, S=S, L=L, nT=nT, nz=nz, min_used=min_used, trans=trans, ivar=ivar, zabs=zabs,
                                 tbar=tbar, z0=z0, dz=dz, kT=kT, okT=okT, okz=okz, row=row, kw=kw)


def write(out, rec):
    """print the record and append it to ``out`` (line by line: a later shape may not fit the device)"""
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")
