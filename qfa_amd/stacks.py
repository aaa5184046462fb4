"""The result classes of ``QFA``: ``EMStats``, the six stacks of the forest statistics, ``ForestStack``, ``P1DStack``,
``P1DBandStack``, ``XiStack``, ``PDFStack`` and ``VarianceStack``, and ``BootstrapStack``, the sightline bootstrap of the segment ones.  Views and arithmetic on buffers the kernels filled (include/qfa_hip.h): nothing here calls the library or
needs a GPU, the classes work on CPU tensors as well.  ``qfa_amd.model`` re-exports the names."""
from __future__ import annotations

import collections

import numpy as np
import torch

from ._lib import QFAHipError


class EMStats(object):
    """The packed sufficient statistics of the closed-form update of F (include/qfa_hip.h, qfa_em_floats):
    ``buf`` = [S2 (Npix, Nh, Nh) | S1 (Npix, Nh) | cnt (Npix,) | sum NLL, n_spectra, 0, 0] -- sums only, which is what data
    parallelism all-reduces.  ``S2``, ``S1``, ``cnt`` are views of ``buf``; ``loss`` is the (1, 1) mean NLL."""

    def __init__(self, buf, Npix, Nh):
        self.buf, self.Npix, self.Nh = buf, int(Npix), int(Nh)
        n2, n1 = self.Npix * self.Nh * self.Nh, self.Npix * self.Nh
        if buf.numel() != n2 + n1 + self.Npix + 4:
            raise QFAHipError(f"EMStats: {buf.numel()} floats, expected {n2 + n1 + self.Npix + 4}")
        self.S2 = buf[:n2].view(self.Npix, self.Nh, self.Nh)
        self.S1 = buf[n2:n2 + n1].view(self.Npix, self.Nh)
        self.cnt = buf[n2 + n1:n2 + n1 + self.Npix]
        self.tail = buf[n2 + n1 + self.Npix:]

    @property
    def loss(self):
        return (self.tail[0] / self.tail[1]).reshape(1, 1)

    def clone(self):
        return EMStats(self.buf.clone(), self.Npix, self.Nh)

    def blend_(self, other, rho):
        """self <- (1 - rho) self + rho other, in place (stochastic EM on mini-batches); rho = 1 is replacement, bit for bit."""
        rho = float(rho)
        if rho == 1.0:
            self.buf.copy_(other.buf)
        else:
            self.buf.mul_(1.0 - rho).add_(other.buf, alpha=rho)
        return self


def _mode_k(L, dv):
    """(M,) float64 numpy wavenumbers 2 pi m / (L dv), m = 1 .. M = L // 2, in s/km"""
    return 2.0 * np.pi * np.arange(1, int(L) // 2 + 1, dtype=np.float64) / (int(L) * float(dv))


def _window2(k, dv, resolution_kms):
    """W^2(k): the pixel's sinc times a Gaussian of ``resolution_kms`` (1 sigma), squared; ``k`` a float64 numpy array or
    torch tensor, evaluated in its own library"""
    xp = torch if isinstance(k, torch.Tensor) else np
    return (xp.sinc(k * dv / (2.0 * np.pi)) * xp.exp(-0.5 * (k * float(resolution_kms)) ** 2)) ** 2


def _f32(x):
    """x as the float32 number a kernel reads (an overflow is inf, quietly: the checks see it)"""
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def _edges(k_edges):
    """the checked band edges as a tuple of floats: the band stack's parameter rule"""
    e = tuple(float(x) for x in np.asarray(k_edges, np.float64).reshape(-1))
    if not (2 <= len(e) <= 65 and np.all(np.isfinite(e)) and np.all(np.diff(e) > 0.0)):
        raise QFAHipError(f"P1DBandStack: k_edges must be 2 .. 65 increasing finite wavenumbers, got {len(e)}")
    return e


def _check_segments(who, L, dv):
    if not (1 <= int(L) <= 4096 and float(dv) > 0.0 and np.isfinite(float(dv))):
        raise QFAHipError(f"{who}: segments L = {L}, dv = {dv}")


def _band_map(L, dv, k_edges):
    """(band, count): the (M,) int32 band of mode m = 1 .. M (entry m - 1; -1 = in no band) and the (nband,) int64 number of
    modes per band, as numpy arrays"""
    e = np.asarray(k_edges, np.float64)
    a = np.searchsorted(e, _mode_k(L, dv), side="right") - 1
    band = np.where((a >= 0) & (a < len(e) - 1), a, -1).astype(np.int32)
    return band, np.bincount(band[band >= 0], minlength=len(e) - 1).astype(np.int64)


class _DrawStack(object):
    """What the six stacks share: ``buf`` = (S, ...) contiguous float64 sums per draw of the continuum -- sums only, which is
    what data parallelism all-reduces -- over the z-bins [z0 + i dz, z0 + (i + 1) dz), z0 and dz as the float32 numbers the
    kernels bin with.  A class adds its layout (``_like``, ``same_layout``) and, where it is not ``mean``, the per-draw quantity
    the statistics over the draws are taken of (``_per_draw``), its parameter rule -- a static check that returns the parameters as the
    kernels will see them and raises ``QFAHipError``, the one place in Python where the bounds of the C checks are written -- and
    ``arrays()``, what the command line writes of it."""

    @staticmethod
    def _round_bins(z0, dz, n):
        """(z0, dz, n) as ``bins`` reports them: z0 and dz rounded to float32"""
        return float(np.float32(z0)), float(np.float32(dz)), int(n)

    def __init__(self, buf, z0, dz, n, tail):
        """``tail``: the shape of ``buf`` behind its first axis"""
        name = type(self).__name__
        self.z0, self.dz, self._nbins = self._round_bins(z0, dz, n)
        if buf.dtype != torch.float64 or buf.dim() != 3 or buf.shape[0] < 1 or tuple(buf.shape[1:]) != tuple(tail) \
                or not buf.is_contiguous():
            raise QFAHipError(f"{name}: buffer {tuple(buf.shape)} {buf.dtype}, expected contiguous float64 (S, {tail[0]}, {tail[1]})")
        if not (self.dz > 0.0 and np.isfinite(self.dz) and np.isfinite(self.z0) and 1 <= self._nbins <= 4096):
            raise QFAHipError(f"{name}: bins z0 = {z0}, dz = {dz}, n = {n}")
        self.buf = buf

    @property
    def S(self):
        return int(self.buf.shape[0])

    @property
    def bins(self):
        return (self.z0, self.dz, self._nbins)

    @property
    def z_edges(self):
        return self.z0 + self.dz * torch.arange(self._nbins + 1, dtype=torch.float64, device=self.buf.device)

    @property
    def z_centers(self):
        return self.z0 + self.dz * (torch.arange(self._nbins, dtype=torch.float64, device=self.buf.device) + 0.5)

    def _export(self, **named):
        """``arrays()``: tensors as numpy arrays on the host, scalars as they are"""
        return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in named.items()}

    def _per_draw(self):
        return self.mean

    def _draws(self, what):
        if self.S < 2:
            raise QFAHipError(f"{type(self).__name__}.{what}: needs more than one draw of the continuum (S = {self.S})")
        return self._per_draw()

    @property
    def mean_over_draws(self):
        """mean of the per-draw result (``mean``; ``power()`` of a ``P1DStack``) over the S posterior draws of the continuum"""
        return self._draws("mean_over_draws").mean(0)

    def draws(self, s0, s1):
        """the stack of draws [s0, s1): a view of the same buffer"""
        return self._like(self.buf[s0:s1])

    def clone(self):
        return self._like(self.buf.clone())

    def same_layout(self, other):
        return isinstance(other, type(self)) and other.bins == self.bins

    def add_(self, other):
        if not self.same_layout(other) or other.S != self.S:
            raise QFAHipError(f"{type(self).__name__}.add_: the other stack's bins / segments / bands / draws differ from "
                              f"{self.bins}, {self.S}")
        self.buf.add_(other.buf)
        return self

    def all_reduce(self, group=None):
        """in-place sum over the process group (every rank calls it; an exhausted rank adds zeros)"""
        from .distributed import all_reduce_accum
        all_reduce_accum(self.buf.view(-1), group)
        return self


class ForestStack(_DrawStack):
    """The redshift-binned stack of the forest transmission (include/qfa_hip.h, qfa_forest_f32): ``buf`` = (S, 4, nbin) float64
    [sum w | sum w T | sum w T^2 | n] per draw of the continuum over the bins [z0 + k dz, z0 + (k + 1) dz)."""

    def __init__(self, buf, z0, dz, nbin):
        super().__init__(buf, z0, dz, nbin, (4, int(nbin)))
        self.nbin = self._nbins

    @classmethod
    def zeros(cls, S, z0, dz, nbin, device):
        return cls(torch.zeros((int(S), 4, int(nbin)), dtype=torch.float64, device=device), z0, dz, nbin)

    def _like(self, buf):
        return ForestStack(buf, self.z0, self.dz, self.nbin)

    @property
    def sum_w(self):
        return self.buf[:, 0]

    @property
    def n(self):
        """(S, nbin) number of pixels stacked"""
        return self.buf[:, 3]

    @property
    def mean(self):
        """(S, nbin) weighted mean transmission sum w T / sum w (NaN in an empty bin)"""
        return self.buf[:, 1] / self.buf[:, 0]

    @property
    def var(self):
        """(S, nbin) weighted variance of T inside the bin, sum w T^2 / sum w - mean^2"""
        m = self.mean
        return self.buf[:, 2] / self.buf[:, 0] - m * m

    @property
    def tau_eff(self):
        """(S, nbin) effective optical depth -ln <T>"""
        return -torch.log(self.mean)

    @property
    def std_over_draws(self):
        """(nbin,) standard deviation of ``mean`` over the S draws: the continuum posterior's error bar on the stack (the
        continuum errors of a spectrum's pixels are correlated, which repeating the whole stack per draw carries through)"""
        return self._draws("std_over_draws").std(0, unbiased=True)

    def arrays(self):
        """what mean_transmission.npz holds"""
        return self._export(z_centers=self.z_centers, z_edges=self.z_edges, mean=self.mean, var=self.var, n=self.n, tau_eff=self.tau_eff,
                            sums=self.buf)


class _SegmentStack(_DrawStack):
    """A stack over segments of ``L`` pixels ``dv`` km/s wide, M = L // 2 modes k_m = 2 pi m / (L dv): ``buf`` = (S, nz, width),
    the number of segments stacked first."""

    def __init__(self, buf, z0, dz, nz, L, dv, width):
        self.L, self.dv = int(L), float(dv)
        self.M = self.L // 2
        super().__init__(buf, z0, dz, nz, (int(nz), width))
        self.nz = self._nbins
        _check_segments(type(self).__name__, L, dv)

    @property
    def n(self):
        """(S, nz) number of segments stacked"""
        return self.buf[:, :, 0]

    def same_layout(self, other):
        return super().same_layout(other) and other.L == self.L and other.dv == self.dv


class P1DStack(_SegmentStack):
    """The (k, z) stack of the 1D flux power spectrum (include/qfa_hip.h, qfa_p1d_f32): ``buf`` = (S, nz, 2 + 2M) float64
    [n | sum N | sum P_1..M | sum P^2_1..M] per draw of the continuum and z-bin."""

    def __init__(self, buf, z0, dz, nz, L, dv=1.0):
        super().__init__(buf, z0, dz, nz, L, dv, 2 + 2 * (int(L) // 2))

    @classmethod
    def zeros(cls, S, z0, dz, nz, L, dv, device):
        return cls(torch.zeros((int(S), int(nz), 2 + 2 * (int(L) // 2)), dtype=torch.float64, device=device), z0, dz, nz, L, dv)

    def _like(self, buf):
        return P1DStack(buf, self.z0, self.dz, self.nz, self.L, self.dv)

    @property
    def k(self):
        """(M,) wavenumbers 2 pi m / (L dv), m = 1 .. M, in s/km"""
        return torch.tensor(_mode_k(self.L, self.dv), dtype=torch.float64, device=self.buf.device)

    @property
    def noise(self):
        """(S, nz) mean noise level <N> of the stacked segments, in pixel units (NaN in an empty bin)"""
        return self.buf[:, :, 1] / self.n

    @property
    def power_raw(self):
        """(S, nz, M) mean |delta~_m|^2 / L of the stacked segments, in pixel units, noise included"""
        return self.buf[:, :, 2:2 + self.M] / self.n[:, :, None]

    def window2(self, resolution_kms):
        """(M,) W^2(k): the pixel's sinc times a Gaussian of ``resolution_kms`` (1 sigma), squared"""
        return _window2(self.k, self.dv, resolution_kms)

    def power(self, resolution_kms=None):
        """(S, nz, M) P1D in km/s: (power_raw - noise) dv, divided by ``window2(resolution_kms)`` when that is given"""
        P = (self.power_raw - self.noise[:, :, None]) * self.dv
        return P if resolution_kms is None else P / self.window2(resolution_kms)

    def err(self, resolution_kms=None):
        """(S, nz, M) standard error of ``power`` from the scatter of the segments: sqrt((<P^2> - <P>^2) / (n - 1)) dv"""
        m2 = self.buf[:, :, 2 + self.M:] / self.n[:, :, None]
        var = (m2 - self.power_raw ** 2).clamp_min(0.0) / (self.n[:, :, None] - 1.0)
        e = torch.sqrt(var) * self.dv
        e = torch.where(self.n[:, :, None] > 1.0, e, torch.full_like(e, float("nan")))
        return e if resolution_kms is None else e / self.window2(resolution_kms)

    def _per_draw(self):
        return self.power()

    @property
    def std_over_draws(self):
        """(nz, M) standard deviation of ``power()`` over the S draws: the continuum posterior's error bar on P1D"""
        return self._draws("std_over_draws").std(0, unbiased=True)

    def arrays(self):
        """what flux_power.npz holds"""
        return self._export(k=self.k, z_centers=self.z_centers, z_edges=self.z_edges, power=self.power(), err=self.err(),
                            power_raw=self.power_raw, noise=self.noise, n=self.n, seg_len=self.L, dv=self.dv, sums=self.buf)

    @staticmethod
    def bootstrap_estimate(sums, dv=1.0):
        """``power()`` of bootstrap sums (..., 2 + M) = [sum w | sum w N | sum w P_1..M] of the rows [noise | power]: (..., M)"""
        return (sums[..., 2:] - sums[..., 1:2]) / sums[..., 0:1] * float(dv)


class P1DBandStack(_SegmentStack):
    """The stack of band powers of the 1D flux power spectrum and of their outer products (include/qfa_hip.h, qfa_p1d_band_f32):
    ``buf`` = (S, nz, 1 + nband + nband^2) float64 [n | sum Q_a | sum Q_a Q_b] per draw of the continuum and z-bin.  Band a holds
    the modes with ``k_edges[a] <= k_m < k_edges[a + 1]``, k_m in s/km; Q_a is the band's mean power of one segment in km/s
    (``QFA.p1d_bands`` folds dv, 1 / n_a and the window into the weights)."""

    def __init__(self, buf, z0, dz, nz, L, dv, k_edges):
        self._k_edges = _edges(k_edges)
        self.nband = len(self._k_edges) - 1
        super().__init__(buf, z0, dz, nz, L, dv, 1 + self.nband + self.nband ** 2)

    @classmethod
    def zeros(cls, S, z0, dz, nz, L, dv, k_edges, device):
        nband = len(_edges(k_edges)) - 1
        return cls(torch.zeros((int(S), int(nz), 1 + nband + nband * nband), dtype=torch.float64, device=device), z0, dz, nz, L, dv,
                   k_edges)

    @staticmethod
    def linear_k_edges(L, dv, nband):
        """nband + 1 edges of equal bands from the fundamental to Nyquist: mode m sits at m k_1 inside [k_1 / 2, (M + 1 / 2) k_1)"""
        return 2.0 * np.pi / (int(L) * float(dv)) * np.linspace(0.5, int(L) // 2 + 0.5, int(nband) + 1)

    def _like(self, buf):
        return P1DBandStack(buf, self.z0, self.dz, self.nz, self.L, self.dv, self._k_edges)

    def same_layout(self, other):
        return super().same_layout(other) and other._k_edges == self._k_edges

    @property
    def k_edges(self):
        """(nband + 1,) band edges in s/km"""
        return torch.tensor(self._k_edges, dtype=torch.float64, device=self.buf.device)

    def band_map(self):
        """(band, count): the (M,) int32 band of mode m = 1 .. M (entry m - 1; -1 = in no band) and the (nband,) int64 number of
        modes per band, as numpy arrays"""
        return _band_map(self.L, self.dv, self._k_edges)

    @property
    def k_centers(self):
        """(nband,) mean wavenumber of a band's modes in s/km (NaN for a band without modes)"""
        band, count = self.band_map()
        tot = np.bincount(band[band >= 0], weights=_mode_k(self.L, self.dv)[band >= 0], minlength=self.nband)
        with np.errstate(all="ignore"):
            c = np.where(count > 0, tot / count, np.nan)
        return torch.tensor(c, dtype=torch.float64, device=self.buf.device)

    @property
    def mean(self):
        """(S, nz, nband) mean band power of the stacked segments (NaN in an empty bin)"""
        return self.buf[:, :, 1:1 + self.nband] / self.n[:, :, None]

    @property
    def cov(self):
        """(S, nz, nband, nband) covariance of ``mean`` from the scatter of the segments: (<Q Q^T> - <Q> <Q>^T) / (n - 1); NaN
        where n < 2"""
        n = self.n[:, :, None, None]
        m2 = self.buf[:, :, 1 + self.nband:].reshape(self.S, self.nz, self.nband, self.nband) / n
        mu = self.mean
        c = (m2 - mu[:, :, :, None] * mu[:, :, None, :]) / (n - 1.0)
        return torch.where(n > 1.0, c, torch.full_like(c, float("nan")))

    @property
    def err(self):
        """(S, nz, nband) standard error of ``mean``: the root of the diagonal of ``cov``"""
        return torch.sqrt(torch.diagonal(self.cov, dim1=2, dim2=3).clamp_min(0.0))

    @property
    def corr(self):
        """(S, nz, nband, nband) correlation matrix of the bands: cov_ab / sqrt(cov_aa cov_bb)"""
        c = self.cov
        d = torch.sqrt(torch.diagonal(c, dim1=2, dim2=3).clamp_min(0.0))
        return c / (d[:, :, :, None] * d[:, :, None, :])

    @property
    def cov_over_draws(self):
        """(nz, nband, nband) covariance of ``mean`` over the S draws: the continuum posterior's covariance of the band powers"""
        d = self._draws("cov_over_draws")
        d = d - d.mean(0, keepdim=True)
        return torch.einsum("sza,szb->zab", d, d) / (self.S - 1.0)

    @property
    def total_cov(self):
        """(nz, nband, nband) the mean over the draws of ``cov`` plus ``cov_over_draws``"""
        return self.cov.mean(0) + self.cov_over_draws

    def arrays(self):
        """what flux_power_bands.npz holds; ``cov_over_draws`` with more than one draw"""
        over = {"cov_over_draws": self.cov_over_draws} if self.S > 1 else {}
        return self._export(k_edges=self.k_edges, k_centers=self.k_centers, z_edges=self.z_edges, n=self.n, mean=self.mean, cov=self.cov,
                            **over)

    @staticmethod
    def bootstrap_estimate(sums):
        """``mean`` of bootstrap sums (..., 1 + nband) = [sum w | sum w Q_a] of the rows bandpower: (..., nband)"""
        return sums[..., 1:] / sums[..., 0:1]


class XiStack(_SegmentStack):
    """The (lag, z) stack of the pair-weighted line-of-sight correlation function (include/qfa_hip.h, qfa_xi_f32): ``buf`` =
    (S, nz, 2 + 5 nlag) float64 [n | sum N0 | sum W_l | sum A_l | sum W_l^2 | sum A_l W_l | sum A_l^2] per draw of the continuum and
    z-bin, over segments of ``L`` pixels ``dv`` km/s wide; W_l and A_l are a segment's sums of w_j w_{j+l} and of
    w_j w_{j+l} d_j d_{j+l}, N0 the noise in A_0."""

    @staticmethod
    def lag_params(L, n_lags):
        """the checked number of lags on segments of ``L`` pixels"""
        if not 1 <= int(n_lags) <= int(L):
            raise QFAHipError(f"XiStack: {n_lags} lags on segments of {L} pixels")
        return int(n_lags)

    def __init__(self, buf, z0, dz, nz, L, n_lags, dv=1.0):
        self.nlag = self.lag_params(L, n_lags)
        super().__init__(buf, z0, dz, nz, L, dv, 2 + 5 * self.nlag)

    @classmethod
    def zeros(cls, S, z0, dz, nz, L, n_lags, dv, device):
        nlag = cls.lag_params(L, n_lags)
        return cls(torch.zeros((int(S), int(nz), 2 + 5 * nlag), dtype=torch.float64, device=device), z0, dz, nz, L, nlag, dv)

    def _like(self, buf):
        return XiStack(buf, self.z0, self.dz, self.nz, self.L, self.nlag, self.dv)

    def same_layout(self, other):
        return super().same_layout(other) and other.nlag == self.nlag

    def _part(self, i):
        return self.buf[:, :, 2 + i * self.nlag:2 + (i + 1) * self.nlag]

    @property
    def lags_kms(self):
        """(nlag,) velocity separations l dv in km/s"""
        return self.dv * torch.arange(self.nlag, dtype=torch.float64, device=self.buf.device)

    @property
    def noise0(self):
        """(S, nz) sum N0 of the stacked segments: the noise in sum A_0"""
        return self.buf[:, :, 1]

    @property
    def sum_w(self):
        """(S, nz, nlag) sum W_l: the pair weight behind every lag"""
        return self._part(0)

    def xi(self, subtract_noise=True):
        """(S, nz, nlag) xi_l = sum A_l / sum W_l, with sum N0 taken off lag 0 unless ``subtract_noise`` is False; NaN where
        sum W_l = 0"""
        A = self._part(1)
        if subtract_noise:
            A = A.clone()
            A[:, :, 0] -= self.noise0
        W = self.sum_w
        x = A / W
        return torch.where(W != 0.0, x, torch.full_like(x, float("nan")))

    def err(self):
        """(S, nz, nlag) standard error of ``xi(subtract_noise=False)`` from the scatter of the segments, the delta method of a
        ratio of sums: sqrt((sum A^2 - 2 xi sum A W + xi^2 sum W^2) / (sum W)^2 n / (n - 1)); NaN below two segments.  (The noise
        taken off lag 0 moves its mean, not, to this order, its scatter.)"""
        W, x = self.sum_w, self.xi(subtract_noise=False)
        n = self.n[:, :, None]
        num = (self._part(4) - 2.0 * x * self._part(3) + x * x * self._part(2)).clamp_min(0.0)
        e = torch.sqrt(num / (W * W) * n / (n - 1.0))
        return torch.where((n > 1.0) & (W != 0.0), e, torch.full_like(e, float("nan")))

    def _per_draw(self):
        return self.xi()

    @property
    def std_over_draws(self):
        """(nz, nlag) standard deviation of ``xi()`` over the S draws: the continuum posterior's error bar on xi"""
        return self._draws("std_over_draws").std(0, unbiased=True)

    def arrays(self):
        """what flux_correlation.npz holds"""
        return self._export(lags_kms=self.lags_kms, z_centers=self.z_centers, z_edges=self.z_edges, xi=self.xi(),
                            xi_raw=self.xi(subtract_noise=False), err=self.err(), n=self.n, sum_w=self.sum_w, seg_len=self.L, dv=self.dv,
                            sums=self.buf)

    @staticmethod
    def bootstrap_estimate(sums, nlag, subtract_noise=True):
        """``xi()`` of bootstrap sums (..., 2 + 2 nlag) = [sum w | sum w N0 | sum w W_l | sum w A_l] of the rows [noise0 | pairs]:
        (..., nlag), NaN where sum w W_l = 0"""
        W, A = sums[..., 2:2 + nlag], sums[..., 2 + nlag:2 + 2 * nlag]
        if subtract_noise:
            A = A.clone()
            A[..., 0] -= sums[..., 1]
        x = A / W
        return torch.where(W != 0.0, x, torch.full_like(x, float("nan")))


class PDFStack(_DrawStack):
    """The stack of the flux PDF of forest segments and of the outer products of their counts (include/qfa_hip.h,
    qfa_flux_pdf_f32): ``buf`` = (S, nz, 2 + nt + nt^2) float64 [n_seg | sum n_cnt | sum h_a | sum h_a h_b] per draw of the continuum
    and z-bin, over segments of ``L`` pixels; h_a is a segment's number of counted pixels in the flux bin
    [t0 + a dt, t0 + (a + 1) dt), n_cnt its number of counted pixels in a bin or not.  ``relative``: the bins are of T / <T>(z);
    ``clamp``: pixels outside the range sit in the first / last bin; ``ivar_min``: the least inverse variance of a counted pixel.
    Every entry is an integer, exact below 2^53: stacks add up exactly, in any order.  t0 and dt are held as the float32 numbers
    the kernel bins with."""

    @staticmethod
    def flux_params(t0, dt, n_tbins, relative=False, clamp=False, ivar_min=0.0):
        """(t0, dt, nt, relative, clamp, ivar_min) checked, t0, dt and ivar_min as the float32 numbers the kernel reads"""
        p = (_f32(t0), _f32(dt), int(n_tbins), bool(relative), bool(clamp), _f32(ivar_min))
        if not (1 <= p[2] <= 64 and p[1] > 0.0 and np.isfinite(p[1]) and np.isfinite(p[0]) and p[5] >= 0.0 and np.isfinite(p[5])):
            raise QFAHipError(f"PDFStack: {n_tbins} flux bins from {t0} in steps of {dt}, ivar_min = {ivar_min}")
        return p

    def __init__(self, buf, z0, dz, nz, L, t0, dt, n_tbins, relative=False, clamp=False, ivar_min=0.0):
        self.t0, self.dt, self.nt, self.relative, self.clamp, self.ivar_min = self.flux_params(t0, dt, n_tbins, relative, clamp, ivar_min)
        self.L = int(L)
        _check_segments("PDFStack", L, 1.0)
        super().__init__(buf, z0, dz, nz, (int(nz), 2 + self.nt + self.nt ** 2))
        self.nz = self._nbins

    @classmethod
    def zeros(cls, S, z0, dz, nz, L, t0, dt, n_tbins, relative=False, clamp=False, ivar_min=0.0, device="cpu"):
        nt = cls.flux_params(t0, dt, n_tbins, relative, clamp, ivar_min)[2]
        return cls(torch.zeros((int(S), int(nz), 2 + nt + nt * nt), dtype=torch.float64, device=device), z0, dz, nz, L, t0, dt, nt,
                   relative, clamp, ivar_min)

    def _like(self, buf):
        return PDFStack(buf, self.z0, self.dz, self.nz, self.L, self.t0, self.dt, self.nt, self.relative, self.clamp, self.ivar_min)

    @property
    def flux_bins(self):
        """(t0, dt, nt), t0 and dt as the float32 numbers the kernel bins with"""
        return (self.t0, self.dt, self.nt)

    def same_layout(self, other):
        return super().same_layout(other) and other.L == self.L and other.flux_bins == self.flux_bins and \
            (other.relative, other.clamp, other.ivar_min) == (self.relative, self.clamp, self.ivar_min)

    @property
    def z_centres(self):
        return self.z_centers

    @property
    def t_edges(self):
        """(nt + 1,) edges of the flux bins"""
        return self.t0 + self.dt * torch.arange(self.nt + 1, dtype=torch.float64, device=self.buf.device)

    @property
    def t_centres(self):
        """(nt,) centres of the flux bins"""
        return self.t0 + self.dt * (torch.arange(self.nt, dtype=torch.float64, device=self.buf.device) + 0.5)

    @property
    def n_segments(self):
        """(S, nz) number of segments stacked"""
        return self.buf[:, :, 0]

    @property
    def n_pixels(self):
        """(S, nz) number of counted pixels of the stacked segments, in a bin or not"""
        return self.buf[:, :, 1]

    @property
    def counts(self):
        """(S, nz, nt) H_a: counted pixels per flux bin"""
        return self.buf[:, :, 2:2 + self.nt]

    @property
    def outer(self):
        """(S, nz, nt, nt) M_ab = sum over the segments of h_a h_b"""
        return self.buf[:, :, 2 + self.nt:].reshape(self.S, self.nz, self.nt, self.nt)

    def pdf(self):
        """(S, nz, nt) P_a = H_a / (N dt) with N = sum_a H_a: normalised over the in-range pixels, so that sum_a P_a dt = 1; NaN
        where N = 0"""
        H = self.counts
        N = H.sum(-1, keepdim=True)
        p = H / (N * self.dt)
        return torch.where(N > 0.0, p, torch.full_like(p, float("nan")))

    def out_of_range(self):
        """(S, nz) 1 - N / sum n_cnt: the fraction of counted pixels no bin holds (0 under ``clamp`` unless x is NaN); NaN
        without pixels"""
        f = 1.0 - self.counts.sum(-1) / self.n_pixels
        return torch.where(self.n_pixels > 0.0, f, torch.full_like(f, float("nan")))

    def cov(self):
        """(S, nz, nt, nt) covariance of ``pdf()``: the delta method of the ratio estimator with segments as the independent units,
        Cov_ab = n / (n - 1) sum_seg (h_a - r_a m)(h_b - r_b m) / (dt^2 N^2), r_a = H_a / N, m = sum_a h_a of a segment.  It is
        formed in float64 from the stacked M = sum h h^T as M_ab - r_b sum_c M_ac - r_a sum_c M_bc + r_a r_b sum_cd M_cd.  Its rows
        sum to zero by construction -- the PDF is normalised, it has nt - 1 degrees of freedom: the matrix is singular and a fit
        must drop a bin.  NaN below two segments or without pixels."""
        M, H = self.outer, self.counts
        N = H.sum(-1)
        r = H / N[:, :, None]
        rows = M.sum(-1)                                          # (S, nz, nt) sum_c M_ac: integers, exact
        tot = rows.sum(-1)
        ra, rb = r[:, :, :, None], r[:, :, None, :]
        c = M - rb * rows[:, :, :, None] - ra * rows[:, :, None, :] + ra * rb * tot[:, :, None, None]
        n = self.n_segments[:, :, None, None]
        N2 = (N * N)[:, :, None, None]
        c = n / (n - 1.0) * c / (self.dt * self.dt * N2)
        return torch.where((n > 1.0) & (N2 > 0.0), c, torch.full_like(c, float("nan")))

    def err(self):
        """(S, nz, nt) standard error of ``pdf()``: the root of the diagonal of ``cov()``"""
        return torch.sqrt(torch.diagonal(self.cov(), dim1=2, dim2=3).clamp_min(0.0))

    def corr(self):
        """(S, nz, nt, nt) correlation matrix of the flux bins: cov_ab / sqrt(cov_aa cov_bb)"""
        c = self.cov()
        d = torch.sqrt(torch.diagonal(c, dim1=2, dim2=3))
        return c / (d[:, :, :, None] * d[:, :, None, :])

    def _per_draw(self):
        return self.pdf()

    @property
    def std_over_draws(self):
        """(nz, nt) standard deviation of ``pdf()`` over the S draws: the continuum posterior's error bar on the PDF"""
        return self._draws("std_over_draws").std(0, unbiased=True)

    @property
    def cov_over_draws(self):
        """(nz, nt, nt) covariance of ``pdf()`` over the S draws: the continuum posterior's covariance of the flux bins"""
        d = self._draws("cov_over_draws")
        d = d - d.mean(0, keepdim=True)
        return torch.einsum("sza,szb->zab", d, d) / (self.S - 1.0)

    @property
    def total_cov(self):
        """(nz, nt, nt) the mean over the draws of ``cov()`` plus ``cov_over_draws``"""
        return self.cov().mean(0) + self.cov_over_draws

    def arrays(self):
        """what flux_pdf.npz holds; ``std_over_draws`` and ``total_cov`` with more than one draw"""
        over = {"std_over_draws": self.std_over_draws, "total_cov": self.total_cov} if self.S > 1 else {}
        return self._export(z=self.z_centers, t_edges=self.t_edges, pdf=self.pdf(), err=self.err(), cov=self.cov(), counts=self.counts,
                            n_segments=self.n_segments, out_of_range=self.out_of_range(), **over)

    @staticmethod
    def bootstrap_estimate(sums, dt):
        """``pdf()`` of bootstrap sums (..., 1 + nt) = [sum w | sum w h_a] of the rows hist: (..., nt), NaN without pixels"""
        H = sums[..., 1:]
        N = H.sum(-1, keepdim=True)
        p = H / (N * float(dt))
        return torch.where(N > 0.0, p, torch.full_like(p, float("nan")))


# what ``VarianceStack.fit`` returns: (S, nz) tensors, ``cov`` (S, nz, P, P) in the order (eta, sigma2_lss[, eps]); ``eps`` None
# without the third term
VarianceFit = collections.namedtuple("VarianceFit", "eta sigma2_lss eps cov chi2 ndof n_bins")


def _sym_inverse(N):
    """(inverse, determinant) of (..., P, P) symmetric matrices, P = 2 or 3, by cofactors: elementwise arithmetic only"""
    P = N.shape[-1]
    if P == 2:
        a, b, d = N[..., 0, 0], N[..., 0, 1], N[..., 1, 1]
        det = a * d - b * b
        inv = torch.stack([torch.stack([d, -b], -1), torch.stack([-b, a], -1)], -2)
        return inv / det[..., None, None], det
    a, b, c, d, e, f = N[..., 0, 0], N[..., 0, 1], N[..., 0, 2], N[..., 1, 1], N[..., 1, 2], N[..., 2, 2]
    A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
    D, E, F = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * A + b * B + c * Cc
    inv = torch.stack([torch.stack([A, B, Cc], -1), torch.stack([B, D, E], -1), torch.stack([Cc, E, F], -1)], -2)
    return inv / det[..., None, None], det


class VarianceStack(_SegmentStack):
    """The (v-bin, z) stack of the variance function of the forest (include/qfa_hip.h, qfa_variance_f32): ``buf`` =
    (S, nz, 2 + 5 nv) float64 [n_seg | n_used | n_a | sum v_a | sum d_a | sum d^2_a | sum d^4_a] per draw of the continuum and z-bin,
    over segments of ``L`` pixels; d = delta_F of a pixel, v the pipeline's noise variance of d.  The nv = ``n_oct`` << ``sub`` bins of
    v are defined on the bits of the float32 v, 2^sub per octave from 2^``e_lo`` on (``v_edges``); a pixel with |d| > ``d_max``
    (float32; None = the largest finite float32, which cuts the non-finite d alone) is left out.  ``fit`` turns the stack into
    eta(z) and sigma2_lss(z) of var(d) = eta v + sigma2_lss."""

    FLT_MAX = float(np.finfo(np.float32).max)

    @classmethod
    def var_params(cls, e_lo, n_oct, sub=1, d_max=None):
        """(e_lo, n_oct, sub, d_max) checked -- what ``var_bins`` reports --, d_max as the float32 number the kernel cuts with"""
        p = (int(e_lo), int(n_oct), int(sub), cls.FLT_MAX if d_max is None else _f32(d_max))
        if not (0 <= p[2] <= 4 and p[1] >= 1 and 1 <= (p[1] << p[2]) <= 64 and p[0] >= -126 and p[0] + p[1] <= 127 and p[3] > 0.0):
            raise QFAHipError(f"VarianceStack: e_lo = {e_lo}, n_oct = {n_oct}, sub = {sub}, d_max = {d_max}")
        return p

    def __init__(self, buf, z0, dz, nz, L, e_lo, n_oct, sub=1, d_max=None):
        self.e_lo, self.n_oct, self.sub, self.d_max = self.var_params(e_lo, n_oct, sub, d_max)
        self.nv = self.n_oct << self.sub
        super().__init__(buf, z0, dz, nz, L, 1.0, 2 + 5 * self.nv)

    @classmethod
    def zeros(cls, S, z0, dz, nz, L, e_lo, n_oct, sub=1, d_max=None, device="cpu"):
        p = cls.var_params(e_lo, n_oct, sub, d_max)
        nv = p[1] << p[2]
        return cls(torch.zeros((int(S), int(nz), 2 + 5 * nv), dtype=torch.float64, device=device), z0, dz, nz, L, e_lo, n_oct, sub, d_max)

    def _like(self, buf):
        return VarianceStack(buf, self.z0, self.dz, self.nz, self.L, self.e_lo, self.n_oct, self.sub, self.d_max)

    @property
    def var_bins(self):
        """(e_lo, n_oct, sub, d_max), d_max as the float32 number the kernel cuts with"""
        return (self.e_lo, self.n_oct, self.sub, self.d_max)

    def same_layout(self, other):
        return super().same_layout(other) and other.var_bins == self.var_bins

    def _part(self, i):
        return self.buf[:, :, 2 + i * self.nv:2 + (i + 1) * self.nv]

    @property
    def v_edges(self):
        """(nv + 1,) edges of the variance bins, exact: 2^(e_lo + (c >> sub)) (1 + (c & (2^sub - 1)) / 2^sub), c = 0 .. nv; an edge
        belongs to the bin above it"""
        c = np.arange(self.nv + 1)
        e = np.ldexp(1.0 + (c & ((1 << self.sub) - 1)) / float(1 << self.sub), self.e_lo + (c >> self.sub))
        return torch.tensor(e, dtype=torch.float64, device=self.buf.device)

    @property
    def n_segments(self):
        """(S, nz) number of segments stacked"""
        return self.buf[:, :, 0]

    @property
    def n_pixels(self):
        """(S, nz) number of used pixels of the stacked segments, in a bin or not"""
        return self.buf[:, :, 1]

    @property
    def counts(self):
        """(S, nz, nv) n_a: counted pixels per variance bin"""
        return self._part(0)

    def out_of_range(self):
        """(S, nz) 1 - sum_a n_a / n_used: the fraction of used pixels that no bin holds or the cut on |d| removed; NaN without
        pixels"""
        f = 1.0 - self.counts.sum(-1) / self.n_pixels
        return torch.where(self.n_pixels > 0.0, f, torch.full_like(f, float("nan")))

    @property
    def v_mean(self):
        """(S, nz, nv) mean pipeline variance <v> of a bin's pixels (NaN in an empty bin)"""
        return self._part(1) / self.counts

    @property
    def mean_delta(self):
        """(S, nz, nv) <d> of a bin's pixels"""
        return self._part(2) / self.counts

    @property
    def var_delta(self):
        """(S, nz, nv) the variance function <d^2> - <d>^2 of a bin's pixels (NaN in an empty bin)"""
        m = self.mean_delta
        return self._part(3) / self.counts - m * m

    @property
    def var_err(self):
        """(S, nz, nv) standard error of ``var_delta`` from the fourth moment: sqrt((<d^4> - <d^2>^2) / n_a)"""
        n = self.counts
        m2 = self._part(3) / n
        return torch.sqrt(((self._part(4) / n - m2 * m2) / n).clamp_min(0.0))

    def fit(self, min_count=100, epsilon=False):
        """The weighted least squares fit var_delta = eta v_mean + sigma2_lss (+ eps / v_mean with ``epsilon``) per draw and z-bin,
        in closed form in float64 on the stack's device: over the bins with n_a >= ``min_count`` and var_err > 0, weights
        1 / var_err^2.  The normal matrix is scaled to a unit diagonal and inverted by cofactors.  Returns a ``VarianceFit`` of
        (S, nz) tensors: ``eta``, ``sigma2_lss``, ``eps`` (None without ``epsilon``), ``cov`` (S, nz, P, P) of the P parameters in that
        order, ``chi2``, ``ndof`` = n_bins - P and ``n_bins``, the usable bins.  A cell with fewer usable bins than parameters, or
        whose scaled normal matrix has a determinant below 64 x 2^-52 (singular), gets NaN.  ``sigma2_lss`` is the number
        ``QFA.xi`` / ``QFA.flux_correlation`` take as their one scalar ``sigma2_lss``."""
        P = 3 if epsilon else 2
        x, y, e = self.v_mean, self.var_delta, self.var_err
        ok = (self.counts >= float(min_count)) & (e > 0.0) & torch.isfinite(e) & torch.isfinite(y) & (x > 0.0)
        zero, one = torch.zeros_like(x), torch.ones_like(x)
        w = torch.where(ok, 1.0 / torch.where(ok, e * e, one), zero)
        xs, ys = torch.where(ok, x, one), torch.where(ok, y, zero)
        cols = [xs, one] + ([1.0 / xs] if epsilon else [])
        f = torch.stack(cols, -1)                                 # (S, nz, nv, P)
        N = torch.einsum("szc,szcp,szcq->szpq", w, f, f)
        r = torch.einsum("szc,szcp,szc->szp", w, f, ys)
        n_bins = ok.sum(-1).to(torch.float64)
        sc = torch.sqrt(torch.diagonal(N, dim1=2, dim2=3))        # (S, nz, P)
        good = (n_bins >= P) & (sc > 0.0).all(-1)
        sc = torch.where(good[..., None], sc, torch.ones_like(sc))
        eye = torch.eye(P, dtype=torch.float64, device=self.buf.device).expand_as(N)
        Ns = torch.where(good[..., None, None], N / (sc[..., :, None] * sc[..., None, :]), eye)
        inv, det = _sym_inverse(Ns)
        good = good & (det > 64.0 * 2.0 ** -52)
        par = torch.einsum("szpq,szq->szp", inv, r / sc) / sc
        cov = inv / (sc[..., :, None] * sc[..., None, :])
        res = ys - torch.einsum("szcp,szp->szc", f, par)
        chi2 = (w * res * res).sum(-1)
        nan = torch.full_like(n_bins, float("nan"))
        par = torch.where(good[..., None], par, nan[..., None])
        cov = torch.where(good[..., None, None], cov, nan[..., None, None])
        chi2 = torch.where(good, chi2, nan)
        return VarianceFit(par[..., 0], par[..., 1], par[..., 2] if epsilon else None, cov, chi2, n_bins - P, n_bins)

    @staticmethod
    def bootstrap_estimate(sums, nv):
        """``var_delta`` of bootstrap sums (..., 1 + 5 nv) = [sum w | sum w (n_a | sum v | sum d | sum d^2 | sum d^4)] of the rows
        moments: (..., nv)"""
        n = sums[..., 1:1 + nv]
        m = sums[..., 1 + 2 * nv:1 + 3 * nv] / n
        return sums[..., 1 + 3 * nv:1 + 4 * nv] / n - m * m

    def _per_draw(self):
        return self.var_delta

    def std_over_draws(self, min_count=100):
        """((nz,), (nz,)) standard deviation of ``fit(min_count)``'s eta and sigma2_lss over the S draws: the continuum posterior's
        error bar on both"""
        if self.S < 2:
            raise QFAHipError(f"VarianceStack.std_over_draws: needs more than one draw of the continuum (S = {self.S})")
        ft = self.fit(min_count=min_count)
        return ft.eta.std(0, unbiased=True), ft.sigma2_lss.std(0, unbiased=True)

    def arrays(self, min_count=100):
        """what variance_function.npz holds: the stack, ``fit(min_count)`` and, with more than one draw, ``std_over_draws(min_count)``"""
        ft = self.fit(min_count=min_count)
        over = dict(zip(("eta_std_over_draws", "sigma2_lss_std_over_draws"), self.std_over_draws(min_count))) if self.S > 1 else {}
        return self._export(z=self.z_centers, z_edges=self.z_edges, v_edges=self.v_edges, v_mean=self.v_mean, var_delta=self.var_delta,
                            var_err=self.var_err, mean_delta=self.mean_delta, counts=self.counts, n_segments=self.n_segments,
                            n_pixels=self.n_pixels, out_of_range=self.out_of_range(), seg_len=self.L, sums=self.buf, eta=ft.eta,
                            sigma2_lss=ft.sigma2_lss, cov=ft.cov, chi2=ft.chi2, ndof=ft.ndof, n_bins=ft.n_bins, **over)


class BootstrapStack(object):
    """The sightline bootstrap of a segment statistic (include/qfa_hip.h, qfa_bootstrap_f64): ``buf`` = (S, R, nz, 1 + W) float64
    [sum w | sum w x_0 .. x_{W-1}] per draw of the continuum, bootstrap replicate and z-bin, over the per-segment rows x of the
    statistic; w ~ Poisson(1) is drawn per (``seed``, global row of the spectrum, replicate), one weight for all the segments of a
    quasar.  Sums only, which is what data parallelism all-reduces.  ``estimate``: the map from sums (..., 1 + W) to the statistic
    (..., n) -- a stack class's ``bootstrap_estimate`` --, None = the weighted mean of the rows.  ``bins`` = (z0, dz, nz) as the
    kernels binned (None when the caller made the codes itself)."""

    def __init__(self, buf, seed=0, bins=None, estimate=None):
        if buf.dtype != torch.float64 or buf.dim() != 4 or min(buf.shape) < 1 or buf.shape[3] < 2 or not buf.is_contiguous():
            raise QFAHipError(f"BootstrapStack: buffer {tuple(buf.shape)} {buf.dtype}, expected contiguous float64 (S, R, nz, 1 + W)")
        if bins is not None:
            bins = _DrawStack._round_bins(*bins)
            if bins[2] != buf.shape[2]:
                raise QFAHipError(f"BootstrapStack: {bins[2]} z-bins, the buffer has {buf.shape[2]}")
        self.buf, self.seed, self.bins, self.estimate = buf, int(seed), bins, estimate

    @classmethod
    def zeros(cls, S, n_boot, nz, W, seed=0, bins=None, estimate=None, device="cpu"):
        return cls(torch.zeros((int(S), int(n_boot), int(nz), 1 + int(W)), dtype=torch.float64, device=device), seed, bins, estimate)

    S = property(lambda self: int(self.buf.shape[0]))
    R = property(lambda self: int(self.buf.shape[1]))
    nz = property(lambda self: int(self.buf.shape[2]))
    W = property(lambda self: int(self.buf.shape[3]) - 1)

    def _like(self, buf):
        return BootstrapStack(buf, self.seed, self.bins, self.estimate)

    def draws(self, s0, s1):
        """the stack of draws [s0, s1): a view of the same buffer"""
        return self._like(self.buf[s0:s1])

    def clone(self):
        return self._like(self.buf.clone())

    def all_reduce(self, group=None):
        """in-place sum over the process group (every rank calls it; an exhausted rank adds zeros)"""
        from .distributed import all_reduce_accum
        all_reduce_accum(self.buf.view(-1), group)
        return self

    @property
    def n(self):
        """(S, R, nz) the weighted number of segments of a replicate, sum w"""
        return self.buf[..., 0]

    @property
    def mean_rows(self):
        """(S, R, nz, W) the weighted mean of the rows, sum w x / sum w (NaN in an empty bin)"""
        return self.buf[..., 1:] / self.buf[..., 0:1]

    def estimates(self, fn=None):
        """(S, R, nz, n) the statistic of every replicate: ``fn`` (default ``estimate``, else ``mean_rows``) of the sums"""
        fn = fn if fn is not None else self.estimate
        return self.mean_rows if fn is None else fn(self.buf)

    def cov(self, across_z=False, fn=None):
        """the covariance over the R replicates of ``estimates(fn)``: (S, nz, n, n), or (S, nz n, nz n) with ``across_z`` -- the
        z-bins share quasars, which this carries.  NaN below two replicates"""
        e = self.estimates(fn)
        if across_z:
            e = e.reshape(self.S, self.R, 1, -1)
        d = e - e.mean(1, keepdim=True)
        c = torch.einsum("srza,srzb->szab", d, d) / (self.R - 1.0) if self.R > 1 else \
            torch.full((self.S, e.shape[2], e.shape[3], e.shape[3]), float("nan"), dtype=torch.float64, device=self.buf.device)
        return c[:, 0] if across_z else c

    def err(self, fn=None):
        """(S, nz, n) the bootstrap standard error of the statistic: the root of the diagonal of ``cov``"""
        return torch.sqrt(torch.diagonal(self.cov(fn=fn), dim1=2, dim2=3))

    def corr(self, across_z=False, fn=None):
        """the correlation matrix of ``cov``: cov_ab / sqrt(cov_aa cov_bb)"""
        c = self.cov(across_z, fn)
        d = torch.sqrt(torch.diagonal(c, dim1=-2, dim2=-1))
        return c / (d[..., :, None] * d[..., None, :])

    def arrays(self):
        """what <statistic>_bootstrap.npz holds"""
        z = {} if self.bins is None else {"z_edges": self.bins[0] + self.bins[1] * np.arange(self.nz + 1, dtype=np.float64)}
        named = dict(estimates=self.estimates(), cov=self.cov(), err=self.err(), n=self.n, n_boot=self.R, seed=self.seed, sums=self.buf, **z)
        return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in named.items()}
