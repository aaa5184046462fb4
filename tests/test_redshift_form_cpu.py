"""The one rule for the redshift form of a qfa_batch_t (QFA._redshift_form) through its two callers, `_batch_struct` (training,
prediction, forest) and `_p1d_inputs` (the segment statistics), on CPU tensors: which of zabs / zq1 / pix_ratio each fills, which
conversions it keeps alive, and what each refuses.  No pointer is dereferenced: `require_device_tensor` is replaced by one that
checks the dtype and returns the address."""
import ctypes as C

import pytest
import torch

from qfa_amd import _lib
from qfa_amd._lib import QFAHipError
from qfa_amd.model import QFA

B, NB, NPIX = 3, 5, 8


@pytest.fixture
def m(monkeypatch):
    def address(t, dtype, name):
        assert t.dtype == dtype and t.is_contiguous(), name
        return C.c_void_p(t.data_ptr())
    monkeypatch.setattr(_lib, "require_device_tensor", address)
    m = object.__new__(QFA)                                   # (no device to build a model on)
    m.Nb, m.Npix, m.device, m._tau_callable, m.use_factored_z, m.auto_factor_zabs = NB, NPIX, torch.device("cpu"), None, True, True
    m.auto_calls = []
    m._auto_zfac = lambda zabs: m.auto_calls.append(zabs)     # (returns None: nothing derived)
    return m


def both(m, zabs, zfac):
    """(qfa_batch_t, keep) of `_batch_struct` and of `_p1d_inputs` for the same redshift arguments"""
    x, mask = torch.ones(B, NPIX), torch.ones(B, NPIX, dtype=torch.bool)
    tr = torch.ones(B, 1, NB)
    a = m._batch_struct(x, x, zabs, mask, zfac, auto_factor=False)
    b = m._p1d_inputs("p1d", True, tr, tr, zabs, zfac, None, torch.ones(4), (2.0, 0.1, 4))[5:]
    return a, b


def kept(keep, address):
    return any(isinstance(t, torch.Tensor) and t.data_ptr() == address for t in keep)


def test_zabs_alone(m):
    z = torch.full((B, NB), 2.5)
    for bs, keep in both(m, z, None):
        assert bs.zabs == z.data_ptr() and bs.zq1 is None and bs.pix_ratio is None and kept(keep, bs.zabs)
    z64 = z.double()[:, ::1].t().contiguous().t()              # float64 and not contiguous: converted, and the copy kept alive
    for bs, keep in both(m, z64, None):
        assert bs.zabs not in (None, z64.data_ptr()) and kept(keep, bs.zabs) and bs.zq1 is None
    assert m.auto_calls == []


def test_the_pair_when_the_model_reads_it(m):
    z, zq1, ratio = torch.full((B, NB), 2.5), torch.full((B,), 3.5), torch.ones(NB)
    given = (z, (zq1, ratio))
    attached = torch.full((B, NB), 2.5)
    attached.zfac = (zq1, ratio)                              # (what a DeviceDataloader attaches)
    for zabs, zfac in (given, (attached, None), (None, (zq1, ratio))):
        (a, ka), (b, kb) = both(m, zabs, zfac)
        for bs, keep in ((a, ka), (b, kb)):
            assert bs.zq1 == zq1.data_ptr() and bs.pix_ratio == ratio.data_ptr() and kept(keep, bs.zq1) and kept(keep, bs.pix_ratio)
        # training and prediction pass zabs on next to the pair, the statistics pass one form only
        assert a.zabs == (None if zabs is None else zabs.data_ptr()) and b.zabs is None
    (a, ka), (b, kb) = both(m, None, (zq1.double(), ratio.double()))
    for bs, keep in ((a, ka), (b, kb)):
        assert bs.zq1 not in (None, zq1.data_ptr()) and kept(keep, bs.zq1) and kept(keep, bs.pix_ratio) and bs.zabs is None


def test_the_pair_when_the_model_does_not_read_it(m):
    z, zq1, ratio = torch.full((B, NB), 2.5), torch.full((B,), 3.5), torch.ones(NB)
    m.use_factored_z = False
    for bs, keep in both(m, z, (zq1, ratio)):
        assert bs.zabs == z.data_ptr() and bs.zq1 is None and bs.pix_ratio is None
    for call in (lambda: m._batch_struct(z, z, None, None, (zq1, ratio), allow_no_mask=True),
                 lambda: m._p1d_inputs("p1d", True, torch.ones(B, 1, NB), torch.ones(B, 1, NB), None, (zq1, ratio), None, torch.ones(4),
                                       (2.0, 0.1, 4))):
        with pytest.raises(QFAHipError, match="no usable zfac"):
            call()
    # a custom tau callable is evaluated on zabs: the pair is not usable either, and `_batch_struct` adds A_blue
    m.use_factored_z, m._tau_callable = True, lambda zz: 0.1 * zz
    (a, ka), (b, kb) = both(m, z, (zq1, ratio))
    assert a.zabs == b.zabs == z.data_ptr() and a.zq1 is None and b.zq1 is None and a.A_blue is not None and kept(ka, a.A_blue)


def test_what_is_refused(m):
    z, zq1, ratio = torch.full((B, NB), 2.5), torch.full((B,), 3.5), torch.ones(NB)
    x, mask, tr = torch.ones(B, NPIX), torch.ones(B, NPIX, dtype=torch.bool), torch.ones(B, 1, NB)
    p1d = lambda zabs, zfac: m._p1d_inputs("p1d", True, tr, tr, zabs, zfac, None, torch.ones(4), (2.0, 0.1, 4))
    for bad in ((zq1[:2], ratio), (zq1, ratio[:4])):
        with pytest.raises(QFAHipError, match="zfac shapes"):
            m._batch_struct(x, x, z, mask, bad)
        with pytest.raises(QFAHipError, match="zfac shapes"):
            p1d(z, bad)
    with pytest.raises(QFAHipError, match="zabs: shape"):
        p1d(z[:, :4], None)
    with pytest.raises(QFAHipError, match="zabs is None"):
        m._batch_struct(x, x, None, mask)
    with pytest.raises(QFAHipError, match="pass zabs, zfac"):
        p1d(None, None)


def test_factors_are_derived_for_training_only(m):
    """`_auto_zfac` may stand in for a plain zabs in `_batch_struct`; never where the caller turns it off (forest) or in the statistics"""
    z = torch.full((B, NB), 2.5)
    x, mask = torch.ones(B, NPIX), torch.ones(B, NPIX, dtype=torch.bool)
    both(m, z, None)
    assert m.auto_calls == []
    bs, _ = m._batch_struct(x, x, z, mask)
    assert m.auto_calls == [z] and bs.zabs == z.data_ptr() and bs.zq1 is None
