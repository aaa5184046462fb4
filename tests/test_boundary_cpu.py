"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares; the Python surface mirrors the reference's names; nothing computes without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "qfa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(qfa_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from qfa_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    h = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 13
    for s in syms:
        assert hasattr(h, s), s
    assert sorted(_lib.EXPORTS) == syms
    assert _lib.lib().qfa_abi_version() == _lib.ABI_VERSION == 4


def test_host_only_entry_points():
    """qfa_tau_model / qfa_workspace_bytes / qfa_accum_floats are pure host functions."""
    import ctypes as C
    from oracle import qfa_oracle as O
    from qfa_amd import _lib
    for which in ("becker", "fg", "kamble", "mock"):
        for series in (1, 2, 30):
            t = _lib.tau_model(which, series)
            amp, scale, expo, off = O.TAU_MODELS[which]
            c = O.LYMAN_COEFF[series - 1]
            assert abs(t.amp - amp * c) <= 1e-7 * abs(amp * c) + 1e-12
            assert abs(t.offset - off * c) <= 1e-7 * abs(off * c) + 1e-12
            assert abs(t.scale - scale) < 1e-7 and abs(t.expo - expo) < 1e-6
    with pytest.raises(NotImplementedError):
        _lib.tau_model("nope")
    h = _lib.lib()
    assert h.qfa_tau_model(0, 31, C.byref(_lib.TauModel())) == -4
    assert h.qfa_accum_floats(1913, 720, 8) == 1913 * 8 + 3 * 1913 + 720 + 8
    assert h.qfa_workspace_bytes(128, 1913, 8) > 0
    assert h.qfa_workspace_bytes(0, 1913, 8) == 0
    assert h.qfa_workspace_bytes(4, 100, 33) == 0 and h.qfa_workspace_bytes(4, 100, 32) > 0
    # argument validation happens before any device work
    assert h.qfa_nll_grad_f32(None, None, None, 1, 1, 1, 1, None, None, None, 0, None) == -1
    assert h.qfa_adam_clip_f32(None, None, None, None, None, 4, 0, 0, 0, 0, 0, 0, 0, 0, None) == -1


def test_step_entry_points_agree_on_invalid_arguments():
    """The four qfa_nll_grad* and the three qfa_predict* entry points are one function behind different argument lists: the same
    invalid arguments give the same QFA_E_* code from each, and the order of the checks (pointers, shape, workspace, flags) decides
    which.  Every call here returns before any launch (the pointers are never read), so no device is needed."""
    import ctypes as C
    from qfa_amd import _lib
    h = _lib.lib()
    E_NULL, E_SIZE, E_WORKSPACE, E_FLAGS = -1, -2, -3, -5
    B, npix, nb, nh = 5, 40, 13, 8
    fake = 0x1000                                     # stands for a device pointer
    wsb = h.qfa_workspace_bytes(B, npix, nh)
    assert wsb > 0
    tau = _lib.tau_model("becker", 1)
    batch = _lib.Batch(delta=fake, error=fake, zabs=fake, mask=fake)

    def codes(params, nb_, wsb_):
        p, b, t = C.byref(params), C.byref(batch), C.byref(tau)
        shape = (B, npix, nb_, nh)
        grad = (p, b, t) + shape + (fake, fake, fake, wsb_)
        pred = (p, fake, b, t) + shape + (fake,) * 6 + (wsb_,)
        return ([h.qfa_nll_grad_f32(*grad, None), h.qfa_nll_grad_events_f32(*grad, None, None),
                 h.qfa_nll_grad_det_f32(*grad, None, 0, None, None), h.qfa_nll_grad_ex_f32(*grad, None, 0, 0, None, None)],
                [h.qfa_predict_f32(*pred, None), h.qfa_predict_events_f32(*pred, None, None), h.qfa_predict_ex_f32(*pred, 0, None, None)])

    good = _lib.Params(*([fake] * 6))
    no_psi = _lib.Params(F=fake, omega=fake, tau0=fake, c0=fake, beta=fake)
    for what, args, want in (("NULL parameter pointer", (no_psi, nb, wsb), E_NULL),
                             ("Nb > Npix", (good, npix + 1, wsb), E_SIZE),
                             ("workspace one byte short", (good, nb, wsb - 1), E_WORKSPACE),
                             # the first failing check decides
                             ("NULL parameter pointer, Nb > Npix, short workspace", (no_psi, npix + 1, wsb - 1), E_NULL),
                             ("Nb > Npix, short workspace", (good, npix + 1, wsb - 1), E_SIZE)):
        grad, pred = codes(*args)
        assert grad == [want] * 4, (what, grad)
        assert pred == [want] * 3, (what, pred)
    # QFA_F_S3_FAST names a form that exists at N_h = 17..32 only: the step's plan refuses it in front of the first launch
    ex = lambda flags, wsb_: h.qfa_nll_grad_ex_f32(C.byref(good), C.byref(batch), C.byref(tau), B, npix, nb, nh, fake, fake, fake,
                                                   wsb_, None, 0, flags, None, None)
    assert ex(_lib.F_S3_FAST, wsb) == E_FLAGS
    assert ex(_lib.F_S3_FAST, wsb - 1) == E_WORKSPACE          # (the workspace is checked first)


def test_python_surface_matches_reference_names():
    from qfa_amd import model, optimizer, utils
    sig = inspect.signature(model.QFA.__init__)
    assert list(sig.parameters)[1:] == ["Nb", "Nr", "Nh", "device", "tau", "model_params"]
    for name in ("forward", "loglikelihood_and_gradient_for_single_spectra", "prediction_for_single_spectra",
                 "train", "clip", "smooth", "save_to_npz", "load_from_npz", "random_init_func", "parameters",
                 "fit", "predict"):
        assert hasattr(model.QFA, name), name
    assert list(inspect.signature(model.QFA.forward).parameters)[1:5] == ["delta", "error", "zabs", "mask"]
    # the reference's parameters first and in its order; extensions (hipGraph replay) only behind them
    assert list(inspect.signature(model.QFA.train).parameters)[1:9] == [
        "optimizer", "dataloader", "n_epochs", "output_dir", "save_interval", "smooth_interval", "quiet", "logger"]
    assert inspect.signature(model.QFA.train).parameters["use_graph"].default is False
    assert model.QFAModel is model.QFA
    a = inspect.signature(optimizer.Adam.__init__)
    assert list(a.parameters)[1:] == ["params", "device", "scheduler", "learning_rate", "b1", "b2", "eps",
                                      "weight_decay"]
    assert a.parameters["learning_rate"].default == 1e-2 and a.parameters["weight_decay"].default == 1e-3
    for name in ("update", "step", "reset", "scheduled_lr"):
        assert hasattr(optimizer.Adam, name)
    assert optimizer.step_scheduler(0.9, 2)(3, 1.0) == pytest.approx(0.81)
    for name in ("MatrixInverse", "MatrixLogDet", "tauHI", "omega_func", "tau"):
        assert hasattr(utils, name)
    assert model.log2pi == 1.8378770664093453


def test_no_cpu_fallback():
    import torch
    from qfa_amd import QFA, utils
    from qfa_amd._lib import QFAHipError
    with pytest.raises(QFAHipError):
        QFA(4, 4, 2, torch.device("cpu"))
    with pytest.raises(QFAHipError):
        utils.tau(torch.zeros(4))
    with pytest.raises(QFAHipError):
        utils.MatrixLogDet(torch.zeros(4, 2), torch.ones(4))


def test_product_package_never_imports_oracle():
    for root, _, files in os.walk(os.path.join(REPO, "qfa_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), f


def test_synthetic_generator_is_deterministic_and_masks_hold_sentinels():
    from qfa_amd import synthetic
    wav, nb, nr = synthetic.wavelength_grid()
    assert (len(wav), nb, nr) == (1913, 720, 1193)
    for n, enb in ((2000, 753), (4000, 1506), (8000, 3011)):
        assert synthetic.wavelength_grid(n)[1] == enb
    p, mu = synthetic.mock_parameters(400, synthetic.wavelength_grid(400)[1], 8, seed=1)
    w, b_, _ = synthetic.wavelength_grid(400)
    a = synthetic.make_batch_numpy(p, mu, w, b_, 5, seed=9)
    b = synthetic.make_batch_numpy(p, mu, w, b_, 5, seed=9)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert (a["flux"][~a["mask"]] == -999).all() and (a["error"][~a["mask"]] == -999).all()
