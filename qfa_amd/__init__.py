"""qfa_amd -- MI355X-native implementation of the QFA hot path.

The public surface mirrors the reference package (``QFA.model.QFA``, ``QFA.optimizer.Adam``,
``QFA.optimizer.step_scheduler``, ``QFA.utils``); all arithmetic runs in hand-written HIP
kernels for gfx950 behind the C-ABI library ``libqfa_hip.so`` (see ``include/qfa_hip.h``).
Importing this package does not touch the GPU; the library is loaded on first use and
a missing library or device raises ``QFAHipError`` (there is no CPU fallback).
"""
__version__ = "0.1.0"

_LAZY = {
    "QFA": ("qfa_amd.model", "QFA"),
    "QFAModel": ("qfa_amd.model", "QFAModel"),
    "ForestStack": ("qfa_amd.model", "ForestStack"),
    "P1DStack": ("qfa_amd.model", "P1DStack"),
    "P1DBandStack": ("qfa_amd.model", "P1DBandStack"),
    "XiStack": ("qfa_amd.model", "XiStack"),
    "PDFStack": ("qfa_amd.model", "PDFStack"),
    "VarianceStack": ("qfa_amd.model", "VarianceStack"),
    "BootstrapStack": ("qfa_amd.model", "BootstrapStack"),
    "Adam": ("qfa_amd.optimizer", "Adam"),
    "step_scheduler": ("qfa_amd.optimizer", "step_scheduler"),
    # (the function has its module's name: once qfa_amd.preprocess is imported this attribute is the module, which is callable
    #  and calls the function -- qfa_amd/preprocess.py, _CallableModule)
    "preprocess": ("qfa_amd.preprocess", "preprocess"),
    "Preprocessed": ("qfa_amd.preprocess", "Preprocessed"),
    "AbsorberCatalog": ("qfa_amd.absorbers", "AbsorberCatalog"),
    "mask_absorbers": ("qfa_amd.absorbers", "mask_absorbers"),
    "bal_intervals": ("qfa_amd.absorbers", "bal_intervals"),
    "DLAScan": ("qfa_amd.dla", "DLAScan"),
    "ObservedStack": ("qfa_amd.calibration", "ObservedStack"),
    "BALScan": ("qfa_amd.bal", "BALScan"),
    "RedshiftScan": ("qfa_amd.redshift", "RedshiftScan"),
    "calibrate": ("qfa_amd.calibration", "calibrate"),
}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(mod), attr)
    raise AttributeError(name)
