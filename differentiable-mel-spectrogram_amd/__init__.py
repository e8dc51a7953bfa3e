"""dmel_amd: MI355X-native differentiable log-Mel spectrogram layer (DMEL hot path).

Drop-in for the reference's ``models.MelSpectrogramLayer`` (models.py:14-56) and the
``log(s + 1e-10)`` line of its wrapping nets (models.py:73), executed by hand-written
HIP kernels for gfx950 behind a C-ABI shared library (``include/dmel.h``).

Heavy pieces (torch, the HIP library) are imported lazily so that ``dmel_amd.synth``
stays usable from tooling that has neither.
"""
from __future__ import annotations

import importlib

__all__ = ["MelSpectrogramLayer", "MultiWindowMelSpectrogram", "BandSplitMelSpectrogram", "DifferentiableMelSpectrogram", "SpectrogramLayer", "SlotInput", "dmel_log_mel", "GraphedStep", "LambdAdam", "PCEN", "BandNorm", "SpecMask", "Deltas", "StatsPool", "AttentivePool", "capi", "synth", "dist",
           "nets", "panns", "graph", "optim", "pcen", "bandnorm", "specmask", "deltas", "statspool", "attnpool"]

_LAZY = {
    "MelSpectrogramLayer": ("layer", "MelSpectrogramLayer"),
    "MultiWindowMelSpectrogram": ("layer", "MultiWindowMelSpectrogram"),
    "BandSplitMelSpectrogram": ("layer", "BandSplitMelSpectrogram"),
    "DifferentiableMelSpectrogram": ("layer", "DifferentiableMelSpectrogram"),
    "dmel_log_mel": ("layer", "dmel_log_mel"),
    "SpectrogramLayer": ("layer", "SpectrogramLayer"),
    "SlotInput": ("layer", "SlotInput"),
    "GraphedStep": ("graph", "GraphedStep"),
    "LambdAdam": ("optim", "LambdAdam"),
    "PCEN": ("pcen", "PCEN"),
    "BandNorm": ("bandnorm", "BandNorm"),
    "SpecMask": ("specmask", "SpecMask"),
    "Deltas": ("deltas", "Deltas"),
    "StatsPool": ("statspool", "StatsPool"),
    "AttentivePool": ("attnpool", "AttentivePool"),
}


def __getattr__(name):
    if name in _LAZY:
        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(f"dmel_amd.{mod}"), attr)
    if name in ("capi", "synth", "layer", "dist", "nets", "panns", "graph", "optim", "pcen", "bandnorm", "specmask", "deltas", "statspool", "attnpool"):
        return importlib.import_module(f"dmel_amd.{name}")
    raise AttributeError(name)
