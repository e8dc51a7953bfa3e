"""Callers of the layer: the small nets the reference wraps around its mel layer.

Same constructor arguments, attribute / parameter names and ``(logits, s)`` return value as the
reference's ``MelLinearNet``, ``MelMlpNet`` and ``MelConvNet`` (models.py:58-136), so checkpoints
(``state_dict`` keys ``spectrogram_layer.lambd``, ``fc.*`` / ``fc1.*`` / ``fc2.*`` / ``conv1.*``) and the
per-parameter-group optimizer of main.py:36-48 carry over.  The heads are stock torch modules (MIOpen /
rocBLAS); only ``spectrogram_layer`` is ours, and ``energy_normalize=True`` uses its fused
``log(s + 1e-10)`` epilogue instead of a separate torch op (models.py:73, 97, 126).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .layer import MelSpectrogramLayer


class _MelFrontNet(nn.Module):
    """The front end the three nets share.  Two opt-in attributes, both ``None`` by default (nothing changes then): ``compression``
    (``dmel_amd.PCEN``) and, behind it and only while ``self.training``, ``augmentation`` (``dmel_amd.SpecMask``).  ``panns.Cnn6`` keeps its
    ``_IidAxisMask``: its tensor is transposed there and the reference masks the swapped axes."""

    def __init__(self, init_lambd, device, n_mels, sample_rate, n_points, hop_length, optimized, energy_normalize,
                 normalize_window):
        super().__init__()
        self.spectrogram_layer = MelSpectrogramLayer(
            init_lambd, n_mels=n_mels, n_points=n_points, sample_rate=sample_rate, hop_length=hop_length,
            device=device, optimized=optimized, normalize_window=normalize_window, log=bool(energy_normalize))
        self.device = device
        self.size = (n_mels, n_points // hop_length + 1)
        self.energy_normalize = energy_normalize

    def __setattr__(self, name, value):
        if name == "compression" and value is not None and getattr(self, "energy_normalize", False):
            raise ValueError("compression (dmel_amd.PCEN) takes linear mel power: build the net with energy_normalize=False")
        super().__setattr__(name, value)

    def _features(self, x):
        s = self.spectrogram_layer(x)             # already log-compressed when energy_normalize
        compression = getattr(self, "compression", None)      # opt-in: net.compression = dmel_amd.PCEN(n_mels)
        s = s if compression is None else compression(s)
        augmentation = getattr(self, "augmentation", None)    # opt-in: net.augmentation = dmel_amd.SpecMask(...); training only
        return s if augmentation is None or not self.training else augmentation(s)


class MelLinearNet(_MelFrontNet):
    """models.py:58-78: dropout(0.2) on the flattened spectrogram, one linear layer."""

    def __init__(self, n_classes, init_lambd, device, n_mels, sample_rate, n_points, hop_length=1, optimized=False,
                 energy_normalize=False, normalize_window=False):
        super().__init__(init_lambd, device, n_mels, sample_rate, n_points, hop_length, optimized, energy_normalize,
                         normalize_window)
        self.fc = nn.Linear(self.size[0] * self.size[1], n_classes)

    def forward(self, x):
        s = self._features(x)
        h = F.dropout(s.view(-1, self.size[0] * self.size[1]), p=0.2)     # always active, as in the reference
        return self.fc(h), s


class MelMlpNet(_MelFrontNet):
    """models.py:80-103: linear(32) - relu - dropout(0.2) - linear."""

    def __init__(self, n_classes, init_lambd, device, n_mels, sample_rate, n_points, hop_length=1, optimized=False,
                 energy_normalize=False, normalize_window=False):
        super().__init__(init_lambd, device, n_mels, sample_rate, n_points, hop_length, optimized, energy_normalize,
                         normalize_window)
        self.fc1 = nn.Linear(self.size[0] * self.size[1], 32)
        self.fc2 = nn.Linear(32, n_classes)

    def forward(self, x):
        s = self._features(x)
        h = F.dropout(F.relu(self.fc1(s.view(-1, self.size[0] * self.size[1]))), p=0.2)
        return self.fc2(h), s


class MelConvNet(_MelFrontNet):
    """models.py:105-136: conv5x5(32, 'same') - relu - linear(32) - relu - linear (BASELINE config 5's CNN)."""

    def __init__(self, n_classes, init_lambd, device, n_mels, sample_rate, n_points, hop_length=1, optimized=False,
                 energy_normalize=False, normalize_window=False):
        super().__init__(init_lambd, device, n_mels, sample_rate, n_points, hop_length, optimized, energy_normalize,
                         normalize_window)
        self.hidden_state = 32
        self.conv1 = nn.Conv2d(1, self.hidden_state, 5, padding="same")
        self.fc1 = nn.Linear(self.hidden_state * self.size[0] * self.size[1], self.hidden_state)
        self.fc2 = nn.Linear(self.hidden_state, n_classes)

    def forward(self, x):
        s = self._features(x)
        h = F.relu(self.conv1(s)).view(-1, self.hidden_state * self.size[0] * self.size[1])
        return self.fc2(F.relu(self.fc1(h))), s


class MelPoolNet(nn.Module):
    """The first net that takes a zero-padded batch: the mel layer over clips of per-clip lengths, ``dmel_amd.StatsPool`` over each clip's
    own valid frames, one linear layer on the ``S * n_mels`` pooled values -- no frame of the padding reaches the head, so a clip's logits
    do not depend on what it was batched with.  ``forward(x, lengths=None)`` returns ``(logits, s)``, ``s`` the image in front of the pool;
    ``lengths=None`` means every clip is full.  Two opt-in attributes, both ``None`` by default and both called as ``(s, fl)`` with
    ``fl = spectrogram_layer.frame_lengths(lengths)`` (``None`` for full clips): ``normalization`` (``dmel_amd.BandNorm``) and, behind it
    and only while ``self.training``, ``augmentation`` (``dmel_amd.SpecMask``).  The layer is the scalar ``MelSpectrogramLayer`` with
    ``optimized=True``, which takes ``lengths`` as it is; its parameter name ``spectrogram_layer.lambd`` keeps ``make_optimizer`` working."""

    def __init__(self, n_classes, init_lambd, device, n_mels, sample_rate, n_points, hop_length=1, energy_normalize=True,
                 normalize_window=False, stats=("mean", "std", "max")):
        super().__init__()
        from .statspool import StatsPool
        self.spectrogram_layer = MelSpectrogramLayer(
            init_lambd, n_mels=n_mels, n_points=n_points, sample_rate=sample_rate, hop_length=hop_length,
            device=device, optimized=True, normalize_window=normalize_window, log=bool(energy_normalize))
        self.pool = StatsPool(stats)
        self.fc = nn.Linear(self.pool.groups * n_mels, n_classes)
        self.device = device
        self.size = (n_mels, n_points // hop_length + 1)
        self.energy_normalize = energy_normalize
        self.normalization = None
        self.augmentation = None

    def forward(self, x, lengths=None):
        layer = self.spectrogram_layer
        fl = None if lengths is None else layer.frame_lengths(lengths)
        s = layer(x) if lengths is None else layer(x, lengths)
        if self.normalization is not None:
            s = self.normalization(s, fl)
        if self.augmentation is not None and self.training:
            s = self.augmentation(s, fl)
        return self.fc(self.pool(s, fl).flatten(1)), s


class MelAttnPoolNet(nn.Module):
    """``MelPoolNet`` with ``dmel_amd.AttentivePool`` in the pool's place and a per-frame scorer of stock torch modules in front of it:
    ``attention_fc1 = Conv1d(n_mels, attention_hidden, 1)``, tanh, ``attention_fc2 = Conv1d(attention_hidden, A, 1)`` on ``s[:, 0]`` (behind
    ``normalization`` and ``augmentation``); ``attention="shared"`` is one attention for the clip (``A = 1``), ``"band"`` one per mel band
    (``A = n_mels``).  The scorer's kernel size is 1 on purpose: a frame's logit depends on that frame alone, so pad frames reach the scorer
    and stop at the pool -- they cannot leak into valid frames through a context window.  ``forward(x, lengths=None)`` returns
    ``(logits, s)``; ``normalization`` and ``augmentation`` are opt-in exactly as on ``MelPoolNet``; the parameter name
    ``spectrogram_layer.lambd`` keeps ``make_optimizer`` working."""

    def __init__(self, n_classes, init_lambd, device, n_mels, sample_rate, n_points, hop_length=1, energy_normalize=True,
                 normalize_window=False, stats=("mean", "std"), attention="shared", attention_hidden=32):
        super().__init__()
        from .attnpool import AttentivePool
        if attention not in ("shared", "band"):
            raise ValueError(f"MelAttnPoolNet: attention must be 'shared' or 'band', got {attention!r}")
        self.spectrogram_layer = MelSpectrogramLayer(
            init_lambd, n_mels=n_mels, n_points=n_points, sample_rate=sample_rate, hop_length=hop_length,
            device=device, optimized=True, normalize_window=normalize_window, log=bool(energy_normalize))
        self.attention = attention
        self.attention_fc1 = nn.Conv1d(n_mels, attention_hidden, 1)
        self.attention_fc2 = nn.Conv1d(attention_hidden, 1 if attention == "shared" else n_mels, 1)
        self.pool = AttentivePool(stats)
        self.fc = nn.Linear(self.pool.groups * n_mels, n_classes)
        self.device = device
        self.size = (n_mels, n_points // hop_length + 1)
        self.energy_normalize = energy_normalize
        self.normalization = None
        self.augmentation = None

    def forward(self, x, lengths=None):
        layer = self.spectrogram_layer
        fl = None if lengths is None else layer.frame_lengths(lengths)
        s = layer(x) if lengths is None else layer(x, lengths)
        if self.normalization is not None:
            s = self.normalization(s, fl)
        if self.augmentation is not None and self.training:
            s = self.augmentation(s, fl)
        a = self.attention_fc2(torch.tanh(self.attention_fc1(s[:, 0])))
        return self.fc(self.pool(s, a, fl).flatten(1)), s


def make_optimizer(net: nn.Module, lr_model: float, lr_tf: float, name: str = "adam"):
    """The two learning-rate groups of main.py:36-53: ``lr_tf`` for ``spectrogram_layer.lambd``, ``lr_model`` for the rest."""
    groups = [{"params": [p], "lr": (lr_tf if n == "spectrogram_layer.lambd" else lr_model)} for n, p in net.named_parameters()]
    if name == "adam":
        return torch.optim.Adam(groups)
    if name == "sgd":
        return torch.optim.SGD(groups)
    raise ValueError(f"optimizer not found: {name}")
