"""SpecMask: length-aware SpecAugment stripes behind the mel layers.

What the reference applies behind ``bn1`` in training (``Cnn6.mask_time`` / ``mask_freq``, panns.py:141-142, 174-176:
``TimeMasking(64, iid_masks=True)``, ``FrequencyMasking(8, iid_masks=True)``) as a stage of its own behind any layer, behind ``PCEN`` or
behind ``BandNorm``, for a zero-padded batch: every (clip, channel) image draws its own ``time_stripes`` time stripes over the clip's VALID
frames ``t < frame_lengths[b]`` and ``freq_stripes`` frequency stripes over its bands,

    y = fill_value  on a valid frame under a time stripe or in a band under a frequency stripe;   y = s bit for bit elsewhere

and every pad frame passes through bit for bit (what the stage in front wrote there stays).  A stripe on an axis of ``size`` positions has
``width`` uniform in ``0 ... min(param, size) - 1`` and a start uniform over the positions where it fits (torchaudio's
``mask_along_axis_iid``); the time cap is ``min(time_mask_param, Tc * max_time_fraction)`` (SpecAugment's adaptive cap).

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=64, ..., per_clip_lengths=True)
    norm, mask = dmel_amd.BandNorm(64, stats="batch").to("cuda"), dmel_amd.SpecMask(64, 8).to("cuda")
    fl = layer.frame_lengths(lengths)
    y = mask(norm(layer(x, lengths), fl), fl)

``csrc/dmel_specmask.hip`` through ``dmel_specmask_draw`` / ``dmel_specmask_apply`` of include/dmel.h, which is the specification: the
random words are Philox4x32-10 keyed by the first word of the buffer ``rng_state = (seed, calls)`` and counted by the second, which the
draw advances by one per training forward ON THE DEVICE -- no host read, so a captured step draws fresh stripes on every replay, and
because the buffer is in the state dict a resumed run draws what the uninterrupted run would have drawn.  Everything is integer
arithmetic: ``tests/specmask_cases.py`` restates every stripe and every output bit in numpy.  fp32 or bf16, moved and never converted.  The
gradient is the same selection of the cotangent with fill ``+0.0``; the autograd function saves the (images, stripes, 2) int32 table and
the lengths, no mask tensor exists.  A ``frame_lengths[b]`` outside ``1 ... T`` makes that clip NaN, as in ``BandNorm``.  In ``eval()``, and
with both stripe counts 0, the module returns its argument and launches nothing.  ``nets._MelFrontNet.augmentation`` is the opt-in hook
of the small nets; ``panns.Cnn6`` keeps its ``_IidAxisMask`` (its tensor is transposed there and the reference masks the swapped axes).

Out of scope here: fusing the stage into BandNorm's apply; mixup; masks shared across a batch (``iid_masks=False``); different seeds per
rank (the caller seeds with the rank: ``SpecMask(..., seed=base + rank)``); ``GraphedStep`` knowledge of the buffer beyond its being an
ordinary device buffer; a CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr

MAX_STRIPES = 8
DTYPES = (torch.float32, torch.bfloat16)


def _geometry(s):
    n_mels, T = s.shape[-2], s.shape[-1]
    channels = s.shape[1] if s.dim() == 4 else 1
    return s.shape[0] * channels, channels, n_mels, T


class _SpecMaskFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, stripes, lengths, n_time, n_freq, fill):
        y = torch.empty_like(s)
        _SpecMaskFunction._apply(s, stripes, lengths, n_time, n_freq, fill, y)
        ctx.save_for_backward(stripes, lengths)
        ctx.n_time, ctx.n_freq = n_time, n_freq
        return y

    @staticmethod
    def _apply(s, stripes, lengths, n_time, n_freq, fill, y):
        images, channels, n_mels, T = _geometry(s)
        _stage.launch(capi.specmask_apply, s, s.data_ptr(), images * n_mels, n_mels, channels * n_mels, T, ptr(lengths), stripes.data_ptr(), n_time,
                      n_freq, s.dtype == torch.bfloat16, fill, y.data_ptr())

    @staticmethod
    def backward(ctx, g):
        stripes, lengths = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        g = _stage.cotangent("SpecMask", g, DTYPES, "fp32 or bf16")
        ds = torch.empty_like(g)
        _SpecMaskFunction._apply(g, stripes, lengths, ctx.n_time, ctx.n_freq, 0.0, ds)
        return (ds,) + (None,) * 5


class SpecMask(nn.Module):
    """``SpecMask(time_mask_param=64, freq_mask_param=8, time_stripes=1, freq_stripes=1)(s, frame_lengths=None)``: s of shape
    (B, n_mels, T) or (B, C, n_mels, T), fp32 or bf16, on the GPU; the same shape and dtype come back.  ``frame_lengths``: (B,) int32 or int64
    on s's device (``layer.frame_lengths(lengths)``), or None for ``T`` valid frames in every clip.  One buffer: ``rng_state``, int64
    ``(seed, calls)``.  ``max_time_fraction`` f caps a time stripe at ``Tc * round(1000 f) // 1000`` frames."""

    def __init__(self, time_mask_param: int = 64, freq_mask_param: int = 8, *, time_stripes: int = 1, freq_stripes: int = 1,
                 max_time_fraction: float = 1.0, fill_value: float = 0.0, seed: int | None = None):
        super().__init__()
        for name, v in (("time_mask_param", time_mask_param), ("freq_mask_param", freq_mask_param), ("time_stripes", time_stripes),
                        ("freq_stripes", freq_stripes)):
            if int(v) != v or int(v) < 0 or int(v) > 0x7FFFFFFF:
                raise ValueError(f"SpecMask: {name} must be an integer >= 0, got {v}")
        if int(time_stripes) + int(freq_stripes) > MAX_STRIPES:
            raise ValueError(f"SpecMask: time_stripes + freq_stripes must be <= {MAX_STRIPES}, got {time_stripes} + {freq_stripes}")
        if not (0.0 <= float(max_time_fraction) <= 1.0):
            raise ValueError(f"SpecMask: max_time_fraction must lie in 0 ... 1, got {max_time_fraction}")
        self.time_mask_param, self.freq_mask_param = int(time_mask_param), int(freq_mask_param)
        self.time_stripes, self.freq_stripes = int(time_stripes), int(freq_stripes)
        self.max_time_fraction, self.time_permille = float(max_time_fraction), int(round(1000.0 * float(max_time_fraction)))
        self.fill_value = float(fill_value)
        self.register_buffer("rng_state", self._state(torch.initial_seed() if seed is None else seed, 0))
        self._last = None

    @staticmethod
    def _state(seed, calls):
        """(seed, calls) as the int64 pair the kernel reads as two unsigned 64-bit words"""
        words = []
        for name, v in (("seed", seed), ("calls", calls)):
            if int(v) != v or not (-(1 << 63) <= int(v) < (1 << 64)):
                raise ValueError(f"SpecMask: {name} must be an integer of 64 bits, got {v}")
            v = int(v) & 0xFFFFFFFFFFFFFFFF
            words.append(v - (1 << 64) if v >= (1 << 63) else v)
        return torch.tensor(words, dtype=torch.int64)

    def manual_seed(self, seed: int, calls: int = 0) -> "SpecMask":
        """rewrites ``rng_state`` in place: the next training forward draws call number ``calls`` of ``seed``"""
        self.rng_state.copy_(self._state(seed, calls))
        return self

    def last_stripes(self) -> torch.Tensor | None:
        """the (images, time_stripes + freq_stripes, 2) int32 table of ``[lo, hi)`` pairs of the last training forward, time stripes first
        (the device tensor the backward reads: nothing is copied or read here); None before the first"""
        return self._last

    def extra_repr(self) -> str:
        return (f"time_mask_param={self.time_mask_param}, freq_mask_param={self.freq_mask_param}, time_stripes={self.time_stripes}, "
                f"freq_stripes={self.freq_stripes}, max_time_fraction={self.max_time_fraction}, fill_value={self.fill_value}")

    def forward(self, s: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        # (the checks only: this stage works on the tensor as it is given, 3-D or 4-D, and returns that shape)
        _stage.mel_image("SpecMask", s, "an fp32 or bf16 mel image", DTYPES)
        n_time, n_freq = self.time_stripes, self.freq_stripes
        if not self.training or n_time + n_freq == 0:
            return s
        lengths = _stage.frame_lengths_for_kernels("SpecMask", s, frame_lengths)
        _stage.require_gpu("SpecMask", s)
        if self.rng_state.device != s.device:
            raise RuntimeError(f"SpecMask.rng_state is on {self.rng_state.device} but the input is on {s.device}; call mask.to(x.device)")
        if self.rng_state.dtype != torch.int64 or tuple(self.rng_state.shape) != (2,):
            raise RuntimeError(f"SpecMask.rng_state must stay two int64 values, got {self.rng_state.dtype} {tuple(self.rng_state.shape)}")
        if s.numel() == 0:
            return s
        s = s.contiguous()
        images, channels, n_mels, T = _geometry(s)
        stripes = torch.empty((images, n_time + n_freq, 2), dtype=torch.int32, device=s.device)
        _stage.launch(capi.specmask_draw, s, images, channels, n_mels, T, ptr(lengths), self.time_mask_param, self.time_permille, n_time,
                      self.freq_mask_param, n_freq, self.rng_state.data_ptr(), True, stripes.data_ptr())
        self._last = stripes
        return _SpecMaskFunction.apply(s, stripes, lengths, n_time, n_freq, self.fill_value)
