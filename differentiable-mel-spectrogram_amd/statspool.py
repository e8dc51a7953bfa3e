"""StatsPool: length-aware mean / std / max pooling over time -- the stage that ends the length-aware chain behind the mel layers.

``layer(x, lengths)`` -> ``PCEN`` or log -> ``BandNorm`` -> ``SpecMask`` -> ``Deltas`` all take ``layer.frame_lengths(lengths)``; this stage
turns their ``(B, C, n_mels, T)`` image into a fixed-size ``(B, S C, n_mels)`` vector per clip -- the "statistics pooling" of x-vector style
heads -- from each row's own valid frames only.  The torch spelling goes wrong on a zero-padded batch: ``s.mean(-1)`` averages
``log(1e-10) = -23.03`` (or BandNorm's ``+0.0``) into a short clip, ``s.std(-1)`` measures mostly the step between signal and padding, and
``s.max(-1)`` returns a pad frame's ``+0.0`` for a band whose valid frames are all negative.  Here, with ``Tc = frame_lengths[b]``:

    mean   mu = (sum_{t < Tc} s[t]) / Tc
    std    sd = sqrt(sum_{t < Tc} (s[t] - mu)^2 / Tc + eps)          (the biased variance, as in BandNorm; the mean first)
    max    s[am], am by the order: a NaN beats a non-NaN, then the larger value, then the lower t

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=64, ..., optimized=True, log=True)
    norm, pool = dmel_amd.BandNorm(64, stats="clip").to("cuda"), dmel_amd.StatsPool()
    fl = layer.frame_lengths(lengths)
    v = pool(norm(layer(x, lengths), fl), fl)            # (B, 3, 64): torch.cat([mean, std, max], dim=1)

``csrc/dmel_statspool.hip`` through ``dmel_statspool_forward`` / ``dmel_statspool_backward`` of include/dmel.h, which is the specification:
one launch forward, one backward, fp64 inside, no atomics (the same bits every run, and a clip's bits do not depend on what it is batched
with).  The autograd function saves only what the selected statistics need: ``s`` and the fp64 ``(mu, sd)`` pairs when std is selected, the
int32 ``argmax`` when max is selected, and the lengths; under ``torch.no_grad()`` neither is written.  A ``frame_lengths[b]`` outside
``1 ... T`` makes that clip NaN, as in the stages in front.  No parameters, no buffers; the same in ``train()`` and ``eval()``; no host read,
capturable.

Out of scope here: bf16; per-frame weights (``dmel_amd.AttentivePool`` is that stage); the unbiased variance; pooling over bands; double backward; fusing the
stage into BandNorm or Deltas; a CPU fallback.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import capi

STATS = ("mean", "std", "max")         # the canonical order: the order of the output's groups; bit i of ``which`` selects STATS[i]


class _StatsPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, lengths, which, eps, keep):
        B, C, M, T = s.shape
        S = bin(which).count("1")
        rows = B * C * M
        y = torch.empty((B, S * C, M), dtype=s.dtype, device=s.device)
        stats = torch.empty((rows, 2), dtype=torch.float64, device=s.device) if keep and which & capi.STATSPOOL_STD else None
        argmax = torch.empty((rows,), dtype=torch.int32, device=s.device) if keep and which & capi.STATSPOOL_MAX else None
        with torch.cuda.device(s.device):
            capi.statspool_forward(s.data_ptr(), rows, C * M, T, None if lengths is None else lengths.data_ptr(), which, eps, y.data_ptr(),
                                   None if stats is None else stats.data_ptr(), None if argmax is None else argmax.data_ptr(),
                                   torch.cuda.current_stream(s.device).cuda_stream)
        ctx.save_for_backward(s if stats is not None else None, stats, argmax, lengths)
        ctx.which, ctx.in_shape = which, tuple(s.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        s, stats, argmax, lengths = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        if g.dtype != torch.float32:
            raise RuntimeError(f"StatsPool: the gradient of the output must be fp32, got {g.dtype}")
        g = g.contiguous()
        B, C, M, T = ctx.in_shape
        ds = torch.empty(ctx.in_shape, dtype=g.dtype, device=g.device)
        with torch.cuda.device(g.device):
            capi.statspool_backward(g.data_ptr(), None if s is None else s.data_ptr(), None if stats is None else stats.data_ptr(),
                                    None if argmax is None else argmax.data_ptr(), B * C * M, C * M, T,
                                    None if lengths is None else lengths.data_ptr(), ctx.which, ds.data_ptr(),
                                    torch.cuda.current_stream(g.device).cuda_stream)
        return (ds,) + (None,) * 4


class StatsPool(nn.Module):
    """``StatsPool(stats=("mean", "std", "max"), eps=1e-5)(s, frame_lengths=None)``: s of shape (B, n_mels, T) or (B, C, n_mels, T), fp32,
    on the GPU; ``(B, S C, n_mels)`` comes back, ``S = len(stats)`` (a 3-D input is ``C = 1``), in ``torch.cat([mean, std, max], dim=1)``
    order whatever order ``stats`` was given in.  ``frame_lengths``: (B,) int32 or int64 on s's device (``layer.frame_lengths(lengths)``),
    or None for ``T`` valid frames in every clip.  No parameters and no buffers."""

    def __init__(self, stats=("mean", "std", "max"), eps: float = 1e-5):
        super().__init__()
        if isinstance(stats, str):
            stats = (stats,)
        try:
            given = list(stats)
        except TypeError:
            raise ValueError(f"StatsPool: stats must be a non-empty subset of {STATS}, got {stats!r}") from None
        if not given or any(not isinstance(k, str) or k not in STATS for k in given):
            raise ValueError(f"StatsPool: stats must be a non-empty subset of {STATS}, got {stats!r}")
        if len(set(given)) != len(given):
            raise ValueError(f"StatsPool: stats names a statistic twice: {stats!r}")
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or not eps > 0:
            raise ValueError(f"StatsPool: eps must be a finite number > 0, got {eps!r}")
        self.stats = tuple(k for k in STATS if k in given)
        self.eps = float(eps)

    @property
    def which(self) -> int:
        """the bit mask of the C ABI: bit 0 mean, bit 1 std, bit 2 max"""
        return sum(1 << i for i, k in enumerate(STATS) if k in self.stats)

    @property
    def groups(self) -> int:
        """groups of the output: ``len(stats)``"""
        return len(self.stats)

    def extra_repr(self) -> str:
        return f"stats={self.stats}, eps={self.eps}"

    def _lengths(self, s, frame_lengths):
        """shape, dtype and device of ``frame_lengths``; returns them as the kernels read them (int32, contiguous).  Their values never
        leave the device."""
        if not torch.is_tensor(frame_lengths):
            raise TypeError(f"StatsPool: frame_lengths must be a 1-D integer tensor, got {type(frame_lengths).__name__}")
        if frame_lengths.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"StatsPool: frame_lengths must hold int32 or int64 values, got {frame_lengths.dtype}")
        if frame_lengths.dim() != 1 or frame_lengths.shape[0] != s.shape[0]:
            raise ValueError(f"StatsPool: frame_lengths must have shape ({s.shape[0]},), got {tuple(frame_lengths.shape)}")
        if frame_lengths.device != s.device:
            raise RuntimeError(f"StatsPool: frame_lengths is on {frame_lengths.device} but the input is on {s.device}")
        if frame_lengths.dtype != torch.int32:
            # int64 values clamped on the device before the narrowing: 2**32 + 5 must stay invalid (NaN), not wrap to 5
            frame_lengths = frame_lengths.clamp(0, s.shape[-1] + 1).to(torch.int32)
        return frame_lengths.contiguous()

    def forward(self, s: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        if not torch.is_tensor(s) or s.dim() not in (3, 4):
            raise ValueError(f"StatsPool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got {tuple(s.shape) if torch.is_tensor(s) else type(s).__name__}")
        if s.dtype != torch.float32:
            raise RuntimeError(f"StatsPool takes an fp32 mel image, got {s.dtype}")
        lengths = None if frame_lengths is None else self._lengths(s, frame_lengths)
        if s.dim() == 3:
            s = s.unsqueeze(1)
        B, C, M, T = s.shape
        if B * C * M == 0:
            return s.new_empty((B, self.groups * C, M))
        if T == 0:
            raise ValueError("StatsPool: the input has no frames (T = 0): there is nothing to pool")
        if not s.is_cuda:
            raise RuntimeError("dmel_amd runs on MI355X only: StatsPool's input must be a CUDA/HIP tensor (no CPU fallback)")
        keep = torch.is_grad_enabled() and s.requires_grad       # (asked here: inside an autograd function the grad mode is always off)
        return _StatsPoolFunction.apply(s.contiguous(), lengths, self.which, self.eps, keep)
