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

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr

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
        _stage.launch(capi.statspool_forward, s, s.data_ptr(), rows, C * M, T, ptr(lengths), which, eps, y.data_ptr(), ptr(stats), ptr(argmax))
        ctx.save_for_backward(s if stats is not None else None, stats, argmax, lengths)
        ctx.which, ctx.in_shape = which, tuple(s.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        s, stats, argmax, lengths = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        g = _stage.cotangent("StatsPool", g)
        B, C, M, T = ctx.in_shape
        ds = torch.empty(ctx.in_shape, dtype=g.dtype, device=g.device)
        _stage.launch(capi.statspool_backward, g, g.data_ptr(), ptr(s), ptr(stats), ptr(argmax), B * C * M, C * M, T, ptr(lengths), ctx.which,
                      ds.data_ptr())
        return (ds,) + (None,) * 4


class StatsPool(nn.Module):
    """``StatsPool(stats=("mean", "std", "max"), eps=1e-5)(s, frame_lengths=None)``: s of shape (B, n_mels, T) or (B, C, n_mels, T), fp32,
    on the GPU; ``(B, S C, n_mels)`` comes back, ``S = len(stats)`` (a 3-D input is ``C = 1``), in ``torch.cat([mean, std, max], dim=1)``
    order whatever order ``stats`` was given in.  ``frame_lengths``: (B,) int32 or int64 on s's device (``layer.frame_lengths(lengths)``),
    or None for ``T`` valid frames in every clip.  No parameters and no buffers."""

    def __init__(self, stats=("mean", "std", "max"), eps: float = 1e-5):
        super().__init__()
        self.stats, self.eps = _stage.pool_stats("StatsPool", STATS, stats, eps)

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

    def forward(self, s: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        s = _stage.mel_image("StatsPool", s)
        lengths = _stage.frame_lengths_for_kernels("StatsPool", s, frame_lengths)
        B, C, M, T = s.shape
        if B * C * M == 0:
            return s.new_empty((B, self.groups * C, M))
        if T == 0:
            raise ValueError("StatsPool: the input has no frames (T = 0): there is nothing to pool")
        _stage.require_gpu("StatsPool", s)
        keep = torch.is_grad_enabled() and s.requires_grad       # (asked here: inside an autograd function the grad mode is always off)
        return _StatsPoolFunction.apply(s.contiguous(), lengths, self.which, self.eps, keep)
