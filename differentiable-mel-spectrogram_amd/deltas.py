"""Deltas: length-aware delta ("velocity") and delta-delta ("acceleration") channels behind the mel layers.

The classic two- or three-channel image of a mel front end -- log-mel, its deltas and their deltas -- for a zero-padded batch.
``torchaudio.functional.compute_deltas`` and a ``conv1d`` put the stencil's replicate padding at frame ``T - 1`` of the BATCH: under the log
a pad frame holds ``log(1e-10) = -23.03``, so the last ``n`` valid frames of every short clip get deltas of order ten, ``n`` more get wrong
delta-deltas, and the pad frames themselves get non-zero values where nothing happened.  Here the edge is the clip's own last valid frame:

    for t <  Tc:   d[t]  = ( sum_{j = 1 .. n}  j * ( x[min(t + j, Tc - 1)] - x[max(t - j, 0)] ) ) / denom,    Tc = frame_lengths[b]
                   dd[t] = the same formula applied to the stored fp32 row d[0 .. Tc - 1]
    for t >= Tc:   d[t] = dd[t] = +0.0

with ``n = (win_length - 1) / 2`` and ``denom = n (n + 1) (2 n + 1) / 3``; with ``Tc = T`` this is ``compute_deltas(win_length,
mode="replicate")`` applied once and twice.  A constant row, ``Tc = 1`` and a row of silent frames give ``+0.0`` bit for bit.

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=64, ..., per_clip_lengths=True)
    norm, deltas = dmel_amd.BandNorm(64, stats="clip").to("cuda"), dmel_amd.Deltas(win_length=5, order=2)
    fl = layer.frame_lengths(lengths)
    y = deltas(norm(layer(x, lengths), fl), fl)          # (B, 3, 64, T): torch.cat([s, d, dd], dim=1)

``csrc/dmel_deltas.hip`` through ``dmel_deltas_forward`` / ``dmel_deltas_backward`` of include/dmel.h, which is the specification: one launch
forward, one backward.  The output has ``G = include_static + order`` channel groups, ``(B, G C, M, T)``; group 0 is ``s`` moved as words on
every frame (pad frames keep what the stage in front wrote there), then ``d``, then ``dd``.  The stage is linear: the autograd function saves
the lengths only, ``ds = g_static + D^T (g_d + D^T g_dd)`` is gathered lane by lane (no atomics, the same bits every run).  A
``frame_lengths[b]`` outside ``1 ... T`` makes that clip NaN, as in ``BandNorm`` and ``SpecMask``.  No parameters, no buffers; the same in
``train()`` and ``eval()``; no host read, capturable.

Out of scope here: bf16; fusing the stage into BandNorm or SpecMask; double backward; ``mode`` other than replicate; ``order > 2``; a CPU
fallback; and a hook in ``nets`` or ``panns`` -- the small nets' ``Conv2d(1, ...)`` heads do not take two or three channels, so a net that
consumes this stage is built by the caller.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr

WIN_LENGTHS = (3, 5, 7, 9)


def _rows(s):
    B, C, M, T = s.shape
    return B * C * M, C * M, T


class _DeltasFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, lengths, win_length, order, include_static):
        B, C, M, T = s.shape
        G = int(include_static) + order
        y = torch.empty((B, G * C, M, T), dtype=s.dtype, device=s.device)
        rows, rows_per_clip, _ = _rows(s)
        _stage.launch(capi.deltas_forward, s, s.data_ptr(), rows, rows_per_clip, T, ptr(lengths), win_length, order, include_static, y.data_ptr())
        ctx.save_for_backward(lengths)
        ctx.win_length, ctx.order, ctx.include_static, ctx.in_shape = win_length, order, include_static, tuple(s.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        (lengths,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        g = _stage.cotangent("Deltas", g)
        B, C, M, T = ctx.in_shape
        ds = torch.empty(ctx.in_shape, dtype=g.dtype, device=g.device)
        _stage.launch(capi.deltas_backward, g, g.data_ptr(), B * C * M, C * M, T, ptr(lengths), ctx.win_length, ctx.order, ctx.include_static,
                      ds.data_ptr())
        return (ds,) + (None,) * 4


class Deltas(nn.Module):
    """``Deltas(win_length=5, order=2, include_static=True)(s, frame_lengths=None)``: s of shape (B, n_mels, T) or (B, C, n_mels, T), fp32, on
    the GPU; ``(B, G C, n_mels, T)`` comes back, ``G = include_static + order`` (a 3-D input is ``C = 1`` and comes back 4-D), in
    ``torch.cat([s, d, dd], dim=1)`` order.  ``frame_lengths``: (B,) int32 or int64 on s's device (``layer.frame_lengths(lengths)``), or
    None for ``T`` valid frames in every clip.  No parameters and no buffers.  The small nets' ``Conv2d(1, ...)`` heads do not take the
    extra channels: a hook in ``nets`` is out of scope."""

    def __init__(self, win_length: int = 5, order: int = 2, include_static: bool = True):
        super().__init__()
        if isinstance(win_length, bool) or int(win_length) != win_length or int(win_length) not in WIN_LENGTHS:
            raise ValueError(f"Deltas: win_length must be one of 3, 5, 7, 9, got {win_length}")
        if isinstance(order, bool) or int(order) != order or int(order) not in (1, 2):
            raise ValueError(f"Deltas: order must be 1 or 2, got {order}")
        if not isinstance(include_static, bool):
            raise ValueError(f"Deltas: include_static must be True or False, got {include_static}")
        self.win_length, self.order, self.include_static = int(win_length), int(order), include_static

    @property
    def groups(self) -> int:
        """channel groups of the output: ``include_static + order``"""
        return int(self.include_static) + self.order

    def extra_repr(self) -> str:
        return f"win_length={self.win_length}, order={self.order}, include_static={self.include_static}"

    def forward(self, s: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        s = _stage.mel_image("Deltas", s)
        lengths = _stage.frame_lengths_for_kernels("Deltas", s, frame_lengths)
        B, C, M, T = s.shape
        if s.numel() == 0:
            return s.new_empty((B, self.groups * C, M, T))
        _stage.require_gpu("Deltas", s)
        return _DeltasFunction.apply(s.contiguous(), lengths, self.win_length, self.order, self.include_static)
