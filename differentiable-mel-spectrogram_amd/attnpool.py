"""AttentivePool: length-aware attentive statistics pooling over time -- StatsPool with per-frame weights of the caller's scorer.

``StatsPool`` ends the length-aware chain with uniform weights over a clip's valid frames; this stage is the x-vector / ECAPA "attentive
statistics pooling": a scorer gives every frame a logit, a softmax over time turns logits into weights, and the clip vector is the weighted
mean and the weighted standard deviation.  The torch spelling ``softmax(a, -1)`` goes wrong on a zero-padded batch: every pad frame takes a
share of the weight, so a short clip's statistics depend on how much padding its neighbours forced on it.  Here, with
``Tc = frame_lengths[b]`` and over ``t < Tc`` only:

    w[t] = exp(a[t] - max a) / Z        mu = sum w[t] s[t]        sd = sqrt(sum w[t] (s[t] - mu)^2 + eps)

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=64, ..., optimized=True, log=True)
    pool = dmel_amd.AttentivePool()
    fl = layer.frame_lengths(lengths)
    s = layer(x, lengths)                                # (B, 1, 64, T)
    v = pool(s, scorer(s[:, 0]), fl)                     # logits (B, A, T) -> (B, 2, 64): torch.cat([mean, std], dim=1)

The logits are ``(B, T)`` (one attention for the clip), ``(B, A, T)`` with ``A`` dividing ``C n_mels`` (row ``r`` of a clip reads logit row
``r / (C n_mels / A)``: ``A = C`` one per channel, ``A = C n_mels`` one per band, ECAPA's channel-dependent form) or ``(B, C, n_mels, T)``.
``csrc/dmel_attnpool.hip`` through ``dmel_attnpool_forward`` / ``dmel_attnpool_backward`` of include/dmel.h, which is the specification: one
launch forward, one backward, fp64 inside, no atomics (the same bits every run, and a clip's bits do not depend on what it is batched with).
Gradients reach ``s`` and the logits.  The autograd function asks the forward for the fp64 ``(mu, var)`` and ``(m, Z)`` pairs, and saves them
with ``s`` and the logits, only when grad mode is on and an input needs a gradient.  A ``frame_lengths[b]`` outside ``1 ... T`` makes that
clip NaN, as in the stages in front.  No parameters, no buffers -- the scorer is the caller's --; the same in ``train()`` and ``eval()``; no
host read, capturable.

Out of scope here: bf16; a maximum statistic; multi-head outputs (call per head); a temperature; double backward; fusing the scorer or
BandNorm into the stage; a CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr

STATS = ("mean", "std")                # the canonical order: the order of the output's groups; bit i of ``which`` selects STATS[i]


class _AttentivePoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, a, lengths, which, eps, keep):
        B, C, M, T = s.shape
        A = a.shape[1]
        S = bin(which).count("1")
        rows = B * C * M
        y = torch.empty((B, S * C, M), dtype=s.dtype, device=s.device)
        stats = torch.empty((rows, 2), dtype=torch.float64, device=s.device) if keep else None
        norm = torch.empty((B * A, 2), dtype=torch.float64, device=s.device) if keep else None
        _stage.launch(capi.attnpool_forward, s, s.data_ptr(), a.data_ptr(), rows, C * M, A, T, ptr(lengths), which, eps, y.data_ptr(), ptr(stats),
                      ptr(norm))
        if keep:
            ctx.save_for_backward(s, a, stats, norm, lengths)
        ctx.which, ctx.eps = which, eps
        return y

    @staticmethod
    def backward(ctx, g):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 6
        s, a, stats, norm, lengths = ctx.saved_tensors
        g = _stage.cotangent("AttentivePool", g)
        B, C, M, T = s.shape
        ds, da = torch.empty_like(s), torch.empty_like(a)
        _stage.launch(capi.attnpool_backward, g, g.data_ptr(), s.data_ptr(), a.data_ptr(), stats.data_ptr(), norm.data_ptr(), B * C * M, C * M,
                      a.shape[1], T, ptr(lengths), ctx.which, ctx.eps, ds.data_ptr(), da.data_ptr())
        return (ds if ctx.needs_input_grad[0] else None, da if ctx.needs_input_grad[1] else None) + (None,) * 4


class AttentivePool(nn.Module):
    """``AttentivePool(stats=("mean", "std"), eps=1e-5)(s, logits, frame_lengths=None)``: s of shape (B, n_mels, T) or (B, C, n_mels, T),
    fp32, on the GPU; logits fp32 on s's device, of shape (B, T), (B, A, T) with A dividing C n_mels, or (B, C, n_mels, T);
    ``(B, S C, n_mels)`` comes back, ``S = len(stats)`` (a 3-D input is ``C = 1``), in ``torch.cat([mean, std], dim=1)`` order whatever
    order ``stats`` was given in.  ``frame_lengths``: (B,) int32 or int64 on s's device (``layer.frame_lengths(lengths)``), or None for
    ``T`` valid frames in every clip.  No parameters and no buffers."""

    def __init__(self, stats=("mean", "std"), eps: float = 1e-5):
        super().__init__()
        self.stats, self.eps = _stage.pool_stats("AttentivePool", STATS, stats, eps)

    @property
    def which(self) -> int:
        """the bit mask of the C ABI: bit 0 mean, bit 1 std"""
        return sum(1 << i for i, k in enumerate(STATS) if k in self.stats)

    @property
    def groups(self) -> int:
        """groups of the output: ``len(stats)``"""
        return len(self.stats)

    def extra_repr(self) -> str:
        return f"stats={self.stats}, eps={self.eps}"

    @staticmethod
    def _logits(s, logits):
        """the logits as (B, A, T) for s (B, C, M, T)"""
        B, C, M, T = s.shape
        want = f"({B}, {T}), ({B}, A, {T}) with A dividing C n_mels = {C * M}, or ({B}, {C}, {M}, {T})"
        if not torch.is_tensor(logits):
            raise ValueError(f"AttentivePool: logits must be a tensor of shape {want}, got {type(logits).__name__}")
        if logits.dtype != torch.float32:
            raise RuntimeError(f"AttentivePool takes fp32 logits, got {logits.dtype}")
        shape = tuple(logits.shape)
        if shape == (B, T):
            a = logits.unsqueeze(1)
        elif shape == (B, C, M, T):
            a = logits.reshape(B, C * M, T)
        elif logits.dim() == 3 and shape[0] == B and shape[2] == T and (shape[1] >= 1 and (C * M) % shape[1] == 0 or C * M == 0):
            a = logits
        else:
            raise ValueError(f"AttentivePool: logits must have shape {want}, got {shape}")
        if logits.device != s.device:
            raise RuntimeError(f"AttentivePool: logits are on {logits.device} but the input is on {s.device}")
        return a

    def forward(self, s: torch.Tensor, logits: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        s = _stage.mel_image("AttentivePool", s)
        lengths = _stage.frame_lengths_for_kernels("AttentivePool", s, frame_lengths)
        a = self._logits(s, logits)
        B, C, M, T = s.shape
        if B * C * M == 0:
            return s.new_empty((B, self.groups * C, M))
        if T == 0:
            raise ValueError("AttentivePool: the input has no frames (T = 0): there is nothing to pool")
        _stage.require_gpu("AttentivePool", s)
        keep = torch.is_grad_enabled() and (s.requires_grad or a.requires_grad)      # (asked here: inside an autograd function the grad mode is always off)
        return _AttentivePoolFunction.apply(s.contiguous(), a.contiguous(), lengths, self.which, self.eps, keep)
