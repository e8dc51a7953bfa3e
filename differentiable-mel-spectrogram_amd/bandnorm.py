"""BandNorm: length-aware per-band standardisation behind the mel layers.

The first thing every consumer does to a mel image is a per-band standardisation: ``Cnn6.bn1`` (batch normalisation over the mel bins,
panns.py:169-172) or per-clip mean / variance normalisation (CMVN).  On a zero-padded batch (``layer(x, lengths)``) torch's versions take
their statistics over all ``T`` frames, pad included -- ``log(1e-10) = -23.03`` with the log, ``0`` without --, so the result depends on how
much padding a batch happened to carry.  ``BandNorm`` takes them over the valid frames ``t < frame_lengths[b]`` only:

    y = (s - mu) / sqrt(var + eps) * weight[band] + bias[band]     on valid frames (var: the biased variance);  +0.0 on pad frames

``stats="clip"``: ``mu`` and ``var`` of every (clip[, channel], band) row over its own valid frames -- utterance-level CMVN; no buffers, train
and eval behave alike.  ``stats="batch"``: of band m over every valid frame of every row of that band; ``running_mean``, ``running_var``
(unbiased) and ``num_batches_tracked`` move in place on the device by ``nn.BatchNorm2d``'s rule, ``eval()`` uses them instead.  The parameter
and buffer names are ``nn.BatchNorm2d``'s, so the ``bn1`` of a (pretrained) ``Cnn6`` loads into a ``BandNorm(n_mels, stats="batch")``
(``BandNorm.from_batchnorm(bn)`` copies it).

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=64, ..., per_clip_lengths=True)
    norm = dmel_amd.BandNorm(64, stats="batch").to("cuda")
    y = norm(layer(x, lengths), layer.frame_lengths(lengths))

A stage of its own (``csrc/dmel_bandnorm.hip`` through ``dmel_bandnorm_forward`` / ``dmel_bandnorm_backward`` of include/dmel.h): it takes any
``(B, n_mels, T)`` or ``(B, C, n_mels, T)`` fp32 tensor, behind the log or behind PCEN, and composes through autograd with everything the
layers do.  ``frame_lengths`` is read on the device only: the call is capturable.  ``s`` and the cotangent are never read at a pad frame; a
``frame_lengths[b]`` outside ``1 ... T`` makes that clip NaN and keeps it out of every statistic and gradient.  Sums are fp64 in a fixed
order: the same inputs give the same bits.  There is no CPU fallback.

Out of scope here: bf16 input or output; fusing the stage into the forward or into PCEN; a ``lengths`` argument on the nets of ``nets.py`` /
``panns.py`` (``Cnn6`` keeps its ``nn.BatchNorm2d``); ``GraphedStep`` / ``LambdAdam`` knowledge of the parameters (``torch.optim.Adam`` and the
plain ``LambdAdam.step()`` work on them as on any fp32 CUDA parameter); ``momentum=None`` (the cumulative average); synchronised statistics
across ranks.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr


class _BandNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, weight, bias, lengths, batch_stats, training, eps, momentum, running_mean, running_var, num_batches_tracked):
        n_mels, T = s.shape[-2], s.shape[-1]
        rows = s.numel() // T if T else 0
        rows_per_clip = (s.shape[1] if s.dim() == 4 else 1) * n_mels
        y = torch.empty_like(s)
        # the (mu, rstd) pairs in fp64: what the backward reads instead of a saved yh
        stats = torch.empty((n_mels if batch_stats else max(rows, 1), 2), dtype=torch.float64, device=s.device)
        scratch = None
        if batch_stats and training:
            scratch = torch.empty(max(capi.bandnorm_scratch_bytes(rows, n_mels) // 8, 2), dtype=torch.float64, device=s.device)
        _stage.launch(capi.bandnorm_forward, s, s.data_ptr(), rows, n_mels, rows_per_clip, T, ptr(lengths), ptr(weight), ptr(bias), batch_stats,
                      training, eps, momentum, ptr(running_mean), ptr(running_var), ptr(num_batches_tracked) if training else None, y.data_ptr(),
                      stats.data_ptr(), ptr(scratch))
        ctx.save_for_backward(s, stats, weight, lengths)
        ctx.batch_stats, ctx.training, ctx.has_bias = batch_stats, training, bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        s, stats, weight, lengths = ctx.saved_tensors
        n_mels, T = s.shape[-2], s.shape[-1]
        rows = s.numel() // T if T else 0
        rows_per_clip = (s.shape[1] if s.dim() == 4 else 1) * n_mels
        g = _stage.cotangent("BandNorm", g)
        want_s, want_w, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        ds = torch.empty_like(s) if want_s else None
        # (an empty tensor launches nothing: its parameter gradients are empty sums)
        mk = torch.zeros if rows == 0 else torch.empty
        dw = mk(n_mels, dtype=torch.float32, device=s.device) if want_w else None
        db = mk(n_mels, dtype=torch.float32, device=s.device) if want_b else None
        scratch = torch.empty(max(capi.bandnorm_scratch_bytes(rows, n_mels) // 8, 2), dtype=torch.float64, device=s.device)
        _stage.launch(capi.bandnorm_backward, s, g.data_ptr(), s.data_ptr(), stats.data_ptr(), rows, n_mels, rows_per_clip, T, ptr(lengths),
                      ptr(weight), ctx.batch_stats, ctx.training, ptr(ds), ptr(dw), ptr(db), scratch.data_ptr())
        return (ds, dw, db) + (None,) * 8


class BandNorm(nn.Module):
    """``BandNorm(n_mels, stats="clip" | "batch")(s, frame_lengths=None)``: s of shape (B, n_mels, T) or (B, C, n_mels, T), fp32, contiguous or
    not, on the GPU; the same shape comes back.  ``frame_lengths``: (B,) int32 or int64 on s's device (``layer.frame_lengths(lengths)``), or
    None for ``T`` valid frames in every clip.  ``weight``, ``bias``: (n_mels,) parameters (None with ``affine=False``); with
    ``stats="batch"`` the buffers ``running_mean``, ``running_var``, ``num_batches_tracked``."""

    def __init__(self, n_mels: int, stats: str = "clip", affine: bool = True, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        if int(n_mels) < 1:
            raise ValueError(f"BandNorm: n_mels must be positive, got {n_mels}")
        if stats not in ("clip", "batch"):
            raise ValueError(f"BandNorm: stats must be 'clip' or 'batch', got {stats!r}")
        if not (eps > 0.0):
            raise ValueError(f"BandNorm: eps must be > 0, got {eps}")
        if momentum is None:
            raise ValueError("BandNorm: momentum=None (the cumulative average) is not supported; pass a float in 0 ... 1")
        if not (0.0 <= float(momentum) <= 1.0):
            raise ValueError(f"BandNorm: momentum must lie in 0 ... 1, got {momentum}")
        self.n_mels, self.stats, self.affine, self.eps, self.momentum = int(n_mels), stats, bool(affine), float(eps), float(momentum)
        if self.affine:
            self.weight = nn.Parameter(torch.ones(self.n_mels, dtype=torch.float32))
            self.bias = nn.Parameter(torch.zeros(self.n_mels, dtype=torch.float32))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        if stats == "batch":
            self.register_buffer("running_mean", torch.zeros(self.n_mels, dtype=torch.float32))
            self.register_buffer("running_var", torch.ones(self.n_mels, dtype=torch.float32))
            self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        else:
            self.running_mean = self.running_var = self.num_batches_tracked = None

    @classmethod
    def from_batchnorm(cls, bn: nn.modules.batchnorm._BatchNorm) -> "BandNorm":
        """a ``BandNorm(bn.num_features, stats="batch")`` with ``bn``'s eps, momentum, parameters and running buffers (copies)"""
        if not isinstance(bn, nn.modules.batchnorm._BatchNorm):
            raise TypeError(f"BandNorm.from_batchnorm takes an nn.BatchNorm1d / 2d / 3d, got {type(bn).__name__}")
        if not bn.track_running_stats:
            raise ValueError("BandNorm.from_batchnorm: the batch norm keeps no running statistics (track_running_stats=False)")
        m = cls(bn.num_features, stats="batch", affine=bn.affine, eps=bn.eps, momentum=bn.momentum)
        m.load_state_dict(bn.state_dict())
        m.train(bn.training)
        return m.to(bn.running_mean.device)

    def extra_repr(self) -> str:
        return f"n_mels={self.n_mels}, stats={self.stats!r}, affine={self.affine}, eps={self.eps}, momentum={self.momentum}"

    def forward(self, s: torch.Tensor, frame_lengths: torch.Tensor | None = None) -> torch.Tensor:
        # (the checks only: this stage works on the tensor as it is given, 3-D or 4-D, and returns that shape)
        _stage.mel_image("BandNorm", s, "an fp32 mel image (a layer with out_dtype=torch.float32)")
        if s.shape[-2] != self.n_mels:
            raise RuntimeError(f"BandNorm was built for n_mels={self.n_mels} but dim -2 of the input has {s.shape[-2]} bands")
        lengths = _stage.frame_lengths_for_kernels("BandNorm", s, frame_lengths)
        for name in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            p = getattr(self, name)
            if p is None:
                continue
            if p.device != s.device:
                raise RuntimeError(f"BandNorm.{name} is on {p.device} but the input is on {s.device}; call norm.to(x.device)")
            want = torch.int64 if name == "num_batches_tracked" else torch.float32
            if p.dtype != want:
                raise RuntimeError(f"BandNorm.{name} must stay {want}, got {p.dtype}")
        _stage.require_gpu("BandNorm", s)
        batch = self.stats == "batch"
        return _BandNormFunction.apply(s.contiguous(), self.weight, self.bias, lengths, batch, bool(self.training) if batch else True, self.eps,
                                       self.momentum, self.running_mean, self.running_var, self.num_batches_tracked)
