"""PCEN: trainable per-channel energy normalisation behind the mel layers (Wang et al. 2017; LEAF learns it next to its filters).

The other standard compression of a trainable audio front end, next to the forward's fused ``log(s + eps)``: an automatic gain control
along time followed by a root, with per-band parameters.  For every row (one (clip[, channel], band) pair of ``T`` frames of LINEAR mel
power ``E >= 0``, i.e. a layer built with ``log=False``):

    M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t];   y = (E (eps + M)^(-alpha) + delta)^r - delta^r

``PCEN`` is a stage of its own (two HIP kernels, ``csrc/dmel_pcen.hip``, through ``dmel_pcen_forward`` / ``dmel_pcen_backward`` of
include/dmel.h): the recurrence runs along the frame axis, across the fused forward's frame tiles.  It takes any contiguous
``(..., n_mels, T)`` fp32 tensor, so it composes through autograd with everything the layers do -- the scalar, multi-window and band-split
layers, per-clip lengths (pad frames are 0 in and exactly 0 out), the trainable filterbank, the waveform gradients; ``lambd.grad`` keeps
coming from the layer's dot kernel, which reads the ``dL/dE`` this stage's backward wrote.

    layer = dmel_amd.MelSpectrogramLayer(lambd, n_mels=128, ..., log=False)
    pcen = dmel_amd.PCEN(128).to("cuda")
    y = pcen(layer(x))
    ...
    optimizer.step(); pcen.project_()

The kernels do not clamp: ``project_()`` brings the parameters back into their ranges after an optimizer step.  There is no CPU fallback.

Out of scope here: fusing PCEN into the forward kernel; a forward-mode tangent through PCEN; bf16 input or output; ``GraphedStep`` and
``LambdAdam`` knowledge of the four parameters (``torch.optim.Adam`` and the plain ``LambdAdam.step()`` work on them as on any fp32 CUDA
parameter; ``LambdAdam(fused_into_backward=...)`` does not apply); a trainable ``eps``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _stage, capi
from ._stage import ptr

ALPHA_RANGE = (0.0, 1.0)
DELTA_MIN = 1e-3
R_RANGE = (1e-3, 1.0)        # 0 < r <= 1: the open end as the smallest root project_() leaves
S_RANGE = (1e-3, 1.0)


class _PCENFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, alpha, delta, r, s, eps):
        n_mels, T = E.shape[-2], E.shape[-1]
        rows = E.numel() // T if T else 0
        y = torch.empty_like(E)
        train = any(ctx.needs_input_grad[:5])
        M = torch.empty_like(E) if train else None
        _stage.launch(capi.pcen_forward, E, E.data_ptr(), rows, n_mels, T, alpha.data_ptr(), delta.data_ptr(), r.data_ptr(), s.data_ptr(), eps,
                      y.data_ptr(), ptr(M))
        if train:
            ctx.save_for_backward(E, M, alpha, delta, r, s)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        E, M, alpha, delta, r, s = ctx.saved_tensors
        n_mels, T = E.shape[-2], E.shape[-1]
        rows = E.numel() // T if T else 0
        g = _stage.cotangent("PCEN", g)
        want_e, want_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5])
        dE = torch.empty_like(E) if want_e else None
        # (an empty tensor launches nothing: its parameter gradients are empty sums)
        dparams = (torch.zeros if rows == 0 else torch.empty)((4, n_mels), dtype=torch.float32, device=E.device) if want_p else None
        scratch = torch.empty(max(capi.pcen_scratch_bytes(rows) // 4, 4), dtype=torch.float32, device=E.device) if want_p else None
        _stage.launch(capi.pcen_backward, E, g.data_ptr(), E.data_ptr(), M.data_ptr(), rows, n_mels, T, alpha.data_ptr(), delta.data_ptr(),
                      r.data_ptr(), s.data_ptr(), ctx.eps, ptr(dE), ptr(dparams), ptr(scratch))
        grads = [dparams[i] if ctx.needs_input_grad[1 + i] else None for i in range(4)]
        return (dE, *grads, None)


class PCEN(nn.Module):
    """``PCEN(n_mels)(E)``: E of shape (B, n_mels, T) or (B, C, n_mels, T), fp32, contiguous or not, on the GPU; the same shape comes back.
    ``alpha``, ``delta``, ``r``, ``s``: (n_mels,) parameters (buffers with ``trainable=False``); ``eps`` is a constant."""

    def __init__(self, n_mels: int, *, alpha: float = 0.96, delta: float = 2.0, r: float = 0.5, s: float = 0.04, eps: float = 1e-6,
                 trainable: bool = True):
        super().__init__()
        if int(n_mels) < 1:
            raise ValueError(f"PCEN: n_mels must be positive, got {n_mels}")
        if not (eps > 0.0):
            raise ValueError(f"PCEN: eps must be > 0, got {eps}")
        self.n_mels, self.eps, self.trainable = int(n_mels), float(eps), bool(trainable)
        for name, value in (("alpha", alpha), ("delta", delta), ("r", r), ("s", s)):
            t = torch.full((self.n_mels,), float(value), dtype=torch.float32)
            if trainable:
                self.register_parameter(name, nn.Parameter(t))
            else:
                self.register_buffer(name, t)

    def extra_repr(self) -> str:
        return f"n_mels={self.n_mels}, eps={self.eps}, trainable={self.trainable}"

    @torch.no_grad()
    def project_(self) -> "PCEN":
        """clamps the parameters in place to 0 <= alpha <= 1, delta >= 1e-3, 1e-3 <= r <= 1, 1e-3 <= s <= 1 (one launch each): call it after
        ``optimizer.step()``"""
        self.alpha.clamp_(*ALPHA_RANGE)
        self.delta.clamp_(min=DELTA_MIN)
        self.r.clamp_(*R_RANGE)
        self.s.clamp_(*S_RANGE)
        return self

    def forward(self, E: torch.Tensor) -> torch.Tensor:
        # (the checks only: this stage works on the tensor as it is given, 3-D or 4-D, and returns that shape)
        _stage.mel_image("PCEN", E, "fp32 linear mel power (a layer with log=False, out_dtype=torch.float32)")
        if E.shape[-2] != self.n_mels:
            raise RuntimeError(f"PCEN was built for n_mels={self.n_mels} but dim -2 of the input has {E.shape[-2]} bands")
        for name in ("alpha", "delta", "r", "s"):
            p = getattr(self, name)
            if p.device != E.device:
                raise RuntimeError(f"PCEN.{name} is on {p.device} but the input is on {E.device}; call pcen.to(x.device)")
            if p.dtype != torch.float32:
                raise RuntimeError(f"PCEN.{name} must stay fp32, got {p.dtype}")
        _stage.require_gpu("PCEN", E)
        return _PCENFunction.apply(E.contiguous(), self.alpha, self.delta, self.r, self.s, self.eps)
