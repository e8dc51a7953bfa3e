"""What the stages behind the mel layers (PCEN, BandNorm, SpecMask, Deltas, StatsPool, AttentivePool) share on the host: the checks of the
mel image, of ``frame_lengths`` and of the cotangent, and the plumbing of a launch.  Private: nothing here is exported from the package.

A stage's ``forward`` keeps the order that decides which error a doubly wrong call gets: ``mel_image`` (shape, then dtype),
``frame_lengths_for_kernels``, the stage's own checks, its early return for an empty tensor, ``T == 0``, ``require_gpu``."""
from __future__ import annotations

import math

import torch

FP32 = (torch.float32,)


def mel_image(name: str, s, takes: str = "an fp32 mel image", dtypes=FP32) -> torch.Tensor:
    """a tensor, 3-D or 4-D, of one of ``dtypes`` (``takes`` says so in the refusal); returns the (B, C, n_mels, T) view"""
    if not torch.is_tensor(s) or s.dim() not in (3, 4):
        raise ValueError(f"{name}: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got {tuple(s.shape) if torch.is_tensor(s) else type(s).__name__}")
    if s.dtype not in dtypes:
        raise RuntimeError(f"{name} takes {takes}, got {s.dtype}")
    return s.unsqueeze(1) if s.dim() == 3 else s


def require_gpu(name: str, s: torch.Tensor) -> None:
    if not s.is_cuda:
        raise RuntimeError(f"dmel_amd runs on MI355X only: {name}'s input must be a CUDA/HIP tensor (no CPU fallback)")


def frame_lengths_for_kernels(name: str, s: torch.Tensor, frame_lengths) -> torch.Tensor | None:
    """shape, dtype and device of ``frame_lengths`` (None stays None: ``T`` valid frames in every clip); returns them as the kernels read
    them (int32, contiguous).  Their values never leave the device."""
    if frame_lengths is None:
        return None
    if not torch.is_tensor(frame_lengths):
        raise TypeError(f"{name}: frame_lengths must be a 1-D integer tensor, got {type(frame_lengths).__name__}")
    if frame_lengths.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: frame_lengths must hold int32 or int64 values, got {frame_lengths.dtype}")
    if frame_lengths.dim() != 1 or frame_lengths.shape[0] != s.shape[0]:
        raise ValueError(f"{name}: frame_lengths must have shape ({s.shape[0]},), got {tuple(frame_lengths.shape)}")
    if frame_lengths.device != s.device:
        raise RuntimeError(f"{name}: frame_lengths is on {frame_lengths.device} but the input is on {s.device}")
    if frame_lengths.dtype != torch.int32:
        # int64 values clamped on the device before the narrowing: 2**32 + 5 must stay invalid (NaN), not wrap to 5
        frame_lengths = frame_lengths.clamp(0, s.shape[-1] + 1).to(torch.int32)
    return frame_lengths.contiguous()


def pool_stats(name: str, known: tuple, stats, eps) -> tuple:
    """the constructor arguments of the pooling stages: ``stats`` as a tuple in the order of ``known``, ``eps`` as a float"""
    if isinstance(stats, str):
        stats = (stats,)
    try:
        given = list(stats)
    except TypeError:
        raise ValueError(f"{name}: stats must be a non-empty subset of {known}, got {stats!r}") from None
    if not given or any(not isinstance(k, str) or k not in known for k in given):
        raise ValueError(f"{name}: stats must be a non-empty subset of {known}, got {stats!r}")
    if len(set(given)) != len(given):
        raise ValueError(f"{name}: stats names a statistic twice: {stats!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or not eps > 0:
        raise ValueError(f"{name}: eps must be a finite number > 0, got {eps!r}")
    return tuple(k for k in known if k in given), float(eps)


def ptr(t):
    """the address the C ABI takes: None stays None (a NULL pointer)"""
    return None if t is None else t.data_ptr()


def cotangent(name: str, g: torch.Tensor, dtypes=FP32, takes: str = "fp32") -> torch.Tensor:
    if g.dtype not in dtypes:
        raise RuntimeError(f"{name}: the gradient of the output must be {takes}, got {g.dtype}")
    return g.contiguous()


def launch(fn, t: torch.Tensor, *args) -> None:
    """``fn(*args, stream)`` on ``t``'s device and its current stream"""
    with torch.cuda.device(t.device):
        fn(*args, torch.cuda.current_stream(t.device).cuda_stream)
