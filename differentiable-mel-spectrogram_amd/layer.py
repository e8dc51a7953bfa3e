"""Host-side mirror of the reference's layer interface, running on libdmel_hip.so.

``MelSpectrogramLayer`` keeps the constructor, attributes, parameter name (``lambd``), output
shape/dtype and error behaviour of the reference's ``models.MelSpectrogramLayer``
(models.py:14-56) so that the wrapping nets (models.py:58-166), the two-LR-group optimizer keyed
on ``"spectrogram_layer.lambd"`` (main.py:36-48) and ``load_state_dict(strict=True)``
(utils.py:270) work unchanged.  The arithmetic runs in the HIP kernels behind the C ABI
(``include/dmel.h``), reached in two ways: the hot path goes through the torch-registered ops
``torch.ops.dmel.*`` (csrc/dmel_torch.cpp, a C++ autograd function: forward + backward to
``lambd.grad``), the optional gradients (waveform, learnable filterbank) and the DSPEC layer through
``ctypes`` (``capi.py``).  torch is used for device memory, streams and autograd plumbing only.
There is no CPU fallback.

``lambd`` normally never leaves the device (``lambd_sync=False``): the kernels read it themselves and
check the n_fft they were launched for (include/dmel.h, dmel_forward_dev), so a training step queues
without the host waiting and can be captured into a HIP graph.  ``lambd_sync=True`` reads it to the
host at every forward, as the reference does (time_frequency.py:39).

Layout of this file.  What the autograd Functions share is written once, in front of them: ``_cotangent`` (the incoming
gradient), ``_alloc`` (output, tangent, scratch and the rule for a bf16 log output whose backward needs fp32 values),
``_lambd_f32``, ``_launched_for`` (the n_fft candidates of a tracked forward), ``_tracked_backward_x`` (the waveform gradient over
them) and ``_dl_like``.  What the modules share sits in front of them: ``_check_input`` (every refusal of every ``forward``, in one
order), ``_as_f32_contiguous`` and the plan cache (``_PlanCache``; with lambd tracking ``_PlanCachingModule``).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import capi


def _stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


class _on_device:
    """``torch.cuda.device(dev)`` only when ``dev`` is not already current: the context manager costs ~8 us of host time per
    use, which is a third of the forward kernel at BASELINE config 2."""

    __slots__ = ("ctx",)

    def __init__(self, dev):
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.ctx = None if idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def _ptr(t):
    """the device address of an optional tensor"""
    return None if t is None else t.data_ptr()


def _cotangent(grad_out):
    """(g, is_bf16): the gradient of a bf16 output is read as it is and widened in the kernel, any other dtype goes to fp32;
    contiguous either way."""
    bf16 = grad_out.dtype == torch.bfloat16
    g = grad_out
    if not bf16 and g.dtype != torch.float32:
        g = g.to(torch.float32)
    if not g.is_contiguous():
        g = g.contiguous()
    return g, bf16


def _alloc(x, shape, out_dtype, want_tangent, keeps_log_out=False, scratch_bytes=None):
    """(out, tangent, scratch, round_later) of one forward on x's device: the output (models.py:36, fp32 there), the fp32 tangent
    d out / d lambd when a gradient to lambd will be asked for, and the launch's scratch when it takes one.
    ``keeps_log_out``: the backward rebuilds 1 / (mel + eps) from the saved log output (dL/dx, dL/dfb).  That needs the fp32 values, so
    a bf16 output is then produced in fp32 (``round_later``) and rounded by the caller after it has been saved, instead of in the
    kernel: bit-identical either way."""
    round_later = out_dtype == torch.bfloat16 and keeps_log_out
    out = torch.empty(shape, dtype=torch.float32 if round_later else out_dtype, device=x.device)
    tangent = torch.empty(shape, dtype=torch.float32, device=x.device) if want_tangent else None
    scratch = None if scratch_bytes is None else torch.empty((scratch_bytes,), dtype=torch.uint8, device=x.device)
    return out, tangent, scratch, round_later


def _out_flag(out) -> int:
    return capi.DMEL_FLAG_OUT_BF16 if out.dtype == torch.bfloat16 else 0


def _lambd_f32(lambd):
    """lambd as the kernels read it from the device: detached, fp32, contiguous (a (K,) parameter may be a strided view)"""
    lam = lambd.detach()
    if lam.dtype != torch.float32 or not lam.is_contiguous():
        lam = lam.to(torch.float32).contiguous()
    return lam


def _launched_for(plan):
    """The n_fft candidates the tracked forward just issued on ``plan`` launched for: n0, 2 n0, n0 // 2 as its guards say (host-side
    bookkeeping of the plan: no device read)."""
    n0, guards = plan.info()["n_fft"], plan.lambd_status()["guards"]
    return [n0] + ([2 * n0] if guards & 2 else []) + ([n0 // 2] if (guards & 1) and n0 >= 2 else [])


def _tracked_backward_x(plan, x, lengths, lam, cands, g32, out, log, stream):
    """The waveform gradient of a tracked forward, without a host read: one dmel_backward_x_dev(_lengths) per candidate n_fft
    (DMEL_FLAG_CHECK_NFFT: the device value of lambd picks the one that works) over a NaN-filled grad_x; a lambd no launch covered
    leaves the NaN, as that forward's output is."""
    gx = torch.full_like(x, float("nan"))
    for n in cands:
        if lengths is None:
            plan.backward_x_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), n, g32.data_ptr(), _ptr(out), gx.data_ptr(), log, stream,
                                extra_flags=capi.DMEL_FLAG_CHECK_NFFT)
        else:
            plan.backward_x_dev_lengths(x.data_ptr(), lengths.data_ptr(), x.shape[0], lam.data_ptr(), n, g32.data_ptr(), _ptr(out),
                                        gx.data_ptr(), log, stream, extra_flags=capi.DMEL_FLAG_CHECK_NFFT)
    return gx


def _dl_like(dl, shape, dtype):
    """the fp32 gradient the kernels wrote, in the shape and dtype of the parameter ``lambd``"""
    if dl.shape != shape:
        dl = dl.reshape(shape)
    if dtype != torch.float32:
        dl = dl.to(dtype)
    return dl


class _DmelFunction(torch.autograd.Function):
    """forward: dmel_forward (carries d out / d lambd); backward: dmel_backward (one dot product) and, when a
    filterbank tensor that requires grad was passed, dmel_backward_fb (adjoint of models.py:53)."""

    @staticmethod
    def forward(ctx, x, lambd, plan, lam_host, log, eps, full_window=False, fb=None, out_dtype=torch.float32):
        B = x.shape[0]
        want_x, want_tangent = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_fb = fb is not None and ctx.needs_input_grad[7]
        out, tangent, _, round_later = _alloc(x, (B, 1, plan.n_mels, plan.n_time), out_dtype, want_tangent, log and (want_x or want_fb))
        flags = capi.DMEL_FLAG_FULL_WINDOW if full_window else 0
        with _on_device(x.device):
            plan.forward(x.data_ptr(), B, lam_host, out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                         extra_flags=flags | _out_flag(out))
        ctx.plan = plan
        ctx.lambd_shape = lambd.shape
        ctx.lambd_dtype = lambd.dtype
        ctx.want_tangent, ctx.want_fb, ctx.want_x = want_tangent, want_fb, want_x
        ctx.fb_args = (lam_host, bool(log), flags, None if fb is None else (tuple(fb.shape), fb.dtype))
        saved = []
        if want_tangent:
            saved.append(tangent)
        if want_fb or want_x:
            saved.append(x)
            if log:
                saved.append(out)
        ctx.save_for_backward(*saved)
        return out.to(torch.bfloat16) if round_later else out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        g, bf16 = _cotangent(grad_out)
        dl = gfb = gx = None
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent = saved.pop(0)
                dl = torch.empty((1,), dtype=torch.float32, device=g.device)
                ctx.plan.backward(g.data_ptr(), tangent.data_ptr(), g.numel(), dl.data_ptr(), _stream_ptr(g.device), grad_bf16=bf16)
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
            if ctx.want_fb or ctx.want_x:
                lam_host, log, flags, fb_meta = ctx.fb_args
                x = saved.pop(0)
                out = saved.pop(0).to(torch.float32) if log else None
                g = g.to(torch.float32)
            if ctx.want_x:
                gx = torch.empty_like(x)
                ctx.plan.backward_x(x.data_ptr(), x.shape[0], lam_host, g.data_ptr(), _ptr(out), gx.data_ptr(), log, _stream_ptr(g.device),
                                    extra_flags=flags)
            if ctx.want_fb:
                fb_shape, fb_dtype = fb_meta
                gfb = torch.empty(fb_shape, dtype=torch.float32, device=g.device)
                ctx.plan.backward_fb(x.data_ptr(), x.shape[0], lam_host, g.data_ptr(), _ptr(out), gfb.data_ptr(), log, _stream_ptr(g.device),
                                     extra_flags=flags)
                gfb = gfb.to(fb_dtype)
        return gx, dl, None, None, None, None, None, gfb, None


class _DmelFbDevFunction(torch.autograd.Function):
    """The layer with lambd left on the device wherever the transform length does not hang on lambd's host value: a trainable
    filterbank (its row count fixes n_fft: dmel_forward_dev_fixed checks lambd against it on the device) and the optimized=False
    branch (n_fft = 2 n_points whatever lambd is), with or without the gradients w.r.t. the filterbank (dmel_backward_fb_dev) and the
    waveform (dmel_backward_x_dev).  No host read anywhere: the step queues without waiting and can be captured into a HIP graph.
    With ``lengths`` (a trainable filterbank with ``lengths_learnable_fb=True``; int32 on x's device) the forward is
    dmel_forward_dev_fixed_lengths and the filterbank gradient dmel_backward_fb_saved_lengths / dmel_backward_fb_dev_lengths, which stop at
    each clip's last frame; ``lengths`` is kept for the backward next to ``x`` and ``lam``.

    ``n_fft == 0`` (HTK bank, optimized=True, x.requires_grad): the tracked forward dmel_forward_dev -- one launch per candidate n_fft,
    the device value of lambd picks the one that works -- and a waveform gradient issued the same way (_tracked_backward_x)."""

    @staticmethod
    def forward(ctx, x, lambd, plan, n_fft, log, eps, fb, out_dtype, full_window=False, mfma_flags=0, save_spec=False, lengths=None):
        B = x.shape[0]
        if lengths is not None and (n_fft == 0 or full_window or fb is None or ctx.needs_input_grad[0]):
            raise ValueError("lengths here are a trainable filterbank's (fixed n_fft, optimized=True, no waveform gradient)")
        want_x, want_tangent = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_fb = fb is not None and ctx.needs_input_grad[6]
        tracked = n_fft == 0
        if tracked and (fb is not None or full_window):
            raise ValueError("n_fft = 0 (tracked forward) is the HTK bank with optimized=True")
        # the spectrogram the contraction consumes, kept for the filterbank gradient (fused training kernel only)
        keep_spec = bool(save_spec and want_fb and want_tangent and not full_window and 32 <= n_fft <= 16384 and (n_fft & (n_fft - 1)) == 0)
        out, tangent, scratch, round_later = _alloc(x, (B, 1, plan.n_mels, plan.n_time), out_dtype, want_tangent, log and (want_fb or want_x),
                                                    plan.scratch_bytes(B))
        lam = _lambd_f32(lambd)
        flags = (capi.DMEL_FLAG_FULL_WINDOW if full_window else 0) | int(mfma_flags)
        spec = torch.empty((B, n_fft // 2 + 1, plan.n_time), dtype=torch.float32, device=x.device) if keep_spec else None
        ctx.cands = None
        with _on_device(x.device):
            if lengths is not None:
                plan.forward_dev_fixed_lengths(x.data_ptr(), lengths.data_ptr(), B, lam.data_ptr(), n_fft, out.data_ptr(), _ptr(tangent), _ptr(spec),
                                               log, eps, _stream_ptr(x.device), scratch.data_ptr(), extra_flags=flags | _out_flag(out))
            elif tracked:
                plan.forward_dev(x.data_ptr(), B, lam.data_ptr(), out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                                 scratch.data_ptr(), extra_flags=_out_flag(out))
                ctx.cands = _launched_for(plan)
            elif keep_spec:
                plan.forward_dev_fixed_spec(x.data_ptr(), B, lam.data_ptr(), n_fft, out.data_ptr(), tangent.data_ptr(), spec.data_ptr(),
                                            log, eps, _stream_ptr(x.device), scratch.data_ptr(), extra_flags=flags | _out_flag(out))
            else:
                plan.forward_dev_fixed(x.data_ptr(), B, lam.data_ptr(), n_fft, out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                                       scratch.data_ptr(), extra_flags=flags | _out_flag(out))
        ctx.plan, ctx.n_fft, ctx.log, ctx.flags, ctx.keep_spec = plan, n_fft, bool(log), flags, keep_spec
        ctx.lambd_shape, ctx.lambd_dtype = lambd.shape, lambd.dtype
        ctx.want_tangent, ctx.want_fb, ctx.want_x = want_tangent, want_fb, want_x
        ctx.fb_meta = None if fb is None else (tuple(fb.shape), fb.dtype)
        ctx.has_lengths = lengths is not None
        saved = [scratch]
        if want_tangent:
            saved.append(tangent)
        if want_fb or want_x:
            saved += [x, lam]
            if lengths is not None:
                saved.append(lengths)
            if log:
                saved.append(out)
        if keep_spec:
            saved.append(spec)
        ctx.save_for_backward(*saved)
        return out.to(torch.bfloat16) if round_later else out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        spec = saved.pop() if ctx.keep_spec else None
        scratch = saved.pop(0)
        g, bf16 = _cotangent(grad_out)
        dl = gfb = gx = None
        # d lambd rides in the launch of the filterbank gradient (dmel_backward_fb_saved_dl: one kernel less per step, the same bits)
        ride = ctx.want_tangent and ctx.want_fb and spec is not None and not bf16 and g.numel() > 0
        stream = _stream_ptr(g.device)
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent = saved.pop(0)
                dl = torch.empty(tuple(ctx.lambd_shape), dtype=torch.float32, device=g.device)
                if not ride:
                    ctx.plan.backward_scratch(g.data_ptr(), tangent.data_ptr(), g.numel(), dl.data_ptr(), stream, scratch.data_ptr(), grad_bf16=bf16)
            if ctx.want_fb or ctx.want_x:
                x, lam = saved.pop(0), saved.pop(0)
                lengths = saved.pop(0) if ctx.has_lengths else None
                out = saved.pop(0).to(torch.float32) if ctx.log else None
                g32 = g.to(torch.float32)
            if ctx.want_x and ctx.cands is not None and max(ctx.cands) > 16384:
                # transforms beyond the fused kernels have no checked backward: the one case that reads lambd (n_fft >= 16384)
                gx = torch.empty_like(x)
                ctx.plan.backward_x(x.data_ptr(), x.shape[0], float(lam), g32.data_ptr(), _ptr(out), gx.data_ptr(), ctx.log, stream)
            elif ctx.want_x and ctx.cands is not None:
                gx = _tracked_backward_x(ctx.plan, x, None, lam, ctx.cands, g32, out, ctx.log, stream)
            elif ctx.want_x:
                gx = torch.empty_like(x)
                ctx.plan.backward_x_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), ctx.n_fft, g32.data_ptr(), _ptr(out), gx.data_ptr(), ctx.log,
                                        stream, extra_flags=ctx.flags)
            if ctx.want_fb:
                fb_shape, fb_dtype = ctx.fb_meta
                gfb = torch.empty(fb_shape, dtype=torch.float32, device=g.device)
                if lengths is not None and spec is not None:
                    ctx.plan.backward_fb_saved_lengths(spec.data_ptr(), lengths.data_ptr(), x.shape[0], ctx.n_fft, g32.data_ptr(), _ptr(out),
                                                       tangent.data_ptr() if ride else None, gfb.data_ptr(), dl.data_ptr() if ride else None,
                                                       scratch.data_ptr(), ctx.log, stream, extra_flags=ctx.flags)
                elif lengths is not None:
                    ctx.plan.backward_fb_dev_lengths(x.data_ptr(), lengths.data_ptr(), x.shape[0], lam.data_ptr(), ctx.n_fft, g32.data_ptr(),
                                                     _ptr(out), gfb.data_ptr(), ctx.log, stream, extra_flags=ctx.flags)
                elif ride:
                    ctx.plan.backward_fb_saved_dl(spec.data_ptr(), x.shape[0], ctx.n_fft, g32.data_ptr(), _ptr(out), tangent.data_ptr(),
                                                  gfb.data_ptr(), dl.data_ptr(), scratch.data_ptr(), ctx.log, stream, extra_flags=ctx.flags)
                elif spec is not None:
                    ctx.plan.backward_fb_saved(spec.data_ptr(), x.shape[0], ctx.n_fft, g32.data_ptr(), _ptr(out), gfb.data_ptr(), ctx.log, stream,
                                               extra_flags=ctx.flags)
                else:
                    ctx.plan.backward_fb_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), ctx.n_fft, g32.data_ptr(), _ptr(out), gfb.data_ptr(),
                                             ctx.log, stream, extra_flags=ctx.flags)
                gfb = gfb.to(fb_dtype)
            if dl is not None:
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
        return gx, dl, None, None, None, None, gfb, None, None, None, None, None


class _DmelLenXFunction(torch.autograd.Function):
    """forward(x, lengths) with a waveform gradient (``MelSpectrogramLayer(lengths_waveform_grad=True)`` and ``x.requires_grad``): the
    launches of torch.ops.dmel.mel_spectrogram_lengths -- dmel_forward_dev_lengths, or dmel_forward_lengths when ``lam_host`` is given
    (lambd_sync) -- with ``x``, ``lengths`` and the fp32 output kept for the backward.  backward: the same dot product for ``lambd`` and
    dmel_backward_x_lengths for ``x``; with lambd on the device _tracked_backward_x over what the forward launched for, as
    _DmelFbDevFunction: no host read, the step can be captured into a HIP graph.  (The lengths path never launches below n_fft 32.)"""

    @staticmethod
    def forward(ctx, x, lengths, lambd, plan, lam_host, log, eps, out_dtype):
        B = x.shape[0]
        want_x, want_tangent = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        out, tangent, scratch, round_later = _alloc(x, (B, 1, plan.n_mels, plan.n_time), out_dtype, want_tangent, log and want_x,
                                                    plan.scratch_bytes(B))
        lam = _lambd_f32(lambd)
        ctx.cands = None
        with _on_device(x.device):
            if lam_host is not None:
                plan.forward_lengths(x.data_ptr(), lengths.data_ptr(), B, lam_host, out.data_ptr(), _ptr(tangent), log, eps,
                                     _stream_ptr(x.device), scratch.data_ptr(), extra_flags=_out_flag(out))
            else:
                plan.forward_dev_lengths(x.data_ptr(), lengths.data_ptr(), B, lam.data_ptr(), out.data_ptr(), _ptr(tangent), log, eps,
                                         _stream_ptr(x.device), scratch.data_ptr(), extra_flags=_out_flag(out))
                ctx.cands = _launched_for(plan)
        ctx.plan, ctx.lam_host, ctx.log = plan, lam_host, bool(log)
        ctx.lambd_shape, ctx.lambd_dtype = lambd.shape, lambd.dtype
        ctx.want_tangent, ctx.want_x = want_tangent, want_x
        saved = [scratch]
        if want_tangent:
            saved.append(tangent)
        if want_x:
            saved += [x, lengths, lam]
            if log:
                saved.append(out)
        ctx.save_for_backward(*saved)
        return out.to(torch.bfloat16) if round_later else out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        scratch = saved.pop(0)
        g, bf16 = _cotangent(grad_out)
        dl = gx = None
        stream = _stream_ptr(g.device)
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent = saved.pop(0)
                dl = torch.empty(tuple(ctx.lambd_shape), dtype=torch.float32, device=g.device)
                ctx.plan.backward_scratch(g.data_ptr(), tangent.data_ptr(), g.numel(), dl.data_ptr(), stream, scratch.data_ptr(), grad_bf16=bf16)
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
            if ctx.want_x:
                x, lengths, lam = saved.pop(0), saved.pop(0), saved.pop(0)
                out = saved.pop(0) if ctx.log else None
                g32 = g.to(torch.float32)
                if ctx.cands is None:
                    gx = torch.empty_like(x)
                    ctx.plan.backward_x_lengths(x.data_ptr(), lengths.data_ptr(), x.shape[0], ctx.lam_host, g32.data_ptr(), _ptr(out),
                                                gx.data_ptr(), ctx.log, stream)
                else:
                    gx = _tracked_backward_x(ctx.plan, x, lengths, lam, ctx.cands, g32, out, ctx.log, stream)
        return gx, None, dl, None, None, None, None, None


class SlotInput:
    """A batch handed to the layer BY ADDRESS (round 5): ``cell`` is a one-element int64 device tensor holding the address of a contiguous
    fp32 ``(batch, n_points)`` tensor on the same device; the fused forward reads that address when it RUNS (``DMEL_FLAG_X_INDIRECT``).
    A step captured into a HIP graph reads static addresses -- with a ``SlotInput`` the static address is the cell's, and giving the
    replayed step a new batch is an 8-byte write instead of a copy of the batch (``GraphedStep(..., zero_copy=[True, ...]).feed``).
    Only the layer understands it: pass it where the step passes ``x`` to ``net(x)`` / ``layer(x)`` (the reference's nets hand ``x``
    to the layer and to nothing else, models.py:70,93,122,154)."""

    __slots__ = ("cell", "shape", "device")

    def __init__(self, cell, shape):
        if cell.dtype != torch.int64 or cell.numel() != 1 or not cell.is_cuda:
            raise ValueError("SlotInput: cell must be a one-element int64 device tensor")
        self.cell, self.shape, self.device = cell, tuple(int(v) for v in shape), cell.device

    def dim(self):
        return len(self.shape)

    def view(self):
        """the (batch, n_points) fp32 view with zero strides whose data pointer is the cell's (what torch.ops.dmel.* is handed)"""
        return torch.as_strided(self.cell.view(torch.float32), self.shape, (0,) * len(self.shape))


_MEL_OP = None


def _mel_op():
    """torch.ops.dmel.mel_spectrogram.default, resolved once (the packet lookup costs microseconds per call)."""
    global _MEL_OP
    if _MEL_OP is None:
        _MEL_OP = capi.torch_ops().mel_spectrogram.default
    return _MEL_OP


_LEN_OP = None


def _len_op():
    """torch.ops.dmel.mel_spectrogram_lengths.default, resolved once."""
    global _LEN_OP
    if _LEN_OP is None:
        _LEN_OP = capi.torch_ops().mel_spectrogram_lengths.default
    return _LEN_OP


def _as_f32_contiguous(x: torch.Tensor, lengths=None) -> torch.Tensor:
    """``x`` as the kernels read it: fp32 and contiguous.  Nothing is called on a tensor that already is (each no-op torch call still
    costs ~2 us of host time on the hot path); when x requires grad its gradient flows back through these torch ops.
    The kernels compute in fp32.  The reference removes the clip mean in the INPUT dtype (models.py:38: ``x[idx] - torch.mean(x[idx])``):
    for fp64 clips (GaussPulse, datasets.py:33) that subtraction happens here, in fp64, BEFORE the cast -- a DC offset far above the
    signal would otherwise cost the signal its low bits in the rounding to fp32 (tests/golden g13_dc_*_fp64: 1e-2 on the lowest mel
    band).  The kernels' own DC removal then finds a mean of rounding size.  Narrower dtypes are widened as they are.
    With ``lengths`` (forward(x, lengths)) an fp64 clip loses its own mean, over ``x[b, :lengths[b]]``: a masked sum divided by the
    length, on the device (no host read, so a captured step stays capturable).  Samples past a clip are masked out of the sum (NaN or
    inf there reaches no output); an invalid length changes only its own clip, which the kernel makes NaN."""
    if x.dtype != torch.float32:
        if x.dtype == torch.float64 and lengths is None:
            x = x - x.mean(dim=1, keepdim=True)
        elif x.dtype == torch.float64:
            inside = torch.arange(x.shape[1], device=x.device)[None, :] < lengths[:, None]
            mean = torch.where(inside, x, 0.0).sum(dim=1, keepdim=True) / lengths.clamp(min=1)[:, None].to(torch.float64)
            x = x - mean
        x = x.to(torch.float32)
    return x if x.is_contiguous() else x.contiguous()


def _lambd_for_op(lam):
    """lambd as torch.ops.dmel.* take it: the parameter itself (their autograd node returns its gradient), through a cast unless fp32"""
    return lam if lam.dtype == torch.float32 else lam.to(torch.float32)


def _no_lengths(name: str) -> str:
    return f"{name} does not take per-clip lengths (MelSpectrogramLayer does)"


def _frame_lengths(lengths, hop_length):
    """Valid frames per clip of a ``forward(x, lengths)``: ``lengths // hop_length + 1`` (models.py:30 at ``n_points = lengths[b]``), on the
    tensor's own device.  One definition for every layer that takes lengths."""
    return lengths // hop_length + 1


def _lengths_for_kernels(x, lengths, n_points):
    """Type, dtype, shape and device of the ``lengths`` of a ``forward(x, lengths)``; returns them as the kernels read them (int32,
    contiguous, on x's device).  Their values never leave the device.  One copy for every layer that takes lengths."""
    if not torch.is_tensor(lengths):
        raise TypeError(f"lengths must be a 1-D integer tensor, got {type(lengths).__name__}")
    if lengths.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"lengths must hold int32 or int64 values, got {lengths.dtype}")
    if lengths.dim() != 1 or lengths.shape[0] != x.shape[0]:
        raise ValueError(f"lengths must have shape ({x.shape[0]},), got {tuple(lengths.shape)}")
    if lengths.device.type == "cpu":
        lengths = lengths.to(x.device)
    elif lengths.device != x.device:
        raise RuntimeError(f"lengths is on {lengths.device} but x is on {x.device}")
    if lengths.dtype != torch.int32:
        # int64 values clamped on the device before the narrowing: a length such as 2**32 + 4000 must stay invalid (NaN), not wrap to 4000
        lengths = lengths.clamp(0, n_points + 1).to(torch.int32)
    return lengths if lengths.is_contiguous() else lengths.contiguous()


def _check_input(name, x, lambd, lengths=None, *, n_points=None, check_lengths=None, refuse_slot=None, slot_config_ok=None,
                 refuse_x_grad=None):
    """Every refusal the ``forward`` of a layer class starts with, in one order (the order decides which error wins when two apply).
    ``name``: the class, for the messages.  What the class accepts:
      ``n_points``       the clip length it was built for; None: any (SpectrogramLayer, optimized=False)
      ``check_lengths``  None: per-clip lengths are refused; else ``(x, lengths) -> lengths`` that validates and converts them
      ``refuse_slot``    the message a class that takes no SlotInput refuses one with
      ``slot_config_ok`` ``() -> bool`` of the one class that takes a SlotInput: is this layer configured as a slot needs
      ``refuse_x_grad``  the message an ``x`` that requires grad is refused with; None: it is accepted
    Returns the converted ``lengths`` (None without them)."""
    if lengths is not None and check_lengths is None:
        raise RuntimeError(_no_lengths(name))
    if refuse_slot is not None and isinstance(x, SlotInput):
        raise RuntimeError(refuse_slot)
    if x.dim() != 2:
        raise ValueError(f"expected x of shape (batch, n_points), got {tuple(x.shape)}")
    if n_points is not None and x.shape[1] != n_points:
        # the reference fails here too (RuntimeError from the slice-assign at models.py:54)
        raise RuntimeError(f"input has {x.shape[1]} points, the layer was built for n_points={n_points}")
    if lengths is not None:
        lengths = check_lengths(x, lengths)
    if slot_config_ok is not None and isinstance(x, SlotInput):
        # the batch by address: the hot path only (HTK bank, optimized=True, lambd on the device)
        if not slot_config_ok():
            raise RuntimeError("a SlotInput needs the default layer: HTK bank, optimized=True, lambd_sync=False")
        if lambd.device != x.device:
            raise RuntimeError(f"lambd is on {lambd.device} but the slot is on {x.device}; call layer.to(device)")
        return lengths
    if not x.is_cuda:
        raise RuntimeError("dmel_amd runs on MI355X only: x must be a CUDA/HIP tensor (no CPU fallback)")
    if refuse_x_grad is not None and x.requires_grad:
        raise RuntimeError(refuse_x_grad)
    if lambd.device != x.device:
        raise RuntimeError(f"lambd is on {lambd.device} but x is on {x.device}; call layer.to(x.device)")
    return lengths


class _PlanCache(nn.Module):
    """A module with a cache of capi.Plan objects (device tables), one per device and, where a subclass says so, per shape.  Plans are
    not state: copies and pickles of the layer start without them and rebuild them on first use."""

    def __init__(self):
        super().__init__()
        self._plans = {}                                              # device index [, shape key ...] -> capi.Plan

    def _make_plan(self, *shape_key) -> capi.Plan:
        """the plan of this layer's mel configuration (called on the plan's device)"""
        return capi.Plan(self.n_points, self.hop_length, self.n_mels, self.sample_rate, float(self.f_min), float(self.f_max),
                         bool(self.normalize_window))

    def _plan_for(self, dev: torch.device, *shape_key) -> capi.Plan:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        key = (idx,) + shape_key if shape_key else idx
        plan = self._plans.get(key)
        if plan is None:
            with torch.cuda.device(idx):
                plan = self._make_plan(*shape_key)
            if getattr(self, "_tracking", None) is not None:
                plan.set_tracking(*self._tracking)
            self._plans[key] = plan
        return plan

    def _plan_on(self, device=None) -> capi.Plan:
        """the plan on ``device`` (default: the current one), for the status calls"""
        return self._plan_for(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}
        return state


class _PlanCachingModule(_PlanCache):
    """_PlanCache of a layer whose sync-free path tracks ``lambd`` on the host side of its plans."""

    def resync(self):
        """Forget what the sync-free path knows about lambd (every channel's; call after rewriting it from outside the optimizer, e.g.
        ``layer.lambd.data.fill_(v)``); the next forward reads it once.  ``load_state_dict`` does this by itself."""
        for plan in self._plans.values():
            plan.lambd_reset()

    def set_tracking(self, max_ahead: int = 8, guard_mode: int = 0):
        """Run-ahead bound and guard policy of the sync-free path (dmel_plan_set_tracking); applies to plans made later too."""
        self._tracking = (int(max_ahead), int(guard_mode))
        for plan in self._plans.values():
            plan.set_tracking(*self._tracking)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.resync()


class MelSpectrogramLayer(_PlanCachingModule):
    """Differentiable (log-)Mel spectrogram with a trainable Gaussian window width.

    Signature-compatible with the reference (models.py:15):
        MelSpectrogramLayer(init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None,
                            hop_length=1, device='cpu', optimized=False, normalize_window=False)
    Extra keyword-only options: ``log=True`` fuses ``torch.log(s + eps)`` (models.py:73) into the
    kernel epilogue (default False = linear mel power, exactly what the reference layer returns).
    ``learnable_fb=True`` registers the (n_fft/2+1, n_mels) filterbank of models.py:42-48 as a second
    parameter ``mel_fb`` (initialised to the HTK bank) and returns its gradient; the matrix is tied to the
    n_fft it was built for, so the forward raises once ``lambd`` has moved to another power of two.  Off by
    default: the reference has no such parameter and its checkpoints have no such key.
    ``out_dtype=torch.bfloat16`` stores the output as bf16 (the fp32 result rounded to nearest even; BASELINE config 2
    "bf16 activations"); the arithmetic, the saved tangent and ``lambd.grad`` stay fp32.
    ``lambd_sync=False`` (default) keeps ``lambd`` on the device: no host read per forward, the step is HIP-graph
    capturable; a change of ``lambd`` that crosses a power-of-two n_fft boundary is followed by guard launches (see
    include/dmel.h), and one the guards do not cover (e.g. ``lambd`` rewritten by hand to a far value in the middle of a
    run: call ``resync()`` after that) yields NaN outputs and a RuntimeError at the next forward.  ``lambd_sync=True``
    reads ``lambd`` to the host at every forward like the reference (time_frequency.py:39).
    ``mfma="bf16x3"`` (with ``learnable_fb``): the dense contractions -- the forward through the trained matrix, the filterbank
    gradient's GEMM -- run on the bf16 matrix pipe as three split-bf16 products per fp32 product (~2e-5 relative, inside the 1e-4
    bar; default "fp32": exact).  ``save_spec=True`` (with ``learnable_fb``, default): the training forward keeps the power
    spectrogram for the filterbank gradient instead of recomputing it in the backward.

    forward(x: (B, n_points)) -> (B, 1, n_mels, n_points // hop_length + 1) float32.

    forward(x, lengths): zero-padded batches.  ``lengths`` is a (B,) integer tensor, ``1 <= lengths[b] <= n_points``; clip b is
    ``x[b, :lengths[b]]``.  Its first ``frame_lengths(lengths)[b]`` frames are what the reference layer returns for that clip alone at
    ``n_points = lengths[b]`` (the mean over the clip's own samples, the centred frames zero-padded past its end); the frames after
    them are pad frames with the value of a frame of zero mel power (0, or ``log(0 + eps)`` with ``log=True``) and no gradient, and
    their tiles cost no transform.  ``x[b, lengths[b]:]`` is never read.  The values are read by the kernels only (never by the host;
    a captured step sees what the tensor holds when it replays): a length outside ``1 ... n_points`` makes that clip's rows NaN (int64
    lengths are clamped on the device before they are narrowed to int32, so no value wraps into the valid range).  fp64 clips lose their
    own mean in fp64 before the cast to fp32, as ``forward(x)`` does.
    HTK bank with ``optimized=True`` only, clips that start at sample 0, and by default no waveform gradient.
    ``lengths_waveform_grad=True`` (keyword-only, off by default: such a forward keeps ``x``, ``lengths`` and the fp32 output alive until the
    backward) lets ``forward(x, lengths)`` take an ``x`` that requires grad.  The output and ``lambd.grad`` keep their bits;
    ``x.grad[b, :lengths[b]]`` is what autograd through the reference layer built with ``n_points = lengths[b]`` returns for that clip and
    the cotangent of its valid frames (so the gradient's own mean is taken over the clip's samples), ``x.grad[b, lengths[b]:]`` is ``+0.0``,
    the cotangent of pad frames is never read, and a length outside ``1 ... n_points`` makes the row ``x.grad[b]`` NaN.  With
    ``lambd_sync=False`` the step has no host read and can be captured.  A ``SlotInput`` carries no gradient (it is an address, not a
    tensor of the graph); ``learnable_fb`` and ``optimized=False`` refuse ``lengths`` with or without the flag.
    ``lengths_learnable_fb=True`` (keyword-only, off by default, needs ``learnable_fb=True``) makes ``forward(x, lengths)`` run through
    the trained ``mel_fb``: clip b is ``x[b, :lengths[b]]`` alone (its own mean, pad frames as above) contracted through the current
    matrix, with ``mfma="fp32"`` or ``"bf16x3"``, fp32 or bf16 output.  ``lambd.grad`` is the usual dot over the tangent (zero in pad
    frames); ``mel_fb.grad`` is ``sum_b sum_{t < frame_lengths(lengths)[b]} spec_b[f, t] * gm_b[m, t]`` with ``spec_b`` the spectrogram of
    the clip at its own length -- the cotangent, the saved output and the spectrogram are never loaded in pad frames, and an invalid
    length makes every element of ``mel_fb.grad`` NaN.  With every length at ``n_points`` the output and both gradients have the bits of
    ``forward(x)``.  No host read of ``lengths`` (nor, with ``lambd_sync=False``, of ``lambd``): the step can be captured, and a replay
    sees what ``lengths`` holds when it runs.  With ``lambd_sync=True`` the layer reads ``lambd`` and compares it with the bank's row
    count as ``forward(x)`` does, then issues the same device-checked launches with what that ``forward(x)`` uses: the exact contraction and a
    recomputed spectrogram.  There is no waveform gradient (``x.requires_grad`` raises), no ``SlotInput`` and no ``optimized=False``.
    """

    def __init__(self, init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None, hop_length=1,
                 device="cpu", optimized=False, normalize_window=False, *, log=False, eps=1e-10, learnable_fb=False,
                 out_dtype=torch.float32, lambd_sync=False, mfma="fp32", save_spec=True, lengths_waveform_grad=False,
                 lengths_learnable_fb=False):
        super().__init__()
        if lengths_learnable_fb and not learnable_fb:
            raise ValueError("lengths_learnable_fb=True is forward(x, lengths) through the trained filterbank: it needs learnable_fb=True")
        self.lengths_learnable_fb = bool(lengths_learnable_fb)        # forward(x, lengths) runs through mel_fb (opt-in: without it a trained
                                                                      # bank refuses lengths)
        self.lengths_waveform_grad = bool(lengths_waveform_grad)      # forward(x, lengths) accepts an x that requires grad (opt-in: that
                                                                      # forward keeps x, lengths and the fp32 output alive until the backward)
        if not torch.is_tensor(init_lambd):
            init_lambd = torch.tensor(float(init_lambd), dtype=torch.float32)
        if mfma not in ("fp32", "bf16x3"):
            raise ValueError("mfma must be 'fp32' (exact fp32 MFMA, the default) or 'bf16x3' (DMEL_FLAG_MFMA_BF16X3: three split-bf16 "
                             "products per fp32 product on the bf16 matrix pipe, for the DENSE contractions of a trainable filterbank)")
        self.mfma = mfma
        self.save_spec = bool(save_spec)      # trainable filterbank: the training forward also writes the (B, F, T) power spectrogram, so
                                              # that the filterbank gradient skips its recompute (16.8 MB per step at BASELINE config 2)
        self.hop_length = hop_length
        self.lambd = nn.Parameter(init_lambd)                        # models.py:19
        self.device = device
        self.optimized = optimized
        self.normalize_window = normalize_window
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else sample_rate // 2   # models.py:25
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self.n_freq = n_mels                                          # models.py:29
        self.n_time = n_points // hop_length + 1                      # models.py:30
        self.n_points = n_points
        self.log = bool(log)
        self.eps = float(eps)
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be torch.float32 (the reference's, models.py:36) or torch.bfloat16")
        self.out_dtype = out_dtype
        self.lambd_sync = bool(lambd_sync)
        if learnable_fb:
            n0 = capi.n_fft(float(init_lambd)) if optimized else 2 * n_points
            fb0 = capi.mel_fbanks_host(n0 // 2 + 1, float(self.f_min), float(self.f_max), n_mels, sample_rate)   # models.py:42-48
            self.mel_fb = nn.Parameter(torch.from_numpy(fb0))
        else:
            self.mel_fb = None

    # -- plumbing -----------------------------------------------------------------------------
    def plan_info(self, device=None) -> dict:
        return self._plan_on(device).info()

    def _lambd_host(self) -> float:
        """Host value of lambd: a device->host read (the reference does one per sample, time_frequency.py:39).  Never
        cached: writes through ``lambd.data`` leave no trace torch could be asked about."""
        return float(self.lambd.detach())

    def n_fft(self) -> int:
        """n_fft the next forward will use: next_pow2(int(6*|lambd|)) (time_frequency.py:39,60-65), or 2*n_points
        in the optimized=False branch (time_frequency.py:51).  Reads lambd to the host."""
        return capi.n_fft(self._lambd_host()) if self.optimized else 2 * self.n_points

    def lambd_status(self, device=None) -> dict:
        """What the kernels last reported (no synchronisation): see dmel_lambd_status in include/dmel.h."""
        return self._plan_on(device).lambd_status()

    def frame_lengths(self, lengths: torch.Tensor) -> torch.Tensor:
        """Valid frames per clip of ``forward(x, lengths)``: ``lengths // hop_length + 1`` (models.py:30 at ``n_points = lengths[b]``),
        on the tensor's own device."""
        return _frame_lengths(lengths, self.hop_length)

    def _slot_config_ok(self) -> bool:
        return self.mel_fb is None and self.optimized and not self.lambd_sync

    def _sync_filterbank(self, plan, n, x):
        """The plan's tables for n_fft ``n`` are refreshed from the parameter's storage by one small kernel on the current stream at
        every forward (no host copy, no synchronisation: the matrix changes at every optimizer step, and writes through .data leave no
        trace to ask torch about)."""
        fb = self.mel_fb
        if fb.device != x.device:
            raise RuntimeError(f"mel_fb is on {fb.device} but x is on {x.device}; call layer.to(x.device)")
        fbd = fb.detach()
        if fbd.dtype != torch.float32 or not fbd.is_contiguous():
            fbd = fbd.to(torch.float32).contiguous()
        with _on_device(x.device):
            plan.set_filterbank_dev(n, fbd.data_ptr(), _stream_ptr(x.device))

    def _check_lengths(self, x, lengths):
        """Whether this layer takes per-clip lengths, then shape, dtype and device of ``lengths`` (_lengths_for_kernels); returns them as the
        kernels read them (int32, contiguous, on x's device).  Their values never leave the device."""
        want_x = self.lengths_waveform_grad and torch.is_grad_enabled() and not isinstance(x, SlotInput) and x.requires_grad
        if self.mel_fb is not None and not self.lengths_learnable_fb:
            raise RuntimeError("per-clip lengths run the HTK bank only: learnable_fb=True does not take lengths"
                               + (" (and has no waveform gradient with them)" if want_x else ""))
        if not self.optimized:
            raise RuntimeError("per-clip lengths need optimized=True (the optimized=False branch's n_fft = 2 n_points depends on the clip length)"
                               + ("; the waveform gradient of per-clip lengths needs it too" if want_x else ""))
        return _lengths_for_kernels(x, lengths, self.n_points)

    # -- forward ------------------------------------------------------------------------------
    def _forward_lengths(self, x, lengths):
        """forward(x, lengths), both checked: torch.ops.dmel.mel_spectrogram_lengths (the hot path's C++ autograd node over
        dmel_forward_dev_lengths, or dmel_forward_lengths with lambd_sync).  With ``lengths_waveform_grad=True`` an ``x`` that requires
        grad takes _DmelLenXFunction instead: the same launches, and a backward to the waveform."""
        if self.mel_fb is not None:
            return self._forward_lengths_fb(x, lengths)
        flags = capi.DMEL_FLAG_LOG if self.log else 0
        bf16 = self.out_dtype == torch.bfloat16
        plan, lam = self._plan_for(x.device), _lambd_for_op(self.lambd)
        if isinstance(x, SlotInput):
            return _len_op()(x.view(), lengths, lam, plan.handle, flags | capi.DMEL_FLAG_X_INDIRECT, self.eps, False, bf16)
        xf = _as_f32_contiguous(x, lengths)
        if xf.requires_grad and torch.is_grad_enabled():
            # lengths_waveform_grad=True: the gradient flows back through the conversions above (the fp64 path's masked mean included)
            return _DmelLenXFunction.apply(xf, lengths, self.lambd, plan, self._lambd_host() if self.lambd_sync else None, self.log, self.eps,
                                           self.out_dtype)
        return _len_op()(xf, lengths, lam, plan.handle, flags, self.eps, self.lambd_sync, bf16)

    def _forward_lengths_fb(self, x, lengths):
        """forward(x, lengths) through the trained filterbank (lengths_learnable_fb=True), both checked: _DmelFbDevFunction with lengths.
        The bank's row count fixes n_fft; lambd is read and checked against it on the device (one that has left it gives NaN now and
        "tied to one n_fft" at the next forward).  lambd_sync: the layer reads lambd and compares first, as forward(x) does, and keeps that
        path's arithmetic (exact contraction, spectrogram recomputed in the backward)."""
        fb, plan = self.mel_fb, self._plan_for(x.device)
        n = 2 * (fb.shape[0] - 1)
        if self.lambd_sync:
            lam_host = self._lambd_host()
            if fb.shape[0] != capi.n_fft(lam_host) // 2 + 1:
                raise RuntimeError(f"mel_fb was built for n_fft={n} but lambd={lam_host} now gives n_fft={capi.n_fft(lam_host)}; "
                                   "a learnable filterbank is tied to one n_fft")
        xf = _as_f32_contiguous(x, lengths)
        self._sync_filterbank(plan, n, x)
        bf16x3 = self.mfma == "bf16x3" and not self.lambd_sync
        return _DmelFbDevFunction.apply(xf, self.lambd, plan, n, self.log, self.eps, fb, self.out_dtype, False,
                                        capi.DMEL_FLAG_MFMA_BF16X3 if bf16x3 else 0, self.save_spec and not self.lambd_sync, lengths)

    def forward(self, x, lengths=None):
        no_x_grad = None if lengths is None or self.lengths_waveform_grad else "per-clip lengths have no waveform gradient: pass x.detach()"
        if lengths is not None and self.mel_fb is not None and self.lengths_learnable_fb:
            no_x_grad = "learnable_fb with per-clip lengths has no waveform gradient: pass x.detach()"
        lam = self.lambd                # (read once: a parameter is found through nn.Module.__getattr__, a quarter of a microsecond)
        lengths = _check_input("MelSpectrogramLayer", x, lam, lengths, n_points=self.n_points, check_lengths=self._check_lengths,
                               slot_config_ok=self._slot_config_ok, refuse_x_grad=no_x_grad)
        if lengths is not None:
            return self._forward_lengths(x, lengths)
        plan = self._plan_for(x.device)
        if isinstance(x, SlotInput):
            flags = (capi.DMEL_FLAG_LOG if self.log else 0) | capi.DMEL_FLAG_X_INDIRECT
            return _mel_op()(x.view(), _lambd_for_op(lam), plan.handle, flags, self.eps, False, self.out_dtype == torch.bfloat16)
        xf = _as_f32_contiguous(x)
        fb = self.mel_fb
        if fb is None and not x.requires_grad:
            # the hot path: torch-registered op, C++ autograd node, lambd read on the device unless lambd_sync
            flags = (capi.DMEL_FLAG_LOG if self.log else 0) | (0 if self.optimized else capi.DMEL_FLAG_FULL_WINDOW)
            return _mel_op()(xf, _lambd_for_op(lam), plan.handle, flags, self.eps, self.lambd_sync, self.out_dtype == torch.bfloat16)
        if not self.lambd_sync:
            # sync-free: a trainable filterbank fixes n_fft (its row count; lambd is read and checked on the device: one that has left
            # that n_fft gives NaN now and a RuntimeError at the next forward, as models.py:53 fails on the shape), the optimized=False
            # branch runs n_fft = 2 n_points whatever lambd is, and the HTK bank with optimized=True and x.requires_grad (n = 0) runs the
            # tracked forward and a backward that issues the waveform gradient for every n_fft that forward launched for.
            # (What reads lambd to the host: lambd_sync=True, and the waveform gradient at n_fft >= 16384.)
            full = not self.optimized
            n = 2 * self.n_points if full else (2 * (fb.shape[0] - 1) if fb is not None else 0)
            if fb is not None:
                if fb.shape[0] != n // 2 + 1:
                    raise RuntimeError(f"mel_fb was built for n_fft={2 * (fb.shape[0] - 1)} but this layer runs n_fft={n}; "
                                       "a learnable filterbank is tied to one n_fft")
                self._sync_filterbank(plan, n, x)
            return _DmelFbDevFunction.apply(xf, lam, plan, n, self.log, self.eps, fb, self.out_dtype, full,
                                            capi.DMEL_FLAG_MFMA_BF16X3 if self.mfma == "bf16x3" else 0, self.save_spec)
        lam_host = self._lambd_host()
        if fb is not None:
            n = capi.n_fft(lam_host) if self.optimized else 2 * self.n_points
            if fb.shape[0] != n // 2 + 1:
                raise RuntimeError(f"mel_fb was built for n_fft={2 * (fb.shape[0] - 1)} but lambd={lam_host} now gives n_fft={n}; "
                                   "a learnable filterbank is tied to one n_fft")
            self._sync_filterbank(plan, n, x)
        return _DmelFunction.apply(xf, lam, plan, lam_host, self.log, self.eps, not self.optimized, fb, self.out_dtype)

    def extra_repr(self):
        return (f"n_mels={self.n_mels}, n_points={self.n_points}, sample_rate={self.sample_rate}, "
                f"hop_length={self.hop_length}, f_min={self.f_min}, f_max={self.f_max}, "
                f"normalize_window={self.normalize_window}, log={self.log}"
                + (", lengths_learnable_fb=True" if self.lengths_learnable_fb else ""))


class _MultiFunction(torch.autograd.Function):
    """forward: dmel_forward_multi(_dev) -- one launch per distinct n_fft for all K channels, carrying d out / d lambd[k] per channel;
    backward: dmel_backward_multi (K dot products in one launch) and, for a waveform that requires grad (waveform_grad=True),
    dmel_backward_x_multi(_dev): one x-gradient for all K channels, the sum of the K scalar layers' in ascending channel order.
    With ``lengths`` (per_clip_lengths=True; int32 on x's device) the forward is dmel_forward_multi(_dev)_lengths; the backward is the same
    dot over its tangent, whose pad frames are zero, and for a waveform that requires grad (lengths_waveform_grad=True)
    dmel_backward_x_multi(_dev)_lengths: ``lengths`` is then saved too."""

    @staticmethod
    def forward(ctx, x, lambd, plan, lam_host, log, eps, out_dtype, want_tangent, lengths=None):
        B, K = x.shape[0], lambd.shape[0]
        want_x = ctx.needs_input_grad[0]
        out, tangent, scratch, round_later = _alloc(x, (B, K, plan.n_mels, plan.n_time), out_dtype, want_tangent, log and want_x,
                                                    plan.scratch_bytes_multi(B, K))
        bf16 = out.dtype == torch.bfloat16
        lam = None
        with _on_device(x.device):
            if lam_host is not None:
                plan.forward_multi(x.data_ptr(), B, lam_host, out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                                   scratch.data_ptr(), out_bf16=bf16, lengths_ptr=_ptr(lengths))
            else:
                lam = _lambd_f32(lambd)
                plan.forward_multi_dev(x.data_ptr(), B, lam.data_ptr(), K, out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                                       scratch.data_ptr(), out_bf16=bf16, lengths_ptr=_ptr(lengths))
        ctx.plan, ctx.K, ctx.lambd_shape, ctx.lambd_dtype = plan, K, lambd.shape, lambd.dtype
        ctx.want_tangent, ctx.want_x, ctx.log, ctx.lam_host = want_tangent, want_x, bool(log), lam_host
        # what this forward launched for (host bookkeeping of the plan, no device read): a later forward cannot change what the backward covers
        ctx.launches = plan.last_multi_launch() if (want_x and lam_host is None) else None
        saved = [tangent, scratch] if want_tangent else []
        if want_x:
            saved += [x] + ([lengths] if lengths is not None else []) + ([lam] if lam is not None else []) + ([out] if log else [])
        ctx.has_lengths = lengths is not None
        ctx.save_for_backward(*saved)
        return out.to(torch.bfloat16) if round_later else out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        g, bf16 = _cotangent(grad_out)
        dl = gx = None
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent, scratch = saved.pop(0), saved.pop(0)
                dl = torch.empty((ctx.K,), dtype=torch.float32, device=g.device)
                ctx.plan.backward_multi(g.data_ptr(), tangent.data_ptr(), g.shape[0], ctx.K, dl.data_ptr(), _stream_ptr(g.device),
                                        scratch.data_ptr(), grad_bf16=bf16)
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
            if ctx.want_x:
                x = saved.pop(0)
                lengths = saved.pop(0) if ctx.has_lengths else None
                lam = saved.pop(0) if ctx.lam_host is None else None
                out = saved.pop(0) if ctx.log else None
                g32 = g.to(torch.float32)
                gx = torch.empty_like(x)
                if lam is None:
                    ctx.plan.backward_x_multi(x.data_ptr(), x.shape[0], ctx.lam_host, g32.data_ptr(), _ptr(out), gx.data_ptr(), ctx.log,
                                              _stream_ptr(g.device), lengths_ptr=_ptr(lengths))
                else:
                    ctx.plan.backward_x_multi_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), ctx.K, ctx.launches, g32.data_ptr(), _ptr(out),
                                                  gx.data_ptr(), ctx.log, _stream_ptr(g.device), lengths_ptr=_ptr(lengths))
        return gx, dl, None, None, None, None, None, None, None


class MultiWindowMelSpectrogram(_PlanCachingModule):
    """K trainable window widths at once, returned as K output channels.

        MultiWindowMelSpectrogram(init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None, hop_length=1,
                                  normalize_window=False, *, log=False, eps=1e-10, out_dtype=torch.float32, lambd_sync=False,
                                  waveform_grad=False, per_clip_lengths=False, lengths_waveform_grad=False)
        forward(x: (B, n_points)) -> (B, K, n_mels, n_points // hop_length + 1)

    ``y[:, k:k+1]`` is what ``MelSpectrogramLayer(lambd[k], ..., optimized=True)`` returns for the same ``x``, bit for bit (each
    channel has its own n_fft = next_pow2(int(6 |lambd[k]|)) and HTK bank), and ``lambd.grad[k]`` is that channel's gradient.  The
    parameter ``lambd`` has shape ``(K,)``, 1 <= K <= 8; every channel's n_fft must lie in 32 ... 16384 (about 2.84 <= |lambd| <= 2730).
    A channel whose lambd leaves that range (or moves further than the sync-free forward covers) is NaN and the next forward raises.
    The kernels launch once per distinct n_fft for all the channels that need it; the backward is one launch for all K gradients.
    ``waveform_grad=True`` accepts an ``x`` that requires grad: ``x.grad`` is, bit for bit, the sum in ascending channel order of what the K
    scalar layers give (one x-gradient launch per distinct n_fft and one combine for all channels).  The forward then keeps ``x`` and the
    fp32 output alive until the backward, which the default layer does not; without it ``x.requires_grad`` raises.
    ``per_clip_lengths=True`` (keyword-only, off by default: without it ``lengths`` is refused) makes ``forward(x, lengths)`` compute a
    zero-padded batch clip by clip: ``lengths`` as ``MelSpectrogramLayer.forward(x, lengths)`` takes them (a (B,) int32 / int64 tensor, read by
    the kernels only, so the sync-free step stays capturable), and ``y[:, k:k+1]`` is what that scalar forward returns at ``lambd[k]``, bit for
    bit -- each clip's own mean, pad frames (``0`` or ``log(0 + eps)``, no gradient) from ``frame_lengths(lengths)[b]`` on, tiles of pad
    frames not transformed, ``x[b, lengths[b]:]`` never read, a length outside ``1 ... n_points`` NaN in every channel of that clip.
    ``lambd.grad`` comes through the same backward.  ``forward(x)`` is unchanged.
    ``lengths_waveform_grad=True`` (keyword-only, off by default, needs ``per_clip_lengths=True``; the name and meaning are
    ``MelSpectrogramLayer``'s) lets ``forward(x, lengths)`` take an ``x`` that requires grad; ``waveform_grad`` keeps governing ``forward(x)``
    only.  The output and ``lambd.grad`` keep their bits and ``x.grad`` is ``0 + gx_0 + ... + gx_{K-1}`` in ascending channel order, ``gx_k``
    the ``x.grad`` of ``MelSpectrogramLayer(lambd[k], ..., optimized=True, lengths_waveform_grad=True)(x, lengths)`` for ``g[:, k:k+1]``, bit
    for bit: ``x.grad[b, lengths[b]:]`` is ``+0.0``, the gradient's own mean is taken over the clip's samples, the cotangent of pad frames is
    never read, and a length outside ``1 ... n_points`` makes the row ``x.grad[b]`` NaN.  With ``lambd_sync=False`` the step has no host read
    and can be captured; a channel no launch covered makes all of ``x.grad`` NaN.  Without the flag ``x.requires_grad`` together with
    ``lengths`` raises, with or without ``waveform_grad``.
    Not supported: ``SlotInput``, ``GraphedStep`` and ``LambdAdam(fused_into_backward=...)``."""

    MAX_CHANNELS = 8

    def __init__(self, init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None, hop_length=1, normalize_window=False, *,
                 log=False, eps=1e-10, out_dtype=torch.float32, lambd_sync=False, waveform_grad=False, per_clip_lengths=False,
                 lengths_waveform_grad=False):
        super().__init__()
        if lengths_waveform_grad and not per_clip_lengths:
            raise ValueError("lengths_waveform_grad=True is the waveform gradient of forward(x, lengths): it needs per_clip_lengths=True")
        lam = init_lambd.detach().clone() if torch.is_tensor(init_lambd) else torch.tensor([float(v) for v in init_lambd])
        if lam.dim() != 1:
            raise ValueError(f"init_lambd must be 1-D (K values), got shape {tuple(lam.shape)}")
        K = lam.shape[0]
        if not 1 <= K <= self.MAX_CHANNELS:
            raise ValueError(f"the multi-window layer has 1 ... {self.MAX_CHANNELS} channels, got K = {K}")
        lam = lam.to(torch.float32)
        for k, v in enumerate(lam.tolist()):
            n = capi.n_fft(v) if v == v else 0
            if not capi.MIN_FAST_NFFT <= n <= capi.MAX_NFFT:
                raise ValueError(f"init_lambd[{k}] = {v} gives n_fft {n}: the multi-window layer serves n_fft {capi.MIN_FAST_NFFT} ... "
                                 f"{capi.MAX_NFFT} (about 2.84 <= |lambd| <= 2730)")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be torch.float32 or torch.bfloat16")
        self.lambd = nn.Parameter(lam)
        self.n_mels, self.n_points, self.sample_rate, self.hop_length = n_mels, n_points, sample_rate, hop_length
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else sample_rate // 2
        self.normalize_window = normalize_window
        self.n_time = n_points // hop_length + 1
        self.log, self.eps, self.out_dtype, self.lambd_sync = bool(log), float(eps), out_dtype, bool(lambd_sync)
        self.waveform_grad = bool(waveform_grad)
        self.per_clip_lengths = bool(per_clip_lengths)                # forward(x, lengths) is taken (opt-in: without it lengths are refused)
        self.lengths_waveform_grad = bool(lengths_waveform_grad)      # ... and accepts an x that requires grad (opt-in: that forward keeps
                                                                      # x, lengths and the fp32 output alive until the backward)

    @property
    def channels(self) -> int:
        return self.lambd.shape[0]

    def lambd_status(self, channel: int = 0, device=None) -> dict:
        return self._plan_on(device).lambd_status_channel(channel)

    def frame_lengths(self, lengths: torch.Tensor) -> torch.Tensor:
        """Valid frames per clip of ``forward(x, lengths)``: ``lengths // hop_length + 1``, as MelSpectrogramLayer.frame_lengths."""
        return _frame_lengths(lengths, self.hop_length)

    def _prepare(self, name, x, lengths, refuse_slot, refuse_x_grad):
        """the checks and conversions the K-channel forwards share: (x as fp32, lambd's host values or None, whether to carry the tangent,
        the lengths as the kernels read them or None)"""
        check = None
        if self.per_clip_lengths:
            check = lambda x_, l_: _lengths_for_kernels(x_, l_, self.n_points)      # noqa: E731
            if lengths is not None:                                                # (waveform_grad governs forward(x) only)
                refuse_x_grad = None
                if not self.lengths_waveform_grad:
                    refuse_x_grad = (f"per-clip lengths have no waveform gradient on {name} yet: pass x.detach() "
                                     "(MelSpectrogramLayer(lengths_waveform_grad=True) has one)")
        lengths = _check_input(name, x, self.lambd, lengths, n_points=self.n_points, check_lengths=check, refuse_slot=refuse_slot,
                               refuse_x_grad=refuse_x_grad)
        xf = _as_f32_contiguous(x, lengths)
        lam_host = [float(v) for v in self.lambd.detach().cpu().tolist()] if self.lambd_sync else None
        # the tangent only when a gradient will be asked for (as torch.ops.dmel.mel_spectrogram: grad mode and lambd.requires_grad);
        # otherwise the inference kernels, which pair two frames per FFT
        return xf, lam_host, torch.is_grad_enabled() and self.lambd.requires_grad, lengths

    def forward(self, x, lengths=None):
        no_x_grad = None if self.waveform_grad else ("MultiWindowMelSpectrogram has no waveform gradient by default: pass waveform_grad=True, "
                                                     "or x.detach()")
        xf, lam_host, want, lengths = self._prepare("MultiWindowMelSpectrogram", x, lengths, "MultiWindowMelSpectrogram does not take a SlotInput",
                                                    no_x_grad)
        return _MultiFunction.apply(xf, self.lambd, self._plan_for(x.device), lam_host, self.log, self.eps, self.out_dtype, want, lengths)

    def extra_repr(self):
        return (f"channels={self.channels}, n_mels={self.n_mels}, n_points={self.n_points}, sample_rate={self.sample_rate}, "
                f"hop_length={self.hop_length}, f_min={self.f_min}, f_max={self.f_max}, normalize_window={self.normalize_window}, log={self.log}, "
                f"waveform_grad={self.waveform_grad}, per_clip_lengths={self.per_clip_lengths}, "
                f"lengths_waveform_grad={self.lengths_waveform_grad}")


class _BandFunction(torch.autograd.Function):
    """forward: dmel_forward_band(_dev) -- one launch per distinct n_fft for all K channels, every channel writing its own rows of ONE
    (B, 1, M, T) image and of its tangent; backward: dmel_backward_band (the K row-group dot products in one launch) and, for a waveform
    that requires grad (waveform_grad=True), dmel_backward_x_band(_dev): every channel's x-gradient from its own rows of the ONE cotangent,
    summed in ascending channel order (what _MultiFunction saves for it, this one saves too).  With ``lengths``:
    dmel_forward_band(_dev)_lengths and, for the waveform, dmel_backward_x_band(_dev)_lengths, as _MultiFunction."""

    @staticmethod
    def forward(ctx, x, lambd, plan, lam_host, edges, log, eps, out_dtype, want_tangent, lengths=None):
        B, K = x.shape[0], lambd.shape[0]
        want_x = ctx.needs_input_grad[0]
        out, tangent, scratch, round_later = _alloc(x, (B, 1, plan.n_mels, plan.n_time), out_dtype, want_tangent, log and want_x,
                                                    plan.scratch_bytes_multi(B, K))
        bf16 = out.dtype == torch.bfloat16
        lam = None
        with _on_device(x.device):
            if lam_host is not None:
                plan.forward_band(x.data_ptr(), B, lam_host, edges, out.data_ptr(), _ptr(tangent), log, eps, _stream_ptr(x.device),
                                  scratch.data_ptr(), out_bf16=bf16, lengths_ptr=_ptr(lengths))
            else:
                lam = _lambd_f32(lambd)
                plan.forward_band_dev(x.data_ptr(), B, lam.data_ptr(), edges, out.data_ptr(), _ptr(tangent), log, eps,
                                      _stream_ptr(x.device), scratch.data_ptr(), out_bf16=bf16, lengths_ptr=_ptr(lengths))
        ctx.plan, ctx.lambd_shape, ctx.lambd_dtype, ctx.edges, ctx.want_tangent = plan, lambd.shape, lambd.dtype, edges, want_tangent
        ctx.want_x, ctx.log, ctx.lam_host = want_x, bool(log), lam_host
        # what this forward launched for (host bookkeeping of the plan, no device read): a later forward cannot change what the backward covers
        ctx.launches = plan.last_multi_launch() if (want_x and lam_host is None) else None
        saved = [tangent, scratch] if want_tangent else []
        if want_x:
            saved += [x] + ([lengths] if lengths is not None else []) + ([lam] if lam is not None else []) + ([out] if log else [])
        ctx.has_lengths = lengths is not None
        ctx.save_for_backward(*saved)
        return out.to(torch.bfloat16) if round_later else out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        g, bf16 = _cotangent(grad_out)
        dl = gx = None
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent, scratch = saved.pop(0), saved.pop(0)
                dl = torch.empty((len(ctx.edges) - 1,), dtype=torch.float32, device=g.device)
                ctx.plan.backward_band(g.data_ptr(), tangent.data_ptr(), g.shape[0], ctx.edges, dl.data_ptr(), _stream_ptr(g.device),
                                       scratch.data_ptr(), grad_bf16=bf16)
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
            if ctx.want_x:
                x = saved.pop(0)
                lengths = saved.pop(0) if ctx.has_lengths else None
                lam = saved.pop(0) if ctx.lam_host is None else None
                out = saved.pop(0) if ctx.log else None
                g32 = g.to(torch.float32)
                gx = torch.empty_like(x)
                if lam is None:
                    ctx.plan.backward_x_band(x.data_ptr(), x.shape[0], ctx.lam_host, ctx.edges, g32.data_ptr(), _ptr(out), gx.data_ptr(), ctx.log,
                                             _stream_ptr(g.device), lengths_ptr=_ptr(lengths))
                else:
                    ctx.plan.backward_x_band_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), ctx.edges, ctx.launches, g32.data_ptr(), _ptr(out),
                                                 gx.data_ptr(), ctx.log, _stream_ptr(g.device), lengths_ptr=_ptr(lengths))
        return gx, dl, None, None, None, None, None, None, None, None


class BandSplitMelSpectrogram(MultiWindowMelSpectrogram):
    """A trainable window width per GROUP OF MEL BANDS inside one image: the scalar layer's output shape, K resolutions.

        BandSplitMelSpectrogram(init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None, hop_length=1, normalize_window=False, *,
                                band_edges=None, log=False, eps=1e-10, out_dtype=torch.float32, lambd_sync=False, waveform_grad=False,
                                per_clip_lengths=False, lengths_waveform_grad=False)
        forward(x: (B, n_points)) -> (B, 1, n_mels, n_points // hop_length + 1)

    ``band_edges`` are K + 1 integers ``0 = e_0 < e_1 < ... < e_K = n_mels`` (default ``e_k = (k * n_mels) // K``).  Rows
    ``e_k ... e_{k+1} - 1`` of the image are those rows of what ``MelSpectrogramLayer(lambd[k], ..., optimized=True)`` returns for the
    same ``x``, bit for bit (fp32 and bf16, training and ``torch.no_grad()`` kernels): each group has its own n_fft =
    next_pow2(int(6 |lambd[k]|)) and the HTK bank of THAT n_fft, and ``lambd.grad[k]`` sums ``grad_out * d out / d lambd[k]`` over the
    group's rows.  The rows of the other channels are never computed into memory.  The parameter is ``lambd`` of shape ``(K,)``,
    1 <= K <= 8, every n_fft in 32 ... 16384, so the layer drops into the nets of ``nets.py`` / ``panns.py``
    (``net.spectrogram_layer = BandSplitMelSpectrogram(...)``) and ``nets.make_optimizer`` puts it in the ``lr_tf`` group as it is.

    The intended order is WIDE windows for the LOW bands: a mel band narrower than one bin of its group's n_fft is an all-zero row of
    that HTK bank, as in the scalar layer (value ``0`` / ``log(eps)``, gradient exactly 0), which is what a short window on low bands gives.

    ``band_edges`` is a plain attribute reconstructed from the constructor; it is NOT part of ``state_dict`` (whose only key stays
    ``lambd``, as the scalar layer's checkpoints): build the layer with the same edges before loading.

    ``lambd_sync=False`` keeps the K values on the device with one host picture per channel exactly as the multi-window layer
    (``resync()``, ``lambd_status(channel)``, ``set_tracking``); a channel no launch covered makes ITS rows NaN, leaves the other
    groups' rows untouched, and the next forward raises naming the channel.  The sync-free step can be captured with ``torch.cuda.graph``.

    ``waveform_grad=True`` accepts an ``x`` that requires grad.  With ``G_k`` the cotangent whose rows outside ``e_k ... e_{k+1} - 1`` are
    ``+0.0``, ``x.grad`` is ``0 + gx_0 + ... + gx_{K-1}`` in ascending channel order, ``gx_k`` what
    ``MelSpectrogramLayer(lambd[k], ..., optimized=True)`` gives for ``G_k``, bit for bit -- ``MultiWindowMelSpectrogram(waveform_grad=True)``'s
    ``x.grad`` for the stacked ``G_k`` without the ``(B, K, M, T)`` tensors: every channel loads only its own rows of the one cotangent.
    The forward output and ``lambd.grad`` do not change; the forward then keeps ``x`` and the fp32 output alive until the backward.  A
    channel no launch covered makes ``x.grad`` NaN.  Without the flag ``x.requires_grad`` raises.
    ``per_clip_lengths=True`` (keyword-only, off by default: without it ``lengths`` is refused) makes ``forward(x, lengths)`` compute a
    zero-padded batch clip by clip, as ``MelSpectrogramLayer.forward(x, lengths)`` does and with its ``lengths``: rows
    ``e_k ... e_{k+1} - 1`` are those rows of that scalar forward at ``lambd[k]``, bit for bit (each clip's own mean, pad frames of value
    ``0`` / ``log(0 + eps)`` and no gradient from ``frame_lengths(lengths)[b]`` on, pad tiles not transformed, ``x[b, lengths[b]:]`` never
    read, a length outside ``1 ... n_points`` NaN in every group's rows of that clip); a channel writes pad and NaN rows into its own rows
    only.  The values are read by the kernels only: the sync-free step stays capturable.  ``forward(x)`` is unchanged.
    ``lengths_waveform_grad=True`` (keyword-only, off by default, needs ``per_clip_lengths=True``) lets ``forward(x, lengths)`` take an ``x``
    that requires grad, as on ``MultiWindowMelSpectrogram``: ``x.grad`` is the same sum with ``gx_k`` the ``x.grad`` of
    ``MelSpectrogramLayer(lambd[k], ..., optimized=True, lengths_waveform_grad=True)(x, lengths)`` for ``G_k``, bit for bit; a channel loads
    only its own rows of the cotangent and of the saved log output, and only the clip's own frames of them.  Without the flag
    ``x.requires_grad`` together with ``lengths`` raises, with or without ``waveform_grad``.
    Out of scope, not forgotten (each raises and says what to use instead): ``SlotInput``, ``GraphedStep`` and
    ``LambdAdam(fused_into_backward=...)``; band edges and the filterbank are not trainable."""

    def __init__(self, init_lambd, n_mels, n_points, sample_rate, f_min=0, f_max=None, hop_length=1, normalize_window=False, *,
                 band_edges=None, log=False, eps=1e-10, out_dtype=torch.float32, lambd_sync=False, waveform_grad=False,
                 per_clip_lengths=False, lengths_waveform_grad=False):
        super().__init__(init_lambd, n_mels, n_points, sample_rate, f_min, f_max, hop_length, normalize_window, log=log, eps=eps,
                         out_dtype=out_dtype, lambd_sync=lambd_sync, waveform_grad=waveform_grad, per_clip_lengths=per_clip_lengths,
                         lengths_waveform_grad=lengths_waveform_grad)
        K = self.lambd.shape[0]
        if band_edges is None:
            if K > n_mels:
                raise ValueError(f"{K} groups need at least {K} mel bands, got n_mels = {n_mels}")
            edges = [(k * n_mels) // K for k in range(K + 1)]
        else:
            raw = band_edges.tolist() if torch.is_tensor(band_edges) else list(band_edges)
            if any(int(v) != v for v in raw):
                raise ValueError(f"band_edges must be integers, got {raw}")
            edges = [int(v) for v in raw]
        if len(edges) != K + 1:
            raise ValueError(f"band_edges needs K + 1 = {K + 1} entries for {K} window widths, got {len(edges)}")
        if edges[0] != 0 or edges[-1] != n_mels or any(b <= a for a, b in zip(edges, edges[1:])):
            raise ValueError(f"band_edges must be 0 = e_0 < e_1 < ... < e_K = n_mels = {n_mels} (every group non-empty), got {edges}")
        self.band_edges = tuple(edges)

    def forward(self, x, lengths=None):
        no_x_grad = None if self.waveform_grad else ("BandSplitMelSpectrogram has no waveform gradient: pass x.detach() (MelSpectrogramLayer and "
                                                     "MultiWindowMelSpectrogram(waveform_grad=True) have one)")
        xf, lam_host, want, lengths = self._prepare("BandSplitMelSpectrogram", x, lengths,
                                                    "BandSplitMelSpectrogram does not take a SlotInput: pass the batch tensor (MelSpectrogramLayer takes slots)",
                                                    no_x_grad)
        return _BandFunction.apply(xf, self.lambd, self._plan_for(x.device), lam_host, self.band_edges, self.log, self.eps, self.out_dtype, want,
                                   lengths)

    def extra_repr(self):
        return (f"band_edges={list(self.band_edges)}, n_mels={self.n_mels}, n_points={self.n_points}, sample_rate={self.sample_rate}, "
                f"hop_length={self.hop_length}, f_min={self.f_min}, f_max={self.f_max}, normalize_window={self.normalize_window}, log={self.log}, "
                f"waveform_grad={self.waveform_grad}, per_clip_lengths={self.per_clip_lengths}, "
                f"lengths_waveform_grad={self.lengths_waveform_grad}")


class _DspecFunction(torch.autograd.Function):
    """forward: dmel_spectrogram_ex (carries d spec / d lambd); backward: dmel_backward and, for a waveform that requires grad,
    dmel_backward_x_spec."""

    @staticmethod
    def forward(ctx, x, lambd, plan, lam_host, n_fft, half_window):
        """lam_host None: lambd is read by the kernels from the parameter's storage (no host read: capturable)"""
        B = x.shape[0]
        want_tangent = ctx.needs_input_grad[1]
        out, tangent, _, _ = _alloc(x, (B, 1, n_fft // 2 + 1, plan.n_time), torch.float32, want_tangent)
        lam = _lambd_f32(lambd) if lam_host is None else None
        with _on_device(x.device):
            if lam is None:
                plan.spectrogram_ex(x.data_ptr(), B, lam_host, n_fft, out.data_ptr(), _ptr(tangent), _stream_ptr(x.device), remove_dc=True,
                                    half_window=half_window)
            else:
                plan.spectrogram_ex_dev(x.data_ptr(), B, lam.data_ptr(), n_fft, out.data_ptr(), _ptr(tangent), _stream_ptr(x.device),
                                        remove_dc=True, half_window=half_window)
        ctx.plan, ctx.lambd_shape, ctx.lambd_dtype = plan, lambd.shape, lambd.dtype
        ctx.want_tangent, ctx.want_x = want_tangent, ctx.needs_input_grad[0]
        ctx.args = (lam_host, n_fft, half_window)
        saved = ([tangent] if want_tangent else []) + ([x] if ctx.want_x else []) + ([lam] if (ctx.want_x and lam is not None) else [])
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        g = _cotangent(grad_out)[0].to(torch.float32)            # the spectrogram is fp32 only
        dl = gx = None
        with _on_device(g.device):
            if ctx.want_tangent:
                tangent = saved.pop(0)
                dl = torch.empty((1,), dtype=torch.float32, device=g.device)
                ctx.plan.backward(g.data_ptr(), tangent.data_ptr(), g.numel(), dl.data_ptr(), _stream_ptr(g.device))
                dl = _dl_like(dl, ctx.lambd_shape, ctx.lambd_dtype)
            if ctx.want_x:
                x = saved.pop(0)
                lam_host, n_fft, half_window = ctx.args
                gx = torch.empty_like(x)
                if lam_host is None:
                    lam = saved.pop(0)
                    ctx.plan.backward_x_spec_dev(x.data_ptr(), x.shape[0], lam.data_ptr(), n_fft, g.data_ptr(), gx.data_ptr(),
                                                 _stream_ptr(g.device), half_window=half_window)
                else:
                    ctx.plan.backward_x_spec(x.data_ptr(), x.shape[0], lam_host, n_fft, g.data_ptr(), gx.data_ptr(), _stream_ptr(g.device),
                                             half_window=half_window)
        return gx, dl, None, None, None, None


class SpectrogramLayer(_PlanCache):
    """DSPEC: differentiable spectrogram with a trainable Gaussian window width.

    Signature-compatible with the reference (models.py:171-200):
        SpectrogramLayer(init_lambd, device='cpu', optimized=False, size=(512, 1024), hop_length=1, normalize_window=False)
    ``optimized=False``: window = whole signal, n_fft = 2*n_points (time_frequency.py:41,51), output
    ``(B, 1, n_points + 1, n_points // hop_length + 1)``; any n_points (a length that is not a power of two takes the
    chirp-z path of csrc/dmel_big.hip).
    ``optimized=True``: n_fft = next_pow2(int(6*|lambd|)) and the output must have the shape ``size``.
    """

    def __init__(self, init_lambd, device="cpu", optimized=False, size=(512, 1024), hop_length=1, normalize_window=False, *, lambd_sync=False):
        super().__init__()
        self.lambd_sync = bool(lambd_sync)          # True: read lambd to the host at every forward, as the reference does
        if not torch.is_tensor(init_lambd):
            init_lambd = torch.tensor(float(init_lambd), dtype=torch.float32)
        self.hop_length = hop_length
        self.lambd = nn.Parameter(init_lambd)                        # models.py:176
        self.device = device
        self.size = size
        self.optimized = optimized
        self.normalize_window = normalize_window

    def _make_plan(self, n_points) -> capi.Plan:
        """one plan per (device, clip length); the mel stage is never run: a fixed dummy mel configuration, and no lambd tracking"""
        return capi.Plan(n_points, self.hop_length, 1, 2, 0.0, 1.0, bool(self.normalize_window))

    def forward(self, x, lengths=None):
        _check_input("SpectrogramLayer", x, self.lambd, lengths)
        n_points = x.shape[1]
        # optimized=False (the reference's only DSPEC configuration, search_spaces.py:71-91): n_fft = 2 n_points whatever lambd is, so
        # lambd stays on the device -- no host read, the step is HIP-graph capturable.  optimized=True derives n_fft from lambd on the
        # host like the reference (time_frequency.py:39): the output SHAPE depends on it.
        lam_host = float(self.lambd.detach()) if (self.optimized or self.lambd_sync) else None
        if self.optimized:
            n_fft, half = capi.n_fft(lam_host), False
            expect = (n_fft // 2 + 1, n_points // self.hop_length + 1)
            if tuple(self.size) != expect:     # the reference's slice-assign at models.py:198 fails the same way
                raise RuntimeError(f"size={tuple(self.size)} but the spectrogram is {expect}")
        else:
            n_fft, half = 2 * n_points, True      # any clip length: powers of two on the FFT kernels, the rest through Bluestein
        return _DspecFunction.apply(_as_f32_contiguous(x), self.lambd, self._plan_for(x.device, n_points), lam_host, n_fft, half)


# BASELINE.json's north_star calls the layer by this name; the reference has no such symbol.
DifferentiableMelSpectrogram = MelSpectrogramLayer


def dmel_log_mel(x, lambd, n_mels, sample_rate, hop_length, f_min=0.0, f_max=None, normalize_window=False,
                 log=True, eps=1e-10, _plan_cache={}, *, lengths=None):
    """Functional form: log-mel (or mel) of x with window width ``lambd`` (a tensor that may require grad)."""
    if lengths is not None:
        raise RuntimeError(_no_lengths("dmel_log_mel"))
    key = (x.device.index, x.shape[1], hop_length, n_mels, sample_rate, float(f_min), f_max, bool(normalize_window))
    plan = _plan_cache.get(key)
    if plan is None:
        with torch.cuda.device(x.device):
            plan = capi.Plan(x.shape[1], hop_length, n_mels, sample_rate, float(f_min),
                             None if f_max is None else float(f_max), bool(normalize_window))
        _plan_cache[key] = plan
    return _DmelFunction.apply(_as_f32_contiguous(x.detach()), lambd, plan, float(lambd.detach()), log, eps)
