"""Per-clip lengths for the trainable filterbank (MelSpectrogramLayer(learnable_fb=True, lengths_learnable_fb=True)): what needs no GPU --
the opt-in and its refusals with their exact words, the three C entry points in the header, the ctypes table and INTEGRATION.md, and
their NULL checks, which come before any device call."""
import ctypes as C
import os
import re

import pytest
import torch

from dmel_amd import MelSpectrogramLayer, capi
from dmel_amd import layer as layer_mod
from test_layer_refusals_cpu import HOP, LEN, M, N, SR, OnDevice, slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmel_forward_dev_fixed_lengths", "dmel_backward_fb_dev_lengths", "dmel_backward_fb_saved_lengths")
OLD = "per-clip lengths run the HTK bank only: learnable_fb=True does not take lengths"


def mel(**kw):
    return MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=kw.pop("optimized", True), **kw)


def test_the_flag_needs_a_trainable_filterbank():
    with pytest.raises(ValueError) as info:
        mel(lengths_learnable_fb=True)
    assert str(info.value) == "lengths_learnable_fb=True is forward(x, lengths) through the trained filterbank: it needs learnable_fb=True"
    assert mel(learnable_fb=True, lengths_learnable_fb=True).lengths_learnable_fb is True
    assert mel(learnable_fb=True).lengths_learnable_fb is False and mel().lengths_learnable_fb is False


def test_without_the_flag_the_old_words():
    for kw, x, msg in (({}, torch.zeros(3, N), OLD),
                       (dict(lengths_waveform_grad=True), torch.zeros(3, N, requires_grad=True), OLD + " (and has no waveform gradient with them)")):
        with pytest.raises(RuntimeError) as info:
            mel(learnable_fb=True, **kw)(x, LEN)
        assert str(info.value) == msg


def test_with_the_flag_the_other_refusals_keep_their_words(monkeypatch):
    lay = mel(learnable_fb=True, lengths_learnable_fb=True)
    with pytest.raises(RuntimeError) as info:                                    # lengths are accepted: the next check is the device's
        lay(torch.zeros(3, N), LEN)
    assert str(info.value) == "dmel_amd runs on MI355X only: x must be a CUDA/HIP tensor (no CPU fallback)"
    with pytest.raises(RuntimeError) as info:
        mel(learnable_fb=True, lengths_learnable_fb=True, optimized=False)(torch.zeros(3, N), LEN)
    assert str(info.value) == "per-clip lengths need optimized=True (the optimized=False branch's n_fft = 2 n_points depends on the clip length)"
    with pytest.raises(TypeError):
        lay(torch.zeros(3, N), [N, 129, 1])
    # what follows x.is_cuda, with stand-ins that only claim to be on a device (the lengths then stay where they are)
    monkeypatch.setattr(layer_mod, "_lengths_for_kernels", lambda x, lengths, n_points: lengths)
    with pytest.raises(RuntimeError) as info:
        lay(slot(), LEN)
    assert str(info.value) == "a SlotInput needs the default layer: HTK bank, optimized=True, lambd_sync=False"
    for kw in ({}, dict(lengths_waveform_grad=True)):
        with pytest.raises(RuntimeError) as info:
            mel(learnable_fb=True, lengths_learnable_fb=True, **kw)(OnDevice(requires_grad=True), LEN)
        assert str(info.value) == "learnable_fb with per-clip lengths has no waveform gradient: pass x.detach()"
    with pytest.raises(RuntimeError) as info:                                    # the HTK layer keeps its own words
        mel()(OnDevice(requires_grad=True), LEN)
    assert str(info.value) == "per-clip lengths have no waveform gradient: pass x.detach()"


def test_extra_repr_names_the_flag():
    assert "lengths_learnable_fb=True" in repr(mel(learnable_fb=True, lengths_learnable_fb=True))
    assert "lengths_learnable_fb" not in repr(mel(learnable_fb=True)) and "lengths_learnable_fb" not in repr(mel())


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "dmel.h")).read()
    m = re.search(r"dmel_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_symbols_and_signatures_agree():
    L = capi.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s), s
        assert f"`{s}`" in doc, s
        restype, argtypes = capi._SIGNATURES[s]
        args = _header_args(s)
        assert restype is C.c_int and len(args) == len(argtypes), (s, args)
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is C.c_void_p, (s, a)
            elif a.startswith("int32_t"):
                assert t is C.c_int32, (s, a)
            elif a.startswith("uint32_t"):
                assert t is C.c_uint32, (s, a)
            elif a.startswith("double"):
                assert t is C.c_double, (s, a)
            else:
                raise AssertionError((s, a))
    assert _header_args(NEW[0])[:6] == ["dmel_plan* plan", "const float* x", "const int32_t* lengths", "int32_t batch", "const float* lambd_dev",
                                        "int32_t n_fft"]
    assert _header_args(NEW[1])[-4:] == ["const float* grad_out", "const float* out", "float* grad_fb", "void* stream"]
    assert _header_args(NEW[2])[-6:] == ["const float* out", "const float* tangent", "float* grad_fb", "float* dlambd", "void* scratch", "void* stream"]
    for s, cites in ((NEW[0], ("models.py:38", "models.py:53", "models.py:73", "datasets.py:175")), (NEW[1], ("models.py:38", "models.py:53", "models.py:73", "datasets.py:175"))):
        text = open(os.path.join(ROOT, "include", "dmel.h")).read()
        comment = text[:text.index("dmel_status " + s)].rsplit("/*", 1)[1]
        assert all(c in comment for c in cites), (s, comment)


def test_null_arguments_are_invalid_argument_without_a_device():
    L = capi.load()
    buf = (C.c_float * 64)()
    lens = (C.c_int32 * 4)(1, 2, 3, 4)
    p, q = C.cast(buf, C.c_void_p), C.cast(lens, C.c_void_p)
    bad = capi.DMEL_ERR_INVALID_ARGUMENT
    # (the checks read no plan: `p` stands in for one where another argument is the NULL one)
    for plan, x, ln, lam, out in ((None, p, q, p, p), (p, None, q, p, p), (p, p, None, p, p), (p, p, q, None, p), (p, p, q, p, None)):
        assert L.dmel_forward_dev_fixed_lengths(plan, x, ln, 4, lam, 512, 0, 1e-10, out, None, None, None, None) == bad
    assert L.dmel_forward_dev_fixed_lengths(p, p, q, 4, p, 512, 0, 1e-10, p, None, p, None, None) == bad             # spec without a tangent
    assert "tangent is NULL" in L.dmel_last_error().decode()
    for plan, x, ln, lam, g, gfb in ((None, p, q, p, p, p), (p, None, q, p, p, p), (p, p, None, p, p, p), (p, p, q, None, p, p), (p, p, q, p, None, p),
                                     (p, p, q, p, p, None)):
        assert L.dmel_backward_fb_dev_lengths(plan, x, ln, 4, lam, 512, 0, g, None, gfb, None) == bad
    for plan, sp, ln, g, gfb in ((None, p, q, p, p), (p, None, q, p, p), (p, p, None, p, p), (p, p, q, None, p), (p, p, q, p, None)):
        assert L.dmel_backward_fb_saved_lengths(plan, sp, ln, 4, 512, 0, g, None, None, gfb, None, None, None) == bad
    assert L.dmel_backward_fb_saved_lengths(p, p, q, 4, 512, 0, p, None, p, p, None, None, None) == bad               # a tangent without dlambd
    assert L.dmel_backward_fb_saved_lengths(p, p, q, 4, 512, capi.DMEL_FLAG_LOG, p, None, None, p, None, None, None) == bad   # LOG without the output
    # a store pointer that is not 16-byte aligned is refused by name
    off = C.c_void_p(C.addressof(buf) + 4 if C.addressof(buf) % 16 == 0 else C.addressof(buf) + (16 - C.addressof(buf) % 16) + 4)
    assert L.dmel_forward_dev_fixed_lengths(p, p, q, 4, p, 512, 0, 1e-10, off, None, None, None, None) == bad
    assert "out must be 16-byte aligned" in L.dmel_last_error().decode()
    assert L.dmel_backward_fb_dev_lengths(p, p, q, 4, p, 512, 0, p, None, off, None) == bad
    assert "grad_fb must be 16-byte aligned" in L.dmel_last_error().decode()
