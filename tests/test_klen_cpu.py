"""Per-clip lengths on MultiWindowMelSpectrogram and BandSplitMelSpectrogram without a GPU: the flag is opt-in (off: today's refusal, word for
word), on: the scalar layer's lengths errors; lengths have no waveform gradient on these layers yet; a SlotInput and a CPU batch stay refused;
frame_lengths, extra_repr, pickling; and the four C entry points refuse NULL arguments and foreign flags before any device work."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, capi
from test_layer_refusals_cpu import HOP, LEN, M, N, NO_LEN, ON_GPU, SR, X, OnDevice, slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmel_forward_multi_lengths", "dmel_forward_multi_dev_lengths", "dmel_forward_band_lengths", "dmel_forward_band_dev_lengths")


def multi(**kw):
    return MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP, **kw)


def band(**kw):
    return BandSplitMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP, **kw)


LAYERS = [("MultiWindowMelSpectrogram", multi), ("BandSplitMelSpectrogram", band)]


def _raises(exc, message, fn, *args):
    with pytest.raises(exc) as info:
        fn(*args)
    assert type(info.value) is exc and str(info.value) == message, str(info.value)


@pytest.mark.parametrize("name,make", LAYERS)
def test_flag_off_refuses_lengths_with_the_same_words(name, make):
    assert make().per_clip_lengths is False
    for lay in (make(), make(per_clip_lengths=False), make(waveform_grad=True)):
        _raises(RuntimeError, NO_LEN.format(name), lay, X, LEN)
        _raises(RuntimeError, NO_LEN.format(name), lay, torch.zeros(N), LEN)           # lengths first: before the rank of x
        _raises(RuntimeError, NO_LEN.format(name), lay, slot(), LEN)                   # ... and before the SlotInput
    with pytest.raises(TypeError):
        type(make())([10.0, 40.0], M, N, SR, 0, None, HOP, False, True)                # keyword-only: there is no ninth positional


@pytest.mark.parametrize("name,make", LAYERS)
def test_flag_on_lengths_errors_are_the_scalar_layers(name, make):
    lay = make(per_clip_lengths=True)
    ref = MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=True)
    bad = [[N, 129, 1], LEN.float(), LEN.double(), LEN[:2], LEN[None], torch.empty(3, dtype=torch.int64, device="meta")]
    for lengths in bad:
        with pytest.raises(Exception) as want:
            ref(X, lengths)
        assert type(want.value) in (TypeError, ValueError, RuntimeError) and str(want.value) != ON_GPU
        _raises(type(want.value), str(want.value), lay, X, lengths)
    _raises(TypeError, "lengths must be a 1-D integer tensor, got list", lay, X, [N, 129, 1])
    _raises(ValueError, "lengths must have shape (3,), got (2,)", lay, X, LEN[:2])
    # the order of the scalar layer: rank and n_points of x first, the CPU batch after the lengths
    _raises(ValueError, "expected x of shape (batch, n_points), got (2000,)", lay, torch.zeros(N), "no tensor")
    _raises(RuntimeError, "input has 1999 points, the layer was built for n_points=2000", lay, torch.zeros(3, N - 1), LEN)
    _raises(RuntimeError, ON_GPU, lay, X, LEN)
    _raises(RuntimeError, ON_GPU, lay, X, LEN.long())
    _raises(RuntimeError, ON_GPU, lay, X)                                              # forward(x) is today's path


class OnMeta(OnDevice):
    """an ``x`` that says it is a device tensor where a meta ``lengths`` tensor is too: reaches the checks behind ``x.is_cuda`` with lengths"""
    device = torch.device("meta")


@pytest.mark.parametrize("name,make", LAYERS)
def test_lengths_have_no_waveform_gradient_yet(name, make):
    message = (f"per-clip lengths have no waveform gradient on {name} yet: pass x.detach() "
               "(MelSpectrogramLayer(lengths_waveform_grad=True) has one)")
    lengths = torch.empty(3, dtype=torch.int32, device="meta")
    for kw in ({}, {"waveform_grad": True}):
        _raises(RuntimeError, message, make(per_clip_lengths=True, **kw), OnMeta(requires_grad=True), lengths)
    # without lengths the flag changes nothing: waveform_grad decides, as before
    with pytest.raises(RuntimeError, match="has no waveform gradient"):
        make(per_clip_lengths=True)(OnDevice(requires_grad=True))
    _raises(RuntimeError, "lambd is on cpu but x is on cuda:0; call layer.to(x.device)", make(per_clip_lengths=True, waveform_grad=True),
            OnDevice(requires_grad=True))
    # an x that asks for no gradient passes the lengths checks and goes on to the next one
    _raises(RuntimeError, "lambd is on cpu but x is on meta; call layer.to(x.device)", make(per_clip_lengths=True), OnMeta(), lengths)


def test_other_refusals_stay():
    _raises(RuntimeError, "MultiWindowMelSpectrogram does not take a SlotInput", multi(per_clip_lengths=True), slot(), LEN)
    _raises(RuntimeError, "BandSplitMelSpectrogram does not take a SlotInput: pass the batch tensor (MelSpectrogramLayer takes slots)",
            band(per_clip_lengths=True), slot(), LEN)
    from dmel_amd import GraphedStep
    for name, make in LAYERS:
        with pytest.raises(ValueError, match=name):
            GraphedStep(lambda: None, [make(per_clip_lengths=True)])


@pytest.mark.parametrize("name,make", LAYERS)
def test_frame_lengths_repr_state_and_pickle(name, make):
    lay = make(per_clip_lengths=True)
    ln = torch.tensor([1, 99, 100, 101, 1999, 2000], dtype=torch.int64)
    fl = lay.frame_lengths(ln)
    assert fl.device.type == "cpu" and fl.dtype == torch.int64 and fl.tolist() == [v // HOP + 1 for v in ln.tolist()] == [1, 1, 2, 2, 20, 21]
    assert fl.tolist() == MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=True).frame_lengths(ln).tolist()
    assert lay.frame_lengths(ln.to(torch.int32)).tolist() == fl.tolist() and int(lay.frame_lengths(torch.tensor([N]))[0]) == lay.n_time
    assert "per_clip_lengths=True" in lay.extra_repr() and "per_clip_lengths=False" in make().extra_repr()
    assert list(lay.state_dict().keys()) == ["lambd"]
    lay._plans["a plan"] = object()
    back = pickle.loads(pickle.dumps(lay))
    assert back.per_clip_lengths is True and back._plans == {} and torch.equal(back.lambd, lay.lambd)
    assert pickle.loads(pickle.dumps(make())).per_clip_lengths is False


def test_symbols_declared_listed_resolved_and_documented():
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert re.search(r"dmel_status\s+" + s + r"\(", header), s
        assert s in capi.SYMBOLS and hasattr(L, s), s
        assert f"`{s}`" in doc, s
    assert re.search(r"#define\s+DMEL_ABI_VERSION\s+5\b", header) and L.dmel_abi_version() == 5


def test_null_arguments_and_foreign_flags_are_invalid_argument_without_a_device():
    L = capi.load()
    buf = (C.c_float * 64)()
    lens = (C.c_int32 * 4)(1, 2, 3, 4)
    edges = (C.c_int32 * 4)(0, 21, 42, 64)
    p, q, ed = C.cast(buf, C.c_void_p), C.cast(lens, C.c_void_p), C.cast(edges, C.c_void_p)

    def calls(plan, x, ln, out, flags=0):
        return (L.dmel_forward_multi_lengths(plan, x, ln, 2, p, 3, flags, 1e-10, out, p, p, None),
                L.dmel_forward_multi_dev_lengths(plan, x, ln, 2, p, 3, flags, 1e-10, out, p, p, None),
                L.dmel_forward_band_lengths(plan, x, ln, 2, p, 3, ed, flags, 1e-10, out, p, p, None),
                L.dmel_forward_band_dev_lengths(plan, x, ln, 2, p, 3, ed, flags, 1e-10, out, p, p, None))

    for plan, x, ln, out in ((None, p, q, p), (None, None, q, p), (None, p, None, p), (None, p, q, None)):
        assert calls(plan, x, ln, out) == (capi.DMEL_ERR_INVALID_ARGUMENT,) * 4
        assert "is NULL" in (L.dmel_last_error() or b"").decode("utf-8", "replace")
    # flags outside LOG | OUT_BF16 (a handle that is never dereferenced: the flags are looked at before the plan)
    fake = C.cast(buf, C.c_void_p)
    for flags in (capi.DMEL_FLAG_X_INDIRECT, capi.DMEL_FLAG_FULL_WINDOW, capi.DMEL_FLAG_MFMA_BF16X3, 1 << 30):
        assert calls(fake, p, q, p, flags | capi.DMEL_FLAG_LOG) == (capi.DMEL_ERR_INVALID_ARGUMENT,) * 4
        assert "flags" in (L.dmel_last_error() or b"").decode("utf-8", "replace")
    # malformed band edges are refused as dmel_forward_band refuses them
    worse = C.cast((C.c_int32 * 4)(0, 42, 21, 64), C.c_void_p)
    assert L.dmel_forward_band_lengths(None, p, q, 2, p, 3, worse, 0, 1e-10, p, p, p, None) == capi.DMEL_ERR_INVALID_ARGUMENT
    assert L.dmel_forward_band_dev_lengths(None, p, q, 2, p, 3, None, 0, 1e-10, p, p, p, None) == capi.DMEL_ERR_INVALID_ARGUMENT
