"""What the five ``forward``s refuse, and with which words: exception type, message and -- where two refusals apply -- which one wins.
Everything here is raised before a kernel or a plan is touched, so it runs without a GPU; the checks behind ``x.is_cuda`` are reached
with a stand-in that only claims to be on a device."""
import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, SlotInput, SpectrogramLayer, dmel_log_mel

N, SR, HOP, M = 2000, 16000, 100, 16
ON_GPU = "dmel_amd runs on MI355X only: x must be a CUDA/HIP tensor (no CPU fallback)"
LAMBD_DEV = "lambd is on cpu but x is on cuda:0; call layer.to(x.device)"


class OnDevice:
    """an ``x`` that says it is a (3, n) fp32 tensor on cuda:0: enough for every check that follows ``x.is_cuda``"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cuda", 0)

    def __init__(self, n=N, requires_grad=False):
        self.shape, self.requires_grad = (3, n), requires_grad

    def dim(self):
        return 2


def slot():
    s = SlotInput.__new__(SlotInput)                 # (the constructor wants a device cell)
    s.cell, s.shape, s.device = torch.zeros(1, dtype=torch.int64), (3, N), torch.device("cuda", 0)
    return s


def mel(**kw):
    return MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=kw.pop("optimized", True), **kw)


def multi(**kw):
    return MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP, **kw)


def band(**kw):
    return BandSplitMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP, **kw)


def spec():
    return SpectrogramLayer(10.0)


X = torch.zeros(3, N)
XG = torch.zeros(3, N, requires_grad=True)
LEN = torch.tensor([N, 129, 1], dtype=torch.int32)
NO_LEN = "{} does not take per-clip lengths (MelSpectrogramLayer does)"
CASES = [
    # MelSpectrogramLayer.forward(x)
    ("mel rank", mel, (torch.zeros(N),), ValueError, "expected x of shape (batch, n_points), got (2000,)"),
    ("mel n_points", mel, (torch.zeros(3, N - 1),), RuntimeError, "input has 1999 points, the layer was built for n_points=2000"),
    ("mel cpu", mel, (X,), RuntimeError, ON_GPU),
    ("mel lambd elsewhere", mel, (OnDevice(),), RuntimeError, LAMBD_DEV),
    ("mel slot, not the default layer", lambda: mel(lambd_sync=True), (slot(),), RuntimeError,
     "a SlotInput needs the default layer: HTK bank, optimized=True, lambd_sync=False"),
    ("mel slot, optimized=False", lambda: mel(optimized=False), (slot(),), RuntimeError,
     "a SlotInput needs the default layer: HTK bank, optimized=True, lambd_sync=False"),
    ("mel slot, lambd elsewhere", mel, (slot(),), RuntimeError, "lambd is on cpu but the slot is on cuda:0; call layer.to(device)"),
    ("mel slot, wrong n_points first", lambda: MelSpectrogramLayer(10.0, M, N + 1, SR, hop_length=HOP, optimized=True, lambd_sync=True), (slot(),),
     RuntimeError, "input has 2000 points, the layer was built for n_points=2001"),
    # MelSpectrogramLayer.forward(x, lengths)
    ("len rank first", mel, (torch.zeros(N), "no tensor"), ValueError, "expected x of shape (batch, n_points), got (2000,)"),
    ("len n_points before the filterbank", lambda: mel(learnable_fb=True), (torch.zeros(3, N - 1), LEN), RuntimeError,
     "input has 1999 points, the layer was built for n_points=2000"),
    ("len mel_fb", lambda: mel(learnable_fb=True), (X, LEN), RuntimeError,
     "per-clip lengths run the HTK bank only: learnable_fb=True does not take lengths"),
    ("len mel_fb, x grad", lambda: mel(learnable_fb=True, lengths_waveform_grad=True), (XG, LEN), RuntimeError,
     "per-clip lengths run the HTK bank only: learnable_fb=True does not take lengths (and has no waveform gradient with them)"),
    ("len optimized=False", lambda: mel(optimized=False), (X, LEN), RuntimeError,
     "per-clip lengths need optimized=True (the optimized=False branch's n_fft = 2 n_points depends on the clip length)"),
    ("len optimized=False, x grad", lambda: mel(optimized=False, lengths_waveform_grad=True), (XG, LEN), RuntimeError,
     "per-clip lengths need optimized=True (the optimized=False branch's n_fft = 2 n_points depends on the clip length)"
     "; the waveform gradient of per-clip lengths needs it too"),
    ("len no tensor", mel, (X, [N, 129, 1]), TypeError, "lengths must be a 1-D integer tensor, got list"),
    ("len dtype", mel, (X, LEN.float()), TypeError, "lengths must hold int32 or int64 values, got torch.float32"),
    ("len shape", mel, (X, LEN[:2]), ValueError, "lengths must have shape (3,), got (2,)"),
    ("len rank 2", mel, (X, LEN[None]), ValueError, "lengths must have shape (3,), got (1, 3)"),
    ("len device", mel, (X, torch.empty(3, dtype=torch.int64, device="meta")), RuntimeError, "lengths is on meta but x is on cpu"),
    ("len dtype before cpu", mel, (X, LEN.double()), TypeError, "lengths must hold int32 or int64 values, got torch.float64"),
    ("len cpu", mel, (X, LEN), RuntimeError, ON_GPU),
    ("len cpu before x grad", mel, (XG, LEN.long()), RuntimeError, ON_GPU),
    # MultiWindowMelSpectrogram
    ("multi lengths first", multi, (torch.zeros(N), LEN), RuntimeError, NO_LEN.format("MultiWindowMelSpectrogram")),
    ("multi slot", multi, (slot(),), RuntimeError, "MultiWindowMelSpectrogram does not take a SlotInput"),
    ("multi rank", multi, (torch.zeros(1, 3, N),), ValueError, "expected x of shape (batch, n_points), got (1, 3, 2000)"),
    ("multi n_points", multi, (torch.zeros(3, N + 1),), RuntimeError, "input has 2001 points, the layer was built for n_points=2000"),
    ("multi cpu before x grad", multi, (XG,), RuntimeError, ON_GPU),
    ("multi x grad", multi, (OnDevice(requires_grad=True),), RuntimeError,
     "MultiWindowMelSpectrogram has no waveform gradient by default: pass waveform_grad=True, or x.detach()"),
    ("multi x grad taken, lambd elsewhere", lambda: multi(waveform_grad=True), (OnDevice(requires_grad=True),), RuntimeError, LAMBD_DEV),
    # BandSplitMelSpectrogram
    ("band lengths first", band, (slot(), LEN), RuntimeError, NO_LEN.format("BandSplitMelSpectrogram")),
    ("band slot", band, (slot(),), RuntimeError,
     "BandSplitMelSpectrogram does not take a SlotInput: pass the batch tensor (MelSpectrogramLayer takes slots)"),
    ("band rank", band, (torch.zeros(N),), ValueError, "expected x of shape (batch, n_points), got (2000,)"),
    ("band n_points", band, (torch.zeros(3, 7),), RuntimeError, "input has 7 points, the layer was built for n_points=2000"),
    ("band cpu", band, (X,), RuntimeError, ON_GPU),
    ("band x grad", band, (OnDevice(requires_grad=True),), RuntimeError,
     "BandSplitMelSpectrogram has no waveform gradient: pass x.detach() (MelSpectrogramLayer and "
     "MultiWindowMelSpectrogram(waveform_grad=True) have one)"),
    ("band lambd elsewhere", band, (OnDevice(),), RuntimeError, LAMBD_DEV),
    # SpectrogramLayer: any n_points, and an x that requires grad is taken
    ("spec lengths", spec, (X, LEN), RuntimeError, NO_LEN.format("SpectrogramLayer")),
    ("spec rank", spec, (torch.zeros(N),), ValueError, "expected x of shape (batch, n_points), got (2000,)"),
    ("spec cpu", spec, (torch.zeros(3, 250),), RuntimeError, ON_GPU),
    ("spec lambd elsewhere", spec, (OnDevice(250, requires_grad=True),), RuntimeError, LAMBD_DEV),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_refuses_with_the_same_words(case):
    _, make, args, exc, message = case
    with pytest.raises(exc) as info:
        make()(*args)
    assert type(info.value) is exc and str(info.value) == message


def test_functional_form_refuses_lengths():
    with pytest.raises(RuntimeError) as info:
        dmel_log_mel(X, torch.tensor(10.0), M, SR, HOP, lengths=LEN)
    assert str(info.value) == NO_LEN.format("dmel_log_mel")
