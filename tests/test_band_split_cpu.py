"""BandSplitMelSpectrogram without a GPU: the three C entry points are declared, exported, listed and documented; NULL and malformed
band_edges are DMEL_ERR_INVALID_ARGUMENT before any device work; the constructor validates lambd and the edges and derives the default
ones; a CPU batch raises; and the code objects of build/dmel_fwd_band_part*.o hold every instantiation the layer dispatches to, the
training ones up to n_fft 4096 free of spills and scratch."""
import ctypes as C
import os
import re

import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram, capi
from test_lengths_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmel_forward_band", "dmel_forward_band_dev", "dmel_backward_band")


def test_symbols_declared_listed_resolved_and_documented():
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert re.search(r"dmel_status\s+" + s + r"\(", header), s
        assert s in capi.SYMBOLS, s
        assert hasattr(L, s), s
        assert f"`{s}`" in doc, s
    assert "net.spectrogram_layer = BandSplitMelSpectrogram(" in doc
    assert re.search(r"#define\s+DMEL_ABI_VERSION\s+5\b", header)
    import dmel_amd
    assert "BandSplitMelSpectrogram" in dmel_amd.__all__


def _calls(L, plan, edges, channels):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ed = C.cast(edges, C.c_void_p) if edges is not None else None
    return (L.dmel_forward_band(plan, p, 2, p, channels, ed, 0, 1e-10, p, p, p, None),
            L.dmel_forward_band_dev(plan, p, 2, p, channels, ed, 0, 1e-10, p, p, p, None),
            L.dmel_backward_band(plan, p, capi.DMEL_DTYPE_F32, p, 2, channels, ed, 0, p, p, None))


def test_bad_arguments_are_invalid_argument_without_a_device():
    L = capi.load()
    good = (C.c_int32 * 4)(0, 21, 42, 64)
    bad = {
        "NULL edges": (None, 3),
        "not ascending": ((C.c_int32 * 4)(0, 42, 21, 64), 3),
        "not starting at 0": ((C.c_int32 * 4)(1, 21, 42, 64), 3),
        "empty group": ((C.c_int32 * 4)(0, 21, 21, 64), 3),
        "K = 0": (good, 0),
        "K = 9": ((C.c_int32 * 10)(*range(0, 10)), 9),
        "K < 0": (good, -1),
    }
    for name, (edges, k) in bad.items():
        assert _calls(L, None, edges, k) == (capi.DMEL_ERR_INVALID_ARGUMENT,) * 3, name
        msg = (L.dmel_last_error() or b"").decode("utf-8", "replace")
        assert "plan is NULL" not in msg, (name, msg)             # refused for the edges themselves, before the plan is looked at
    # well-formed edges, no plan: still refused before any device work ("not ending at n_mels" needs the plan's n_mels: GPU suite)
    assert _calls(L, None, good, 3) == (capi.DMEL_ERR_INVALID_ARGUMENT,) * 3


def test_constructor_validation_and_default_edges():
    lay = BandSplitMelSpectrogram([300.0, 128.0, 40.0], 64, 8000, 16000, hop_length=128)
    assert list(lay.band_edges) == [0, 21, 42, 64]
    assert lay.lambd.shape == (3,) and [n for n, _ in lay.named_parameters()] == ["lambd"]
    assert list(lay.state_dict().keys()) == ["lambd"]                        # the edges come from the constructor, not from checkpoints
    assert isinstance(lay, MultiWindowMelSpectrogram) and lay.MAX_CHANNELS == 8
    assert list(BandSplitMelSpectrogram([128.0], 40, 8000, 16000).band_edges) == [0, 40]
    assert list(BandSplitMelSpectrogram([128.0] * 8, 64, 8000, 16000).band_edges) == [0, 8, 16, 24, 32, 40, 48, 56, 64]
    assert list(BandSplitMelSpectrogram([128.0, 40.0], 64, 8000, 16000, band_edges=[0, 5, 64]).band_edges) == [0, 5, 64]
    assert list(BandSplitMelSpectrogram([128.0, 40.0], 64, 8000, 16000, band_edges=torch.tensor([0, 63, 64])).band_edges) == [0, 63, 64]
    for edges in ([0, 64], [0, 5, 30, 64], [1, 5, 64], [0, 5, 63], [0, 5, 5], [0, 64, 64], [0, 40, 30], [0, 5.5, 64]):
        with pytest.raises(ValueError):
            BandSplitMelSpectrogram([128.0, 40.0], 64, 8000, 16000, band_edges=edges)
    with pytest.raises(ValueError):
        BandSplitMelSpectrogram([128.0] * 9, 64, 8000, 16000)
    with pytest.raises(ValueError):
        BandSplitMelSpectrogram([], 64, 8000, 16000)
    with pytest.raises(ValueError):
        BandSplitMelSpectrogram([128.0, 1.0], 64, 8000, 16000)               # n_fft 8 < 32
    with pytest.raises(ValueError):
        BandSplitMelSpectrogram([128.0, 3000.0], 64, 8000, 16000)            # n_fft 32768 > 16384
    with pytest.raises(ValueError):
        BandSplitMelSpectrogram([128.0, 40.0, 30.0], 2, 8000, 16000)         # more groups than mel bands
    # state_dict round trip: lambd travels, the edges stay the constructor's
    other = BandSplitMelSpectrogram([100.0, 100.0, 100.0], 64, 8000, 16000, hop_length=128, band_edges=[0, 5, 30, 64])
    other.load_state_dict(lay.state_dict())
    assert other.lambd.tolist() == [300.0, 128.0, 40.0] and list(other.band_edges) == [0, 5, 30, 64]


def test_cpu_input_and_out_of_scope_uses_raise():
    lay = BandSplitMelSpectrogram([128.0, 40.0], 32, 8000, 16000, hop_length=128)
    x = torch.zeros(2, 8000)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        lay(x)
    with pytest.raises(RuntimeError, match="lengths"):
        lay(x, lengths=torch.tensor([8000, 8000]))
    with pytest.raises(ValueError):
        lay(x[0])
    with pytest.raises(RuntimeError, match="n_points"):
        lay(x[:, :100])
    from dmel_amd import GraphedStep
    with pytest.raises(ValueError, match="BandSplitMelSpectrogram"):
        GraphedStep(lambda: None, [lay])            # (LambdAdam(fused_into_backward=...) needs device parameters: GPU suite)


def test_band_kernel_resources():
    res = _resources(r"dmel_fwd_band_part\d\.o", "dmel_fwd_band_kernel")
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    # kTrain (0) and kInfer (1) at every size, kTrainW (5) where it is built; one tile per workgroup
    want = {(n, m, 1) for n in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384) for m in (0, 1)} | {(1024, 5, 1), (2048, 5, 1)}
    assert want <= set(res), sorted(want - set(res))
    for (n, mode, tpw), (_, spill, scratch) in sorted(res.items()):
        if mode in (0, 5) and n <= 4096:
            assert spill == 0 and scratch == 0, (n, mode, tpw, res[(n, mode, tpw)])
