"""The host checks the stages behind the mel layers share (dmel_amd/_stage.py), without a GPU: every stage refuses a wrong mel image, wrong
``frame_lengths`` and a CPU tensor with the exception type and the full text it raised while each stage carried its own copy of the checks.
The texts below are literals recorded from those copies, not built from the pattern the shared code builds them from.  The two pooling
stages refuse wrong ``stats`` / ``eps`` alike."""
import re

import pytest
import torch

import dmel_amd

MAKE = {"BandNorm": lambda: dmel_amd.BandNorm(4), "SpecMask": lambda: dmel_amd.SpecMask(), "Deltas": lambda: dmel_amd.Deltas(),
        "StatsPool": lambda: dmel_amd.StatsPool(), "AttentivePool": lambda: dmel_amd.AttentivePool(), "PCEN": lambda: dmel_amd.PCEN(4)}
LENGTH_STAGES = ("BandNorm", "SpecMask", "Deltas", "StatsPool", "AttentivePool")

REFUSALS = {
    "BandNorm": {
        "list": (TypeError, "BandNorm: frame_lengths must be a 1-D integer tensor, got list"),
        "float": (TypeError, "BandNorm: frame_lengths must hold int32 or int64 values, got torch.float32"),
        "shape (3,)": (ValueError, "BandNorm: frame_lengths must have shape (2,), got (3,)"),
        "shape (2, 1)": (ValueError, "BandNorm: frame_lengths must have shape (2,), got (2, 1)"),
        "2-D": (ValueError, "BandNorm: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "BandNorm: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "BandNorm: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "BandNorm takes an fp32 mel image (a layer with out_dtype=torch.float32), got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: BandNorm's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
    "SpecMask": {
        "list": (TypeError, "SpecMask: frame_lengths must be a 1-D integer tensor, got list"),
        "float": (TypeError, "SpecMask: frame_lengths must hold int32 or int64 values, got torch.float32"),
        "shape (3,)": (ValueError, "SpecMask: frame_lengths must have shape (2,), got (3,)"),
        "shape (2, 1)": (ValueError, "SpecMask: frame_lengths must have shape (2,), got (2, 1)"),
        "2-D": (ValueError, "SpecMask: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "SpecMask: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "SpecMask: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "SpecMask takes an fp32 or bf16 mel image, got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: SpecMask's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
    "Deltas": {
        "list": (TypeError, "Deltas: frame_lengths must be a 1-D integer tensor, got list"),
        "float": (TypeError, "Deltas: frame_lengths must hold int32 or int64 values, got torch.float32"),
        "shape (3,)": (ValueError, "Deltas: frame_lengths must have shape (2,), got (3,)"),
        "shape (2, 1)": (ValueError, "Deltas: frame_lengths must have shape (2,), got (2, 1)"),
        "2-D": (ValueError, "Deltas: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "Deltas: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "Deltas: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "Deltas takes an fp32 mel image, got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: Deltas's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
    "StatsPool": {
        "list": (TypeError, "StatsPool: frame_lengths must be a 1-D integer tensor, got list"),
        "float": (TypeError, "StatsPool: frame_lengths must hold int32 or int64 values, got torch.float32"),
        "shape (3,)": (ValueError, "StatsPool: frame_lengths must have shape (2,), got (3,)"),
        "shape (2, 1)": (ValueError, "StatsPool: frame_lengths must have shape (2,), got (2, 1)"),
        "2-D": (ValueError, "StatsPool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "StatsPool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "StatsPool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "StatsPool takes an fp32 mel image, got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: StatsPool's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
    "AttentivePool": {
        "list": (TypeError, "AttentivePool: frame_lengths must be a 1-D integer tensor, got list"),
        "float": (TypeError, "AttentivePool: frame_lengths must hold int32 or int64 values, got torch.float32"),
        "shape (3,)": (ValueError, "AttentivePool: frame_lengths must have shape (2,), got (3,)"),
        "shape (2, 1)": (ValueError, "AttentivePool: frame_lengths must have shape (2,), got (2, 1)"),
        "2-D": (ValueError, "AttentivePool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "AttentivePool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "AttentivePool: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "AttentivePool takes an fp32 mel image, got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: AttentivePool's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
    "PCEN": {
        "2-D": (ValueError, "PCEN: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (4, 8)"),
        "5-D": (ValueError, "PCEN: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got (1, 1, 2, 4, 8)"),
        "no tensor": (ValueError, "PCEN: expected a (B, n_mels, T) or (B, C, n_mels, T) tensor, got list"),
        "fp64": (RuntimeError, "PCEN takes fp32 linear mel power (a layer with log=False, out_dtype=torch.float32), got torch.float64"),
        "cpu": (RuntimeError, "dmel_amd runs on MI355X only: PCEN's input must be a CUDA/HIP tensor (no CPU fallback)"),
    },
}

POOL_REFUSALS = {
    "StatsPool": {
        "unknown": "StatsPool: stats must be a non-empty subset of ('mean', 'std', 'max'), got ('mean', 'median')",
        "empty": "StatsPool: stats must be a non-empty subset of ('mean', 'std', 'max'), got ()",
        "no sequence": "StatsPool: stats must be a non-empty subset of ('mean', 'std', 'max'), got 3",
        "twice": "StatsPool: stats names a statistic twice: ('mean', 'mean')",
        "eps 0": "StatsPool: eps must be a finite number > 0, got 0.0",
        "eps nan": "StatsPool: eps must be a finite number > 0, got nan",
        "eps bool": "StatsPool: eps must be a finite number > 0, got True",
        "eps str": "StatsPool: eps must be a finite number > 0, got '1'",
    },
    "AttentivePool": {
        "unknown": "AttentivePool: stats must be a non-empty subset of ('mean', 'std'), got ('mean', 'median')",
        "empty": "AttentivePool: stats must be a non-empty subset of ('mean', 'std'), got ()",
        "no sequence": "AttentivePool: stats must be a non-empty subset of ('mean', 'std'), got 3",
        "twice": "AttentivePool: stats names a statistic twice: ('mean', 'mean')",
        "eps 0": "AttentivePool: eps must be a finite number > 0, got 0.0",
        "eps nan": "AttentivePool: eps must be a finite number > 0, got nan",
        "eps bool": "AttentivePool: eps must be a finite number > 0, got True",
        "eps str": "AttentivePool: eps must be a finite number > 0, got '1'",
    },
}


def _image():
    return torch.zeros(2, 4, 8)


def _call(name, s, *frame_lengths):
    extra = (torch.zeros(2, 8),) if name == "AttentivePool" else ()
    return MAKE[name]()(s, *extra, *frame_lengths)


def _refused(expected, fn):
    kind, text = expected
    with pytest.raises(kind, match="^" + re.escape(text) + "$") as info:
        fn()
    assert type(info.value) is kind


@pytest.mark.parametrize("name", LENGTH_STAGES)
def test_frame_lengths_refusals(name):
    want, s = REFUSALS[name], _image()
    _refused(want["list"], lambda: _call(name, s, [8, 8]))
    _refused(want["float"], lambda: _call(name, s, torch.tensor([8.0, 8.0])))
    _refused(want["shape (3,)"], lambda: _call(name, s, torch.tensor([8, 8, 8])))
    _refused(want["shape (2, 1)"], lambda: _call(name, s, torch.tensor([[8], [8]])))


@pytest.mark.parametrize("name", LENGTH_STAGES + ("PCEN",))
def test_mel_image_refusals(name):
    want = REFUSALS[name]
    _refused(want["2-D"], lambda: _call(name, torch.zeros(4, 8)))
    _refused(want["5-D"], lambda: _call(name, torch.zeros(1, 1, 2, 4, 8)))
    _refused(want["no tensor"], lambda: _call(name, [1, 2]))
    _refused(want["fp64"], lambda: _call(name, _image().double()))


@pytest.mark.parametrize("name", LENGTH_STAGES + ("PCEN",))
def test_valid_arguments_on_the_cpu_are_refused(name):
    want = REFUSALS[name]["cpu"]
    _refused(want, lambda: _call(name, _image()))
    _refused(want, lambda: _call(name, torch.zeros(2, 1, 4, 8)))
    if name != "PCEN":
        for dtype in (torch.int32, torch.int64):
            _refused(want, lambda: _call(name, _image(), torch.tensor([8, 3], dtype=dtype)))


def test_a_doubly_wrong_call_gets_the_earlier_check():
    """image shape, image dtype, lengths, the stage's own checks, T == 0, the device: the order every stage keeps"""
    for name in LENGTH_STAGES:
        _refused(REFUSALS[name]["2-D"], lambda: _call(name, torch.zeros(4, 8, dtype=torch.float64), [8]))
        _refused(REFUSALS[name]["fp64"], lambda: _call(name, _image().double(), [8, 8]))
    # (BandNorm and PCEN look at the band count with the image, before the lengths)
    _refused((RuntimeError, "BandNorm was built for n_mels=5 but dim -2 of the input has 4 bands"), lambda: dmel_amd.BandNorm(5)(_image(), [8, 8]))
    _refused((RuntimeError, "PCEN was built for n_mels=5 but dim -2 of the input has 4 bands"), lambda: dmel_amd.PCEN(5)(_image()))
    _refused(REFUSALS["AttentivePool"]["list"], lambda: dmel_amd.AttentivePool()(_image(), torch.zeros(3, 8), [8, 8]))
    _refused((ValueError, "AttentivePool: logits must have shape (2, 8), (2, A, 8) with A dividing C n_mels = 4, or (2, 1, 4, 8), got (3, 8)"),
             lambda: dmel_amd.AttentivePool()(_image(), torch.zeros(3, 8)))
    _refused((ValueError, "StatsPool: the input has no frames (T = 0): there is nothing to pool"), lambda: dmel_amd.StatsPool()(torch.zeros(2, 4, 0)))
    assert dmel_amd.Deltas()(torch.zeros(2, 4, 0)).shape == (2, 3, 4, 0)            # an empty tensor comes back before the device is asked for
    assert dmel_amd.SpecMask().eval()(_image(), [8, 8]).shape == (2, 4, 8)          # eval returns its argument before it looks at the lengths


@pytest.mark.parametrize("name", sorted(POOL_REFUSALS))
def test_pooling_constructor_refusals(name):
    cls, want = getattr(dmel_amd, name), {k: (ValueError, v) for k, v in POOL_REFUSALS[name].items()}
    _refused(want["unknown"], lambda: cls(stats=("mean", "median")))
    _refused(want["empty"], lambda: cls(stats=()))
    _refused(want["no sequence"], lambda: cls(stats=3))
    _refused(want["twice"], lambda: cls(stats=("mean", "mean")))
    _refused(want["eps 0"], lambda: cls(eps=0.0))
    _refused(want["eps nan"], lambda: cls(eps=float("nan")))
    _refused(want["eps bool"], lambda: cls(eps=True))
    _refused(want["eps str"], lambda: cls(eps="1"))
    assert cls(stats="std").stats == ("std",) and cls(stats=("std", "mean"), eps=1).stats == ("mean", "std")
    assert cls(eps=1).eps == 1.0 and isinstance(cls(eps=1).eps, float)

