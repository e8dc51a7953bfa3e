"""The multi-window layer without a GPU: the launch choice of dmel_forward_multi_dev as a pure host function (the union over channels of
dmel_decide_launch, with the channels each n_fft serves), the constructor's validation and the parameter's state_dict entry."""
import numpy as np
import pytest
import torch

from dmel_amd import MultiWindowMelSpectrogram, capi


def _union(lams, rates, stale):
    u = {}
    for k, (lam, r) in enumerate(zip(lams, rates)):
        n, g = capi.decide_launch(lam, r, stale)
        for m, on in ((n, True), (2 * n, bool(g & 2)), (n // 2, bool(g & 1))):
            if on:
                u[m] = u.get(m, 0) | (1 << k)
    return sorted(u.items())


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("stale", [0.0, 3.0, 10.0])
def test_decide_launch_multi_is_the_union(seed, stale):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        K = int(rng.integers(1, 9))
        lams = (rng.uniform(3.0, 2700.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32).tolist()
        rates = rng.choice([0.0, 0.01, 0.5, 5.0], K).astype(np.float32).tolist()
        assert capi.decide_launch_multi(lams, rates, stale) == _union(lams, rates, stale)


@pytest.mark.parametrize("rate", [0.0, 0.001, 0.1, 1.0])
def test_decide_launch_multi_boundaries(rate):
    lams = [85.333333, 85.5, -682.6, 682.7, -128.0, 21.3]
    got = capi.decide_launch_multi(lams, [rate] * len(lams), 4.0)
    assert got == _union(lams, [rate] * len(lams), 4.0)
    # every channel's own n_fft is in the union, under its bit
    for k, lam in enumerate(lams):
        n = capi.n_fft(lam)
        assert any(m == n and (mask >> k) & 1 for m, mask in got)
    assert [m for m, _ in got] == sorted({m for m, _ in got})


def test_decide_launch_multi_channel_count():
    with pytest.raises(capi.DmelError):
        capi.decide_launch_multi([], [], 1.0)
    with pytest.raises(capi.DmelError):
        capi.decide_launch_multi([64.0] * 9, [0.0] * 9, 1.0)


def _layer(init, **kw):
    return MultiWindowMelSpectrogram(init, n_mels=32, n_points=4000, sample_rate=16000, hop_length=256, **kw)


@pytest.mark.parametrize("init", [[], [64.0] * 9, [[64.0, 128.0]], [64.0, 2.0], [64.0, 3000.0], [float("nan")]])
def test_constructor_rejects(init):
    with pytest.raises(ValueError):
        _layer(torch.tensor(init) if init and isinstance(init[0], list) else init)


def test_state_dict_and_cpu_input():
    lay = _layer([40.0, -128.0, 300.0])
    sd = lay.state_dict()
    assert list(sd.keys()) == ["lambd"] and tuple(sd["lambd"].shape) == (3,)
    assert lay.lambd.dtype == torch.float32 and lay.channels == 3
    lay2 = _layer(torch.tensor([1.0, 1.0, 1.0]) * 50)
    lay2.load_state_dict(sd)
    assert torch.equal(lay2.lambd.detach(), sd["lambd"])
    with pytest.raises(RuntimeError):
        lay(torch.zeros(2, 4000))
    with pytest.raises(ValueError):
        lay(torch.zeros(4000))


def test_symbols_declared():
    for s in ("dmel_forward_multi", "dmel_forward_multi_dev", "dmel_backward_multi", "dmel_scratch_bytes_multi",
              "dmel_plan_lambd_status_channel", "dmel_decide_launch_multi"):
        assert s in capi.SYMBOLS
