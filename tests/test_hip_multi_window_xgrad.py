"""MultiWindowMelSpectrogram(waveform_grad=True) on the MI355X: x.grad equals, bit for bit, the sum in ascending channel order of what the K
scalar layers give (zeros + gx_0 + gx_1 + ...), on the wave-FFT and LDS paths, with the prep kernel's window (long clips, normalized
window), in bf16 / lambd_sync / inference mode, deterministically, for an uncovered channel (NaN, then named), inside a captured step and in
a multi-resolution loss; and it meets the fp64 oracle's bar."""
import numpy as np
import pytest
import torch

from dmel_amd import MelSpectrogramLayer, MultiWindowMelSpectrogram, synth
from oracle import dmel_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM_SETS = [[128.0, 128.0, 128.0], [40.0, 128.0, 300.0], [-128.0, 85.3, 85.5], [6.0, 700.0, 2000.0]]


def _inputs(B, L, K, M, hop, seed=3, dtype=torch.float32):
    x = torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, K, M, L // hop + 1), seed=seed + 1)).to(DEV).to(dtype)
    return x, g


def _multi_grad(lams, x, g, M, L, sr, hop, log, out_dtype=torch.float32, sync=False, normalize=False, lambd_grad=True):
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, normalize_window=normalize, log=log, out_dtype=out_dtype,
                                      lambd_sync=sync, waveform_grad=True).to(DEV)
    multi.lambd.requires_grad_(lambd_grad)
    xr = x.detach().clone().requires_grad_(True)
    y = multi(xr)
    if out_dtype == torch.float32:
        (y * g).sum().backward()
    else:
        y.backward(g)
    return multi, y.detach(), xr.grad


def _scalar_sum(lams, x, g, M, L, sr, hop, log, out_dtype=torch.float32, normalize=False, lambd_grad=True):
    """zeros + gx_0 + gx_1 + ...: the waveform gradients of K scalar layers, added in ascending channel order; their outputs and lambd.grad"""
    acc = torch.zeros_like(x)
    ys, dls = [], []
    for k, v in enumerate(lams):
        lay = MelSpectrogramLayer(torch.tensor(float(v)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                  normalize_window=normalize, log=log, out_dtype=out_dtype).to(DEV)
        lay.lambd.requires_grad_(lambd_grad)
        xk = x.detach().clone().requires_grad_(True)
        yk = lay(xk)
        gk = g[:, k:k + 1].contiguous()
        if out_dtype == torch.float32:
            (yk * gk).sum().backward()
        else:
            yk.backward(gk)
        acc = acc + xk.grad
        ys.append(yk.detach())
        dls.append(None if lay.lambd.grad is None else float(lay.lambd.grad))
    return acc, ys, dls


def _check(lams, B, L, sr, hop, M, log, **kw):
    x, g = _inputs(B, L, len(lams), M, hop, dtype=kw.get("out_dtype", torch.float32))
    multi, y, gx = _multi_grad(lams, x, g, M, L, sr, hop, log, **kw)
    kw.pop("sync", None)
    ref, ys, dls = _scalar_sum(lams, x, g, M, L, sr, hop, log, **kw)
    for k in range(len(lams)):
        assert torch.equal(y[:, k:k + 1], ys[k]), (k, lams[k])
        if dls[k] is not None:
            d = float(multi.lambd.grad[k])
            assert abs(d - dls[k]) <= 1e-6 * abs(dls[k]) + 1e-12, (k, d, dls[k])
    assert torch.isfinite(gx).all()
    assert torch.equal(gx, ref), float((gx - ref).abs().max())
    return multi, x, g, y, gx


@pytest.mark.parametrize("lams", LAM_SETS)
@pytest.mark.parametrize("log", [False, True])
def test_xgrad_equals_scalar_sum(lams, log):
    _check(lams, 4, 8000, 16000, 128, 64, log)


@pytest.mark.parametrize("lams", [[40.0, 128.0, 300.0], [6.0, 700.0, 2000.0]])
def test_xgrad_against_oracle(lams):
    B, L, sr, hop, M = 3, 8000, 16000, 200, 48
    x, g = _inputs(B, L, len(lams), M, hop, seed=5)
    _, y, gx = _multi_grad(lams, x, g, M, L, sr, hop, True)
    x_np, g_np, y_np = x.cpu().numpy(), g.cpu().numpy(), y.cpu().numpy()
    ref = sum(O.backward_x(x_np, lam, hop, sr, np.ascontiguousarray(g_np[:, k:k + 1]), np.ascontiguousarray(y_np[:, k:k + 1]))
              for k, lam in enumerate(lams))
    err = float(np.abs(gx.cpu().numpy().astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))
    assert err <= 1e-4, err


def test_xgrad_config2_mixed_set():
    _check([40.0, 128.0, 300.0], 256, 16000, 16000, 512, 128, True)


def test_xgrad_prep_paths():
    _check([64.0, 700.0, 2000.0], 2, 40000, 16000, 400, 40, True)               # > 32768 samples: window tables from the prep kernel
    _check([40.0, 128.0, 300.0], 4, 8000, 16000, 128, 64, True, normalize=True)


def test_xgrad_modes():
    lams, B, L, sr, hop, M = [40.0, 128.0, 300.0], 4, 8000, 16000, 128, 64
    # bf16 + log: fp32 computed and rounded afterwards -- the same bits as the default layer's in-kernel rounding
    _, x, g, y, _ = _check(lams, B, L, sr, hop, M, True, out_dtype=torch.bfloat16)
    plain = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, out_dtype=torch.bfloat16).to(DEV)
    assert torch.equal(plain(x), y)
    # lambd_sync=True (host values, dmel_backward_x_multi) gives the bits of the device path
    x, g = _inputs(B, L, 3, M, hop)
    _, y0, gx0 = _multi_grad(lams, x, g, M, L, sr, hop, True)
    _, y1, gx1 = _multi_grad(lams, x, g, M, L, sr, hop, True, sync=True)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    # lambd not trained: the inference-mode forward, still the scalar sum
    _check(lams, B, L, sr, hop, M, True, lambd_grad=False)


def test_xgrad_deterministic():
    lams, B, L, sr, hop, M = [6.0, 128.0, 2000.0], 4, 8000, 16000, 128, 64
    x, g = _inputs(B, L, 3, M, hop)
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    grads = []
    for _ in range(2):
        xr = x.clone().requires_grad_(True)
        (multi(xr) * g).sum().backward()
        grads.append(xr.grad)
    assert torch.equal(grads[0], grads[1])


def test_xgrad_uncovered_channel_is_nan_then_named():
    lams, B, L, sr, hop, M = [40.0, 128.0, 300.0], 2, 8000, 16000, 128, 32
    x, g = _inputs(B, L, 3, M, hop)
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    with torch.no_grad():
        multi(x)
        multi(x)                                              # a second observation: guards only near boundaries
    torch.cuda.synchronize()
    multi.lambd.data[1] = 1500.0                              # n_fft 16384, far from what the tracking expects; no resync()
    xr = x.clone().requires_grad_(True)
    y = multi(xr)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(y[:, 1]).all()
    assert torch.isnan(xr.grad).all()
    with pytest.raises(RuntimeError, match="channel 1"):
        multi(x.clone().requires_grad_(True))
    multi.resync()
    multi.lambd.grad = None
    lams2 = [40.0, 1500.0, 300.0]
    xr = x.clone().requires_grad_(True)
    (multi(xr) * g).sum().backward()
    ref, _, _ = _scalar_sum(lams2, x, g, M, L, sr, hop, True)
    assert torch.equal(xr.grad, ref)


def test_xgrad_captured_step_replays_eager():
    B, L, sr, hop, M = 4, 8000, 16000, 128, 32
    lams = [85.3, 128.0, 300.0]                               # channel 0 just below the 512 | 1024 boundary (85.33)
    x, g = _inputs(B, L, 3, M, hop, seed=7)
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    multi.set_tracking(8, 1)                                  # both neighbours of every channel's n_fft: three candidates each
    xr = x.clone().requires_grad_(True)
    gx_out = torch.empty_like(x)

    def step():
        y = multi(xr)
        gx, = torch.autograd.grad(y, xr, g)
        gx_out.copy_(gx)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                # eager: cold start, workspace sized for the neighbours
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = gx_out.clone()
    launches = multi._plan_for(torch.device(DEV)).last_multi_launch()
    assert [n for n, _ in launches] == [256, 512, 1024, 2048, 4096]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    gx_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gx_out, eager)
    ref, _, _ = _scalar_sum(lams, x, g, M, L, sr, hop, True)
    assert torch.equal(eager, ref)
    for k in range(3):
        assert multi.lambd_status(channel=k)["error"] == 0


def test_multi_resolution_loss():
    lams, B, L, sr, hop, M = [40.0, 128.0, 300.0], 4, 8000, 16000, 128, 64
    x_pred = torch.from_numpy(synth.waveforms(B, L, seed=11)).to(DEV)
    x_tgt = torch.from_numpy(synth.waveforms(B, L, seed=12)).to(DEV)
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    multi.lambd.requires_grad_(False)
    xp = x_pred.clone().requires_grad_(True)
    (multi(xp) - multi(x_tgt)).abs().mean().backward()       # the second forward must not change what the first one's backward covers
    # the same loss through K scalar layers: one leaf per layer, their gradients added in ascending channel order
    scal = [MelSpectrogramLayer(torch.tensor(v), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                log=True).to(DEV) for v in lams]
    for lay in scal:
        lay.lambd.requires_grad_(False)                      # the same forward kernel mode as the multi-window layer (inference)
    leaves = [x_pred.clone().requires_grad_(True) for _ in lams]
    y_p = torch.cat([lay(xk) for lay, xk in zip(scal, leaves)], dim=1)
    with torch.no_grad():
        y_t = torch.cat([lay(x_tgt) for lay in scal], dim=1)
    (y_p - y_t).abs().mean().backward()
    ref = torch.zeros_like(x_pred)
    for xk in leaves:
        ref = ref + xk.grad
    assert torch.equal(xp.grad, ref)
