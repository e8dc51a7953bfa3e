"""MultiWindowMelSpectrogram on the MI355X: every channel is the scalar layer bit for bit (forward) and to 1e-6 (lambd.grad: the two dot
reductions partition the sum differently), the fp64 oracle's bars hold, the backward is deterministic, a captured step replays the
eager lambd_sync=True steps bit for bit across an n_fft boundary, and a channel the sync-free forward did not cover is NaN and named."""
import numpy as np
import pytest
import torch

from dmel_amd import MelSpectrogramLayer, MultiWindowMelSpectrogram, synth
from oracle import dmel_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(lams, B, L, sr, hop, M, log, out_dtype=torch.float32, sync=False):
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=log, out_dtype=out_dtype, lambd_sync=sync).to(DEV)
    scal = [MelSpectrogramLayer(torch.tensor(float(v)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                log=log, out_dtype=out_dtype).to(DEV) for v in lams]
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, len(lams), M, L // hop + 1), seed=4)).to(DEV).to(out_dtype)
    return multi, scal, x, g


def _check_equal(lams, B, L, sr, hop, M, log, out_dtype=torch.float32, sync=False):
    multi, scal, x, g = _pair(lams, B, L, sr, hop, M, log, out_dtype, sync)
    y = multi(x)
    (y.float() * g.float()).sum().backward() if out_dtype == torch.float32 else y.backward(g)
    for k, lay in enumerate(scal):
        yk = lay(x)
        assert torch.equal(y[:, k:k + 1], yk), (k, lams[k])
        (yk.float() * g[:, k:k + 1].float()).sum().backward() if out_dtype == torch.float32 else yk.backward(g[:, k:k + 1].contiguous())
        d, dk = float(multi.lambd.grad[k]), float(lay.lambd.grad)
        assert abs(d - dk) <= 1e-6 * abs(dk) + 1e-12, (k, d, dk)
    return multi, x, g, y


LAM_SETS = [[128.0, 128.0, 128.0], [40.0, 128.0, 300.0], [-128.0, 85.3, 85.5], [6.0, 700.0, 2000.0]]


@pytest.mark.parametrize("lams", LAM_SETS)
@pytest.mark.parametrize("log", [False, True])
def test_equals_scalar_layer(lams, log):
    _check_equal(lams, 4, 8000, 16000, 128, 64, log)


@pytest.mark.parametrize("lams", LAM_SETS[:2])
def test_equals_scalar_layer_bf16_and_sync(lams):
    _check_equal(lams, 4, 8000, 16000, 128, 64, True, out_dtype=torch.bfloat16)
    _check_equal(lams, 4, 8000, 16000, 128, 64, True, sync=True)


def test_baseline_config2_and_long_clip():
    _check_equal([40.0, 128.0, 300.0], 256, 16000, 16000, 512, 128, True)
    _check_equal([64.0, 700.0, 2000.0], 2, 40000, 16000, 400, 40, True)        # > 32768 samples: partial sums from the prep kernel


@pytest.mark.parametrize("lams", [[40.0, 128.0, 300.0], [6.0, 700.0, 2000.0]])
def test_against_oracle(lams):
    B, L, sr, hop, M = 3, 8000, 16000, 200, 48
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True).to(DEV)
    x_np = synth.waveforms(B, L, seed=5)
    g_np = synth.cotangent((B, len(lams), M, L // hop + 1), seed=6)
    y = multi(torch.from_numpy(x_np).to(DEV))
    (y * torch.from_numpy(g_np).to(DEV)).sum().backward()
    yv = y.detach().cpu().numpy()
    for k, lam in enumerate(lams):
        y_ref, t_ref = O.forward(x_np, lam, hop, M, sr, apply_log=True)
        rel = np.abs(yv[:, k:k + 1] - y_ref) / np.maximum(np.abs(y_ref), 1.0)
        assert rel.max() <= 1e-4, (k, rel.max())
        d_ref = O.backward(np.ascontiguousarray(g_np[:, k:k + 1]), t_ref)
        mag = float(np.abs(np.ascontiguousarray(g_np[:, k:k + 1]) * t_ref).sum())
        if abs(d_ref) > 1e-3 * mag:                          # not cancellation-dominated
            assert abs(float(multi.lambd.grad[k]) - d_ref) <= 1e-4 * abs(d_ref), (k, float(multi.lambd.grad[k]), d_ref)


def test_backward_deterministic():
    multi, _, x, g = _pair([40.0, 128.0, 300.0], 8, 16000, 16000, 256, 64, True)
    grads = []
    for _ in range(2):
        multi.lambd.grad = None
        (multi(x) * g).sum().backward()
        grads.append(multi.lambd.grad.clone())
    assert torch.equal(grads[0], grads[1])


def test_k1_and_inference():
    multi, x, g, y = _check_equal([128.0], 4, 8000, 16000, 128, 64, True)
    lams = [40.0, 128.0, 300.0]
    multi, scal, x, g = _pair(lams, 4, 8000, 16000, 128, 64, True)
    y_train = multi(x).detach()
    with torch.no_grad():
        y_inf = multi(x)
        for k, lay in enumerate(scal):
            assert torch.equal(y_inf[:, k:k + 1], lay(x))
    assert (y_inf - y_train).abs().max().item() <= 2e-5


def test_captured_step_replays_eager_steps():
    B, L, sr, hop, M = 4, 8000, 16000, 128, 32
    lams = [84.0, 128.0, 300.0]                               # channel 0: n_fft 512, driven across 85.33 (1024) by the updates
    x = torch.from_numpy(synth.waveforms(B, L, seed=7)).to(DEV)
    g = -torch.ones((B, 3, M, L // hop + 1), device=DEV)      # pushes every lambd up
    steps = 12

    def make(sync):
        lay = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, lambd_sync=sync).to(DEV)
        opt = torch.optim.Adam([lay.lambd], lr=0.4, capturable=True)
        return lay, opt

    ref, opt_r = make(True)
    hist_ref = []
    for _ in range(steps):
        opt_r.zero_grad(set_to_none=False)
        y_r = ref(x)
        y_r.backward(g)
        opt_r.step()
        hist_ref.append(ref.lambd.detach().clone())
    assert capi_n(hist_ref[0][0]) == 512 and capi_n(hist_ref[-1][0]) == 1024

    lay, opt = make(False)
    y_out = torch.empty_like(y_r)

    def step():
        opt.zero_grad(set_to_none=False)
        y = lay(x)
        y.backward(g)
        y_out.copy_(y.detach())
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                 # eager warm-up = step 1 (cold start, optimizer state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(lay.lambd.detach(), hist_ref[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for i in range(1, steps):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lay.lambd.detach(), hist_ref[i]), (i, lay.lambd.detach(), hist_ref[i])
    assert torch.equal(y_out, y_r.detach())
    for k in range(3):
        assert lay.lambd_status(channel=k)["error"] == 0


def capi_n(v):
    from dmel_amd import capi
    return capi.n_fft(float(v))


def test_uncovered_channel_is_nan_and_named():
    lams = [40.0, 128.0, 300.0]
    multi, scal, x, g = _pair(lams, 2, 8000, 16000, 128, 32, True)
    with torch.no_grad():
        y0 = multi(x)
        multi(x)                                              # a second observation: guards only near boundaries
        torch.cuda.synchronize()
        multi.lambd.data[1] = 1500.0                          # far away, no resync()
        y1 = multi(x)
        torch.cuda.synchronize()
        assert torch.isnan(y1[:, 1]).all()
        assert torch.equal(y1[:, 0], y0[:, 0]) and torch.equal(y1[:, 2], y0[:, 2])
        with pytest.raises(RuntimeError, match="channel 1"):
            multi(x)
        multi.resync()
        y2 = multi(x)
        ref = MelSpectrogramLayer(torch.tensor(1500.0), n_mels=32, n_points=8000, sample_rate=16000, hop_length=128, device=DEV,
                                  optimized=True, log=True).to(DEV)
        assert torch.equal(y2[:, 1:2], ref(x)) and torch.equal(y2[:, 0], y0[:, 0])


def test_rejected_uses():
    multi, _, x, _ = _pair([40.0, 128.0], 2, 8000, 16000, 128, 32, True)
    with pytest.raises(RuntimeError):
        multi(x.clone().requires_grad_(True))
    from dmel_amd import GraphedStep, LambdAdam, SlotInput
    with pytest.raises(RuntimeError):
        multi(SlotInput(torch.zeros(1, dtype=torch.int64, device=DEV), (2, 8000)))
    with pytest.raises(ValueError):
        GraphedStep(lambda: None, [multi])
    with pytest.raises(ValueError):
        LambdAdam([multi.lambd], fused_into_backward=multi)
