"""BandSplitMelSpectrogram on the MI355X: rows e_k ... e_{k+1} - 1 of the one image (and of its tangent) are the scalar layer's for lambd[k]
bit for bit, lambd.grad[k] is the scalar layer's for the cotangent masked to the group (1e-6: the two fp64 reductions partition the sum
differently), the fp64 oracle's bars hold without the cancellation exemption, the backward is deterministic, two launches that write into
the one image do not touch each other's rows, an uncovered channel poisons ITS rows only, a captured step replays the eager
lambd_sync=True steps across an n_fft boundary, and the layer drops into the shipped nets."""
import numpy as np
import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, capi, synth
from oracle import dmel_oracle as O
from test_hip_parity import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LAM_SETS = [[128.0, 128.0, 128.0], [300.0, 128.0, 40.0], [40.0, 128.0, 300.0], [-128.0, 85.3, 85.5], [2000.0, 700.0, 6.0]]
K8 = [2000.0, 700.0, 300.0, 200.0, 128.0, 85.4, 40.0, 6.0]
UNEVEN = {1: [], 3: [[0, 5, 30, 64], [0, 5, 6, 64]], 8: [[0, 1, 6, 11, 30, 31, 47, 50, 64]]}      # not multiples of 4 or 16; one-row groups

_SCALAR = {}


def _scalar(lam, shape, log, out_dtype, x, g=None):
    """the scalar layer's output for lambd = lam in grad mode and under no_grad (cached), and its lambd.grad for the cotangent g"""
    B, L, sr, hop, M = shape
    key = (float(lam), shape, bool(log), out_dtype)
    if key not in _SCALAR:
        lay = MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                  log=log, out_dtype=out_dtype).to(DEV)
        with torch.no_grad():
            y_inf = lay(x)
        _SCALAR[key] = (lay, lay(x).detach(), y_inf)
    lay, y_train, y_inf = _SCALAR[key]
    d = None
    if g is not None:
        lay.lambd.grad = None
        y = lay(x)
        (y.float() * g.float()).sum().backward() if out_dtype == torch.float32 else y.backward(g.contiguous())
        d = float(lay.lambd.grad)
    return y_train, y_inf, d


def _edges(lams, M, edges):
    K = len(lams)
    return list(edges) if edges is not None else [(k * M) // K for k in range(K + 1)]


def _check(lams, edges, shape, log, out_dtype=torch.float32, sync=False, seed=3):
    """tests 1 and 2 for one layer: rows (grad mode and no_grad) and lambd.grad against the scalar layers"""
    B, L, sr, hop, M = shape
    lay = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, band_edges=edges, log=log, out_dtype=out_dtype, lambd_sync=sync).to(DEV)
    e = _edges(lams, M, edges)
    assert list(lay.band_edges) == e
    x = torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, 1, M, L // hop + 1), seed=seed + 1)).to(DEV).to(out_dtype)
    y = lay(x)
    assert y.shape == (B, 1, M, L // hop + 1) and y.dtype == out_dtype
    (y.float() * g.float()).sum().backward() if out_dtype == torch.float32 else y.backward(g)
    with torch.no_grad():
        y_inf = lay(x)
    for k, lam in enumerate(lams):
        gk = torch.zeros_like(g)
        gk[:, :, e[k]:e[k + 1]] = g[:, :, e[k]:e[k + 1]]
        yk, yk_inf, dk = _scalar(lam, shape, log, out_dtype, x, gk)
        assert torch.equal(y[:, :, e[k]:e[k + 1]], yk[:, :, e[k]:e[k + 1]]), ("train", k, lam, e)
        assert torch.equal(y_inf[:, :, e[k]:e[k + 1]], yk_inf[:, :, e[k]:e[k + 1]]), ("no_grad", k, lam, e)
        d = float(lay.lambd.grad[k])
        print(f"band_split grad lams={lams} edges={e} log={log} {out_dtype} sync={sync} k={k}: d={d!r} d_k={dk!r}")
        assert abs(d - dk) <= 1e-6 * abs(dk) + 1e-12, (k, d, dk)
    return lay, x, g, y


SHAPE = (4, 8000, 16000, 128, 64)


@pytest.mark.parametrize("lams", LAM_SETS + [[128.0], K8])
@pytest.mark.parametrize("log", [False, True])
def test_rows_equal_scalar_layer(lams, log):
    for edges in [None] + UNEVEN[len(lams)]:
        for out_dtype in (torch.float32, torch.bfloat16):
            for sync in (False, True):
                _check(lams, edges, SHAPE, log, out_dtype, sync)


def test_baseline_config2_and_long_clip():
    _check([300.0, 128.0, 40.0], None, (256, 16000, 16000, 512, 128), True)
    _check([2000.0, 700.0, 64.0], None, (2, 40000, 16000, 400, 40), True)        # > 32768 samples: partial sums from the prep kernel


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("log", [False, True])
def test_tangent_rows_through_the_c_abi(dev, log):
    """dmel_forward_band(_dev) against dmel_forward per channel: out AND tangent rows, bit for bit (the gradient test rests on it)"""
    B, L, sr, hop, M = SHAPE
    T = L // hop + 1
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    for lams, e in (([300.0, 128.0, 40.0], [0, 5, 30, 64]), ([2000.0, 700.0, 6.0], [0, 21, 42, 64]), ([128.0, 128.0, 128.0], [0, 5, 6, 64])):
        plan = capi.Plan(L, hop, M, sr)
        out = torch.full((B, 1, M, T), 7.0, device=DEV)
        tan = torch.full((B, 1, M, T), 7.0, device=DEV)
        scratch = torch.zeros((plan.scratch_bytes_multi(B, len(lams)),), dtype=torch.uint8, device=DEV)
        if dev:
            lam_d = torch.tensor(lams, device=DEV)
            plan.forward_band_dev(x.data_ptr(), B, lam_d.data_ptr(), e, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr())
        else:
            plan.forward_band(x.data_ptr(), B, lams, e, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr())
        ref_plan = capi.Plan(L, hop, M, sr)
        for k, lam in enumerate(lams):
            o_k, t_k = torch.empty_like(out), torch.empty_like(tan)
            ref_plan.forward(x.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), log, 1e-10, st)
            torch.cuda.synchronize()
            assert torch.equal(out[:, :, e[k]:e[k + 1]], o_k[:, :, e[k]:e[k + 1]]), (lams, k)
            assert torch.equal(tan[:, :, e[k]:e[k + 1]], t_k[:, :, e[k]:e[k + 1]]), (lams, k)


ORACLE_CASES = [([300.0, 128.0, 40.0], [0, 16, 32, 48]), ([300.0, 128.0, 40.0], [0, 5, 30, 48]), ([2000.0, 700.0, 6.0], [0, 16, 32, 48]),
                ([700.0, 300.0, 128.0, 40.0], [0, 12, 24, 36, 48])]


@pytest.mark.parametrize("lams,edges", ORACLE_CASES)
@pytest.mark.parametrize("log", [False, True])
def test_against_oracle(lams, edges, log):
    """26 groups in all.  Output: relative error <= 1e-4 on every element (linear: assert_parity without the floor; log: |dy| / max(|y|, 1)).
    Gradient: |d - d_ref| <= 1e-4 |d_ref|.  The project exempts cancellation-dominated sums (|d_ref| <= 1e-3 sum|g t|); on these groups the
    oracle alone gives |d_ref| / sum|g t| between 4.1e-3 and 6.1e-2, so the exemption must never be taken: asserted."""
    B, L, sr, hop, M = 3, 8000, 16000, 200, 48
    lay = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, band_edges=edges, log=log).to(DEV)
    x_np = synth.waveforms(B, L, seed=5)
    g_np = synth.cotangent((B, 1, M, L // hop + 1), seed=6)
    y = lay(torch.from_numpy(x_np).to(DEV))
    (y * torch.from_numpy(g_np).to(DEV)).sum().backward()
    yv = y.detach().cpu().numpy()
    for k, lam in enumerate(lams):
        lo, hi = edges[k], edges[k + 1]
        y_ref, t_ref = O.forward(x_np, lam, hop, M, sr, apply_log=log)
        if log:
            rel = np.abs(yv[:, :, lo:hi] - y_ref[:, :, lo:hi]) / np.maximum(np.abs(y_ref[:, :, lo:hi]), 1.0)
            print(f"band_split oracle lams={lams} edges={edges} log k={k}: max rel {rel.max():.3e}")
            assert rel.max() <= 1e-4, (k, rel.max())
        else:
            assert_parity(f"band_split/{lams}/{edges}/k{k}/mel", yv[:, :, lo:hi], y_ref[:, :, lo:hi], allow_floor=False)
        gk = np.zeros_like(g_np)
        gk[:, :, lo:hi] = g_np[:, :, lo:hi]
        d_ref = O.backward(gk, t_ref)
        mag = float(np.abs(gk * t_ref).sum())
        d = float(lay.lambd.grad[k])
        print(f"band_split oracle lams={lams} edges={edges} log={log} k={k}: d={d!r} d_ref={d_ref!r} |d_ref|/sum|g t|={abs(d_ref) / mag:.3e}")
        assert abs(d_ref) > 1e-3 * mag, ("the cancellation exemption would be taken", k, d_ref, mag)
        assert abs(d - d_ref) <= 1e-4 * abs(d_ref), (k, d, d_ref)


def test_backward_deterministic_and_accumulates():
    B, L, sr, hop, M = 8, 16000, 16000, 256, 64
    lay = BandSplitMelSpectrogram([300.0, 128.0, 40.0], M, L, sr, hop_length=hop, band_edges=[0, 5, 30, 64], log=True).to(DEV)
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, 1, M, L // hop + 1), seed=4)).to(DEV)
    grads = []
    for _ in range(2):
        lay.lambd.grad = None
        (lay(x) * g).sum().backward()
        grads.append(lay.lambd.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert (grads[0] != 0).all()
    # accumulate through the C ABI: a second dmel_backward_band onto the first one's result
    plan = capi.Plan(L, hop, M, sr)
    T = L // hop + 1
    e = [0, 5, 30, 64]
    st = torch.cuda.current_stream().cuda_stream
    out, tan = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
    scratch = torch.zeros((plan.scratch_bytes_multi(B, 3),), dtype=torch.uint8, device=DEV)
    plan.forward_band(x.data_ptr(), B, [300.0, 128.0, 40.0], e, out.data_ptr(), tan.data_ptr(), True, 1e-10, st, scratch.data_ptr())
    dl = torch.zeros(3, device=DEV)
    plan.backward_band(g.data_ptr(), tan.data_ptr(), B, e, dl.data_ptr(), st, scratch.data_ptr())
    once = dl.clone()
    assert torch.equal(once, grads[0])
    plan.backward_band(g.data_ptr(), tan.data_ptr(), B, e, dl.data_ptr(), st, scratch.data_ptr(), accumulate=True)
    torch.cuda.synchronize()
    # (the kernel adds its fp64 total to the fp32 value already there and rounds once: within an ulp of twice the rounded value)
    assert torch.allclose(dl, 2 * once, rtol=2.0 ** -22, atol=0.0), (dl, once)


def test_groups_do_not_touch_each_other():
    """channels 0 and 2 share n_fft 1024, channel 1 has 2048: two launches write into the one image"""
    B, L, sr, hop, M = SHAPE
    T = L // hop + 1
    lams, e = [128.0, 300.0, 100.0], [0, 5, 30, 64]
    assert capi.n_fft(128.0) == capi.n_fft(100.0) == 1024 and capi.n_fft(300.0) == 2048
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    sentinel = -12345.5
    for dev in (False, True):
        plan = capi.Plan(L, hop, M, sr)
        out = torch.full((B, 1, M, T), sentinel, device=DEV)
        tan = torch.full((B, 1, M, T), sentinel, device=DEV)
        scratch = torch.zeros((plan.scratch_bytes_multi(B, 3),), dtype=torch.uint8, device=DEV)
        if dev:
            lam_d = torch.tensor(lams, device=DEV)
            plan.forward_band_dev(x.data_ptr(), B, lam_d.data_ptr(), e, out.data_ptr(), tan.data_ptr(), True, 1e-10, st, scratch.data_ptr())
        else:
            plan.forward_band(x.data_ptr(), B, lams, e, out.data_ptr(), tan.data_ptr(), True, 1e-10, st, scratch.data_ptr())
        torch.cuda.synchronize()
        # (host values: one launch per distinct n_fft; device values, cold start: plus the guard launches of the neighbouring sizes, which return at once)
        assert len(plan.last_multi_launch()) == 2 if not dev else len(plan.last_multi_launch()) >= 2
        assert not (out == sentinel).any() and not (tan == sentinel).any()
        ref_plan = capi.Plan(L, hop, M, sr)
        for k, lam in enumerate(lams):
            o_k, t_k = torch.empty_like(out), torch.empty_like(tan)
            ref_plan.forward(x.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), True, 1e-10, st)
            torch.cuda.synchronize()
            assert torch.equal(out[:, :, e[k]:e[k + 1]], o_k[:, :, e[k]:e[k + 1]]) and torch.equal(tan[:, :, e[k]:e[k + 1]], t_k[:, :, e[k]:e[k + 1]])

    # sync-free layer, lambd[1] moved far away without resync(): ITS rows are NaN, the others are the previous forward's
    lay = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, band_edges=e, log=True).to(DEV)
    with torch.no_grad():
        y0 = lay(x)
        lay(x)                                                # a second observation: guards only near boundaries
        torch.cuda.synchronize()
        lay.lambd.data[1] = 6.0
        y1 = lay(x)
        torch.cuda.synchronize()
        assert torch.isnan(y1[:, :, e[1]:e[2]]).all()
        assert torch.equal(y1[:, :, :e[1]], y0[:, :, :e[1]]) and torch.equal(y1[:, :, e[2]:], y0[:, :, e[2]:])
        with pytest.raises(RuntimeError, match="channel 1"):
            lay(x)
        lay.resync()
        y2 = lay(x)
        ref = MelSpectrogramLayer(torch.tensor(6.0), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                  log=True).to(DEV)
        assert torch.equal(y2[:, :, e[1]:e[2]], ref(x)[:, :, e[1]:e[2]]) and torch.equal(y2[:, :, :e[1]], y0[:, :, :e[1]])
        assert torch.equal(y2[:, :, e[2]:], y0[:, :, e[2]:])


def test_captured_step_replays_eager_steps():
    B, L, sr, hop, M = 4, 8000, 16000, 128, 32
    lams = [84.0, 128.0, 300.0]                               # channel 0: n_fft 512, driven across 85.33 (1024) by the updates
    x = torch.from_numpy(synth.waveforms(B, L, seed=7)).to(DEV)
    g = -torch.ones((B, 1, M, L // hop + 1), device=DEV)      # pushes every lambd up
    steps = 12

    def make(sync):
        lay = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, lambd_sync=sync).to(DEV)
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
    assert capi.n_fft(float(hist_ref[0][0])) == 512 and capi.n_fft(float(hist_ref[-1][0])) == 1024

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


@pytest.mark.parametrize("which", ["conv", "panns"])
def test_drop_in(which):
    from dmel_amd import nets, panns
    torch.manual_seed(0)
    B, L, sr, hop, M = 4, 8000, 16000, 128, 64
    if which == "conv":
        net = nets.MelConvNet(10, torch.tensor(128.0), DEV, M, sr, L, hop_length=hop, optimized=True, energy_normalize=True).to(DEV)
    else:
        net = panns.MelPANNsNet(10, torch.tensor(128.0), DEV, M, sr, L, hop_length=hop, optimized=True, energy_normalize=True).to(DEV)
    lam0 = [300.0, 128.0, 40.0]
    net.spectrogram_layer = BandSplitMelSpectrogram(lam0, M, L, sr, hop_length=hop, log=True).to(DEV)
    opt = nets.make_optimizer(net, lr_model=1e-3, lr_tf=0.5)
    assert [g["lr"] for g, (n, _) in zip(opt.param_groups, net.named_parameters()) if n == "spectrogram_layer.lambd"] == [0.5]
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    target = torch.arange(B, device=DEV) % 10
    opt.zero_grad()
    logits, s = net(x)
    assert s.shape == (B, 1, M, L // hop + 1)
    torch.nn.functional.cross_entropy(logits, target).backward()
    grad = net.spectrogram_layer.lambd.grad
    assert torch.isfinite(logits).all() and torch.isfinite(grad).all() and (grad != 0).all(), grad
    opt.step()
    moved = net.spectrogram_layer.lambd.detach().cpu() - torch.tensor(lam0)
    assert (moved != 0).all() and (moved.abs() <= 0.5 * 1.001).all(), moved      # Adam's first step: lr_tf per parameter


def test_rejected_uses():
    B, L, sr, hop, M = 2, 8000, 16000, 128, 32
    lay = BandSplitMelSpectrogram([128.0, 40.0], M, L, sr, hop_length=hop, log=True).to(DEV)
    x = torch.from_numpy(synth.waveforms(B, L, seed=3)).to(DEV)
    with pytest.raises(RuntimeError, match="waveform gradient"):
        lay(x.clone().requires_grad_(True))
    from dmel_amd import GraphedStep, LambdAdam, SlotInput
    with pytest.raises(RuntimeError, match="SlotInput"):
        lay(SlotInput(torch.zeros(1, dtype=torch.int64, device=DEV), (B, L)))
    with pytest.raises(RuntimeError, match="lengths"):
        lay(x, lengths=torch.full((B,), L, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        lay(x[0])
    with pytest.raises(RuntimeError, match="n_points"):
        lay(x[:, :4000])
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        lay(x.cpu())
    with pytest.raises(ValueError, match="BandSplitMelSpectrogram"):
        GraphedStep(lambda: None, [lay])
    with pytest.raises(ValueError, match="BandSplitMelSpectrogram"):
        LambdAdam([lay.lambd], fused_into_backward=lay)
    # the C ABI refuses edges that do not end at the plan's n_mels
    plan = capi.Plan(L, hop, M, sr)
    with pytest.raises(capi.DmelError):
        plan.forward_band(x.data_ptr(), B, [128.0, 40.0], [0, 16, 31], x.data_ptr(), None, True, 1e-10, 0, x.data_ptr())
