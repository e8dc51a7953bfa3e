"""PCEN on the MI355X (dmel_pcen_forward / dmel_pcen_backward, dmel_amd.PCEN): the C ABI against the fp64 restatement of tests/pcen_cases.py
with the fp32 restatement's own error as the yardstick, the exact properties (silence, determinism, NULL outputs, guards, NaN containment),
PCEN behind the three mel layers against the oracle's tangent, and a captured step."""
import functools

import numpy as np
import pytest
import torch

import pcen_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QUANTITIES = ("y", "dE", "dalpha", "ddelta", "dr", "ds")
GUARD, SENTINEL = 64, -12345.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(E, g, prm, want_m=True, want_de=True, want_dp=True, eps=P.EPS):
    """the C ABI on device tensors: (y, M, dE, dparams), each with GUARD sentinel elements behind it"""
    from dmel_amd import capi
    n_mels, T = E.shape[-2], E.shape[-1]
    rows = E.numel() // T
    stream = torch.cuda.current_stream().cuda_stream
    mk = lambda n: torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)      # noqa: E731
    y, M, dE, dp = mk(E.numel()), mk(E.numel()), mk(E.numel()), mk(4 * n_mels)
    ptrs = [p.data_ptr() for p in prm]
    capi.pcen_forward(E.data_ptr(), rows, n_mels, T, *ptrs, eps, y.data_ptr(), M.data_ptr() if want_m else None, stream)
    if g is not None:
        # the backward reads the smoother: its own forward's, whether or not this call was asked to keep one
        Mk = M
        if not want_m:
            Mk = mk(E.numel())
            capi.pcen_forward(E.data_ptr(), rows, n_mels, T, *ptrs, eps, mk(E.numel()).data_ptr(), Mk.data_ptr(), stream)
        scratch = torch.empty(max(capi.pcen_scratch_bytes(rows) // 4, 4), dtype=torch.float32, device=DEV)
        capi.pcen_backward(g.data_ptr(), E.data_ptr(), Mk.data_ptr(), rows, n_mels, T, *ptrs, eps, dE.data_ptr() if want_de else None,
                           dp.data_ptr() if want_dp else None, scratch.data_ptr() if want_dp else None, stream)
    torch.cuda.synchronize()
    return y, M, dE, dp


@functools.lru_cache(maxsize=None)
def _case(idx):
    """inputs, both restatements and one run of the kernels for SHAPES[idx] (computed once, shared)"""
    shape = P.SHAPES[idx]
    E, g = P.inputs(shape, idx)
    prm = P.params(shape[-2], idx)
    ref = P.backward(g.double(), E.double(), *[p.double() for p in prm])
    r32 = P.backward(g, E, *prm)
    Ed, gd, prmd = E.to(DEV), g.to(DEV), [p.to(DEV) for p in prm]
    out = _call(Ed, gd, prmd)
    return dict(shape=shape, E=Ed, g=gd, prm=prmd, ref=ref, r32=r32, out=out, Ecpu=E)


def _unpack(c, out):
    n, M = c["E"].numel(), c["shape"][-2]
    y, Mm, dE, dp = (t.cpu() for t in out)
    got = {"y": y[:n].reshape(c["shape"]), "M": Mm[:n].reshape(c["shape"]), "dE": dE[:n].reshape(c["shape"])}
    for i, k in enumerate(("dalpha", "ddelta", "dr", "ds")):
        got[k] = dp[i * M:(i + 1) * M]
    guards = [y[n:], Mm[n:], dE[n:], dp[4 * M:]]
    return got, guards


@pytest.mark.parametrize("idx", range(len(P.SHAPES)), ids=[str(s) for s in P.SHAPES])
def test_c_abi_against_fp64_within_eight_times_the_fp32_restatement(idx):
    """Errors in units of the cancellation-free scales of pcen_cases.backward.  On every shape and for each of y, dE and the four parameter
    gradients the kernel is allowed 8 x the worst error of the fp32 torch restatement (sequential scan, torch.pow) on that shape's inputs,
    and never more than 1e-4.
    Measured on an MI355X, worst ratio kernel / restatement over the eleven shapes: y 1.94, dE 1.68, d alpha 2.42, d delta 2.12, d r 5.25 at
    (2, 3, 63), d s 2.09; largest kernel errors: y 6.6e-7, dE 8.9e-7, d alpha 2.1e-7, d delta 2.3e-7, d r 2.3e-7, d s 4.0e-7."""
    c = _case(idx)
    got, _ = _unpack(c, c["out"])
    failed = []
    for k in QUANTITIES:
        scale = c["ref"][k + "_scale"]
        w_kernel = P.worst(got[k], c["ref"][k], scale)
        w_fp32 = P.worst(c["r32"][k], c["ref"][k], scale)
        bound = min(8.0 * w_fp32, 1e-4)
        print(f"pcen {c['shape']} {k}: kernel {w_kernel:.3e} fp32 restatement {w_fp32:.3e} ratio {w_kernel / w_fp32 if w_fp32 else float('nan'):.2f} bound {bound:.3e}")
        if not w_kernel <= bound:
            failed.append((k, w_kernel, w_fp32))
    assert not failed, (c["shape"], failed)
    # the smoother the backward reads: against fp64 in units of itself (every term of M is >= 0)
    assert P.worst(got["M"], c["ref"]["M"], c["ref"]["M"]) <= 1e-4


@pytest.mark.parametrize("idx", range(len(P.SHAPES)), ids=[str(s) for s in P.SHAPES])
def test_exact_properties(idx):
    c = _case(idx)
    shape, T = c["shape"], c["shape"][-1]
    got, guards = _unpack(c, c["out"])
    # silence is +0.0 bit for bit
    y2 = got["y"].reshape(-1, T)
    assert bool((_bits(y2[0]) == 0).all()) and bool((_bits(y2[-1, T // 3:]) == 0).all())
    assert bool((_bits(got["y"])[c["Ecpu"] == 0] == 0).all())
    # guards behind y, M, dE, dparams
    for name, gd in zip(("y", "M", "dE", "dparams"), guards):
        assert gd.numel() == GUARD and bool((gd == SENTINEL).all()), name
    # a second run gives the same bits
    again = _call(c["E"], c["g"], c["prm"])
    for a, b in zip(c["out"], again):
        assert torch.equal(_bits(a), _bits(b))
    # NULL outputs: the other one keeps its bits, nothing else is written
    y, M, dE, dp = c["out"]
    y1, M1, dE1, dp1 = _call(c["E"], c["g"], c["prm"], want_m=False, want_de=False)
    assert torch.equal(_bits(y1), _bits(y)) and bool((M1 == SENTINEL).all()) and bool((dE1 == SENTINEL).all()) and torch.equal(_bits(dp1), _bits(dp))
    y2_, M2, dE2, dp2 = _call(c["E"], c["g"], c["prm"], want_dp=False)
    assert torch.equal(_bits(M2), _bits(M)) and torch.equal(_bits(dE2), _bits(dE)) and bool((dp2 == SENTINEL).all())


@pytest.mark.parametrize("idx", [2, 3, 7, 10], ids=lambda i: str(P.SHAPES[i]))
def test_nan_stays_in_its_row_and_band(idx):
    c = _case(idx)
    shape, n_mels, T = c["shape"], c["shape"][-2], c["shape"][-1]
    rows = c["E"].numel() // T
    bad = rows // 2
    E = c["E"].clone().reshape(rows, T)
    E[bad, T // 2] = float("nan")
    y, M, dE, dp = _call(E.reshape(shape), c["g"], c["prm"])
    y0, M0, dE0, dp0 = c["out"]
    n = rows * T
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[bad] = False
    for a, b in ((y, y0), (M, M0), (dE, dE0)):
        assert torch.equal(_bits(a[:n].reshape(rows, T)[keep]), _bits(b[:n].reshape(rows, T)[keep]))
    assert bool(torch.isnan(y[:n].reshape(rows, T)[bad, T // 2:]).all())
    bands = torch.ones(n_mels, dtype=torch.bool, device=DEV)
    bands[bad % n_mels] = False
    got, clean = dp[:4 * n_mels].reshape(4, n_mels), dp0[:4 * n_mels].reshape(4, n_mels)
    assert torch.equal(_bits(got[:, bands]), _bits(clean[:, bands]))
    assert bool(torch.isfinite(clean).all())


# ---- through the layers ------------------------------------------------------------------------------------------------------------
SR, M_L, B_L = 16000, 8, 3
CONFIGS = [(10.0, 2000, 100), (128.0, 4000, 50)]           # (lambd -> n_fft 64 / 1024, n_points, hop): 21 and 81 frames


def _pcen(seed=0):
    import dmel_amd
    m = dmel_amd.PCEN(M_L)
    with torch.no_grad():
        for p, v in zip((m.alpha, m.delta, m.r, m.s), P.params(M_L, 50 + seed)):
            p.copy_(v)
        m.alpha[0], m.delta[0], m.r[0], m.s[0] = 0.9, 1.0, 0.5, 0.05        # (band 0 off the closed ends: every parameter has a gradient)
    return m.to(DEV)


def _x(L, seed=3):
    from dmel_amd import synth
    return synth.waveforms(B_L, L, seed=seed)


def _ref_dlambd(mels, tangents, pcen, g):
    """sum dE64 * tangent64 and sum |dE64 * tangent64| per window width; mels / tangents: (K, B, C, M, T) pieces that add up to the image"""
    prm = [p.detach().cpu().double() for p in (pcen.alpha, pcen.delta, pcen.r, pcen.s)]
    E = torch.from_numpy(np.sum(mels, axis=0)).double().requires_grad_(True)
    y, _ = P.forward(E, *prm, eps=pcen.eps)
    (dE,) = torch.autograd.grad((y * g.double()).sum(), [E])
    out = []
    for t in tangents:
        prod = dE * torch.from_numpy(t).double()
        out.append((float(prod.sum()), float(prod.abs().sum())))
    return out


def _check_dlambd(name, grad, refs):
    for k, (d_ref, mag) in enumerate(refs):
        d = float(grad.reshape(-1)[k])
        print(f"pcen behind {name} k={k}: d={d!r} d_ref={d_ref!r} |d - d_ref| / sum|dE t| = {abs(d - d_ref) / mag:.3e}")
        assert abs(d - d_ref) <= 1e-4 * mag, (name, k, d, d_ref, mag)


@pytest.mark.parametrize("lam,L,hop", CONFIGS, ids=["nfft64", "nfft1024"])
def test_behind_the_scalar_layer_against_the_oracle(lam, L, hop):
    from dmel_amd import MelSpectrogramLayer
    from oracle import dmel_oracle as O
    x_np = _x(L)
    T = L // hop + 1
    g = torch.randn(B_L, 1, M_L, T, generator=torch.Generator().manual_seed(1))
    lay = MelSpectrogramLayer(torch.tensor(lam), n_mels=M_L, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True).to(DEV)
    pcen = _pcen()
    y = pcen(lay(torch.from_numpy(x_np).to(DEV)))
    assert y.shape == (B_L, 1, M_L, T) and y.dtype == torch.float32
    (y * g.to(DEV)).sum().backward()
    mel, tan = O.forward(x_np, lam, hop, M_L, SR)
    _check_dlambd("MelSpectrogramLayer", lay.lambd.grad, _ref_dlambd([mel], [tan], pcen, g))
    y_ref, _ = P.forward(torch.from_numpy(mel).double(), *[p.detach().cpu().double() for p in pcen.parameters()], eps=pcen.eps)
    assert float((y.detach().cpu().double() - y_ref).abs().max()) <= 1e-4 * float(y_ref.abs().max())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in pcen.parameters())


def test_behind_the_multi_window_and_band_split_layers_against_the_oracle():
    from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram
    from oracle import dmel_oracle as O
    lams, L, hop = [10.0, 40.0, 128.0], 4000, 50
    x_np = _x(L)
    T = L // hop + 1
    x = torch.from_numpy(x_np).to(DEV)
    both = [O.forward(x_np, lam, hop, M_L, SR) for lam in lams]
    # K output channels
    g = torch.randn(B_L, 3, M_L, T, generator=torch.Generator().manual_seed(2))
    multi, pcen = MultiWindowMelSpectrogram(lams, M_L, L, SR, hop_length=hop).to(DEV), _pcen(1)
    (pcen(multi(x)) * g.to(DEV)).sum().backward()
    mels, tans = [], []
    for k, (mel, tan) in enumerate(both):
        for src, dst in ((mel, mels), (tan, tans)):
            full = np.zeros((B_L, 3, M_L, T), src.dtype)
            full[:, k] = src[:, 0]
            dst.append(full)
    _check_dlambd("MultiWindowMelSpectrogram", multi.lambd.grad, _ref_dlambd(mels, tans, pcen, g))
    # one image, a window width per band group
    g = torch.randn(B_L, 1, M_L, T, generator=torch.Generator().manual_seed(3))
    band, pcen = BandSplitMelSpectrogram(lams, M_L, L, SR, hop_length=hop).to(DEV), _pcen(2)
    (pcen(band(x)) * g.to(DEV)).sum().backward()
    edges = [(k * M_L) // 3 for k in range(4)]
    mels, tans = [], []
    for k, (mel, tan) in enumerate(both):
        for src, dst in ((mel, mels), (tan, tans)):
            full = np.zeros_like(src)
            full[:, :, edges[k]:edges[k + 1]] = src[:, :, edges[k]:edges[k + 1]]
            dst.append(full)
    _check_dlambd("BandSplitMelSpectrogram", band.lambd.grad, _ref_dlambd(mels, tans, pcen, g))


def test_lengths_pad_frames_are_exactly_zero():
    from dmel_amd import MelSpectrogramLayer
    lam, L, hop = CONFIGS[1]
    T = L // hop + 1
    lay = MelSpectrogramLayer(torch.tensor(lam), n_mels=M_L, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True).to(DEV)
    pcen = _pcen()
    lengths = torch.tensor([L, 1234, 50], dtype=torch.int32, device=DEV)
    y = pcen(lay(torch.from_numpy(_x(L)).to(DEV), lengths))
    (y * torch.randn_like(y)).sum().backward()
    for b, n in enumerate(lengths.tolist()):
        pad = y[b, :, :, n // hop + 1:]
        assert bool((_bits(pad) == 0).all()), b
        assert bool((y[b, :, :, :n // hop + 1] != 0).any())
    assert bool(torch.isfinite(lay.lambd.grad).all()) and float(lay.lambd.grad.abs()) > 0


@pytest.mark.parametrize("kind", ["waveform", "filterbank"])
def test_waveform_and_filterbank_gradients_flow(kind):
    from dmel_amd import MelSpectrogramLayer
    lam, L, hop = CONFIGS[0]
    T = L // hop + 1
    lay = MelSpectrogramLayer(torch.tensor(lam), n_mels=M_L, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True,
                              learnable_fb=(kind == "filterbank")).to(DEV)
    pcen = _pcen()
    grads = []
    for seed in (4, 5):
        x = torch.from_numpy(_x(L)).to(DEV).requires_grad_(kind == "waveform")
        lay.zero_grad()
        g = torch.randn(B_L, 1, M_L, T, generator=torch.Generator().manual_seed(seed)).to(DEV)
        (pcen(lay(x)) * g).sum().backward()
        grads.append((x.grad if kind == "waveform" else lay.mel_fb.grad).detach().clone())
    assert all(bool(torch.isfinite(v).all()) and bool((v != 0).any()) for v in grads)
    assert not torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("opt_name", ["adam", "lambd_adam"])
def test_one_optimizer_step_moves_all_four_parameters(opt_name):
    import dmel_amd
    lam, L, hop = CONFIGS[0]
    lay = dmel_amd.MelSpectrogramLayer(torch.tensor(lam), n_mels=M_L, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True).to(DEV)
    pcen = _pcen()
    before = [p.detach().clone() for p in pcen.parameters()]
    opt = (torch.optim.Adam if opt_name == "adam" else dmel_amd.LambdAdam)(list(pcen.parameters()), lr=1e-2)
    y = pcen(lay(torch.from_numpy(_x(L)).to(DEV)))
    (y * torch.randn_like(y)).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    for p, b in zip(pcen.parameters(), before):
        assert bool(torch.isfinite(p).all()) and bool((p != b).all())
    pcen.project_()
    assert bool((pcen.alpha <= 1).all()) and bool((pcen.alpha >= 0).all()) and bool((pcen.delta >= 1e-3).all())
    assert bool((pcen.r > 0).all()) and bool((pcen.r <= 1).all()) and bool((pcen.s >= 1e-3).all()) and bool((pcen.s <= 1).all())


def test_captured_step_replays_the_eager_bits():
    from dmel_amd import MelSpectrogramLayer
    lam, L, hop = CONFIGS[1]
    T = L // hop + 1
    lay = MelSpectrogramLayer(torch.tensor(lam), n_mels=M_L, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True).to(DEV)
    pcen = _pcen()
    x = torch.from_numpy(_x(L)).to(DEV)
    g = torch.randn(B_L, 1, M_L, T, device=DEV)
    params = [lay.lambd] + list(pcen.parameters())

    def step():
        y = pcen(lay(x))
        return y, torch.autograd.grad((y * g).sum(), params)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            y_e, grads_e = step()                               # warm-up: plans, allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [t.detach().clone() for t in (y_e, *grads_e)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, grads_c = step()
    for _ in range(2):
        for t in (y_c, *grads_c):
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, (y_c, *grads_c)):
            assert torch.equal(_bits(a), _bits(b.detach()))
