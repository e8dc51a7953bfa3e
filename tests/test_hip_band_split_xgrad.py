"""BandSplitMelSpectrogram(waveform_grad=True) on the MI355X.  With band edges e_0 ... e_K and G_k the (B, 1, M, T) cotangent whose rows
outside [e_k, e_{k+1}) are +0.0, x.grad equals bit for bit (a) zeros + gx_0 + gx_1 + ... over the K scalar layers on G_k and (b) what
MultiWindowMelSpectrogram(waveform_grad=True) gives for the stacked G_k: on the wave-FFT and LDS paths, at edges where the row masks can go
wrong, over all-zero HTK rows, in bf16 / lambd_sync / inference mode, with the prep kernel's window, for a cotangent at an unaligned
address, deterministically, for an uncovered channel (NaN, then named) and inside a captured step; it meets the fp64 oracle's bar; the
output and lambd.grad are the plain band layer's; the default layer still refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, capi, synth
from oracle import dmel_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM_SETS = [[128.0, 128.0, 128.0], [300.0, 128.0, 40.0], [-128.0, 85.3, 85.5], [2000.0, 700.0, 6.0]]
SHAPE = dict(B=4, L=8000, sr=16000, hop=128, M=64)


def _edges(K, M, edges=None):
    return list(edges) if edges is not None else [(k * M) // K for k in range(K + 1)]


def _inputs(B, L, M, hop, seed=3, dtype=torch.float32):
    x = torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, 1, M, L // hop + 1), seed=seed + 1)).to(DEV).to(dtype)
    return x, g


def _masked(g, edges):
    """[G_0, ..., G_{K-1}]: zeros_like + slice assignment, so that the rows outside a group are POSITIVE zeros"""
    out = []
    for lo, hi in zip(edges, edges[1:]):
        gk = torch.zeros_like(g)
        gk[:, :, lo:hi] = g[:, :, lo:hi]
        out.append(gk)
    return out


def _backward(y, g, out_dtype):
    if out_dtype == torch.float32:
        (y * g).sum().backward()
    else:
        y.backward(g)


def _band(lams, edges, x, g, M, L, sr, hop, log, out_dtype=torch.float32, sync=False, normalize=False, lambd_grad=True, waveform_grad=True):
    band = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, normalize_window=normalize, band_edges=edges, log=log, out_dtype=out_dtype,
                                   lambd_sync=sync, waveform_grad=waveform_grad).to(DEV)
    band.lambd.requires_grad_(lambd_grad)
    xr = x.detach().clone().requires_grad_(waveform_grad)
    y = band(xr)
    if lambd_grad or waveform_grad:
        _backward(y, g, out_dtype)
    return band, y.detach(), xr.grad


def _scalar_sum(lams, gks, x, M, L, sr, hop, log, out_dtype=torch.float32, normalize=False, lambd_grad=True):
    """zeros + gx_0 + gx_1 + ...: the K scalar layers on the masked cotangents, added in ascending channel order; outputs and lambd.grad"""
    acc = torch.zeros_like(x)
    ys, dls = [], []
    for v, gk in zip(lams, gks):
        lay = MelSpectrogramLayer(torch.tensor(float(v)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                  normalize_window=normalize, log=log, out_dtype=out_dtype).to(DEV)
        lay.lambd.requires_grad_(lambd_grad)
        xk = x.detach().clone().requires_grad_(True)
        yk = lay(xk)
        _backward(yk, gk, out_dtype)
        acc = acc + xk.grad
        ys.append(yk.detach())
        dls.append(None if lay.lambd.grad is None else float(lay.lambd.grad))
    return acc, ys, dls


def _multi_grad(lams, gks, x, M, L, sr, hop, log, out_dtype=torch.float32, normalize=False, lambd_grad=True):
    multi = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, normalize_window=normalize, log=log, out_dtype=out_dtype,
                                      waveform_grad=True).to(DEV)
    multi.lambd.requires_grad_(lambd_grad)
    xr = x.detach().clone().requires_grad_(True)
    _backward(multi(xr), torch.cat(gks, dim=1), out_dtype)
    return xr.grad


def _check(lams, B, L, sr, hop, M, log, edges=None, seed=3, **kw):
    edges = _edges(len(lams), M, edges)
    dtype = kw.get("out_dtype", torch.float32)
    x, g = _inputs(B, L, M, hop, seed=seed, dtype=dtype)
    band, y, gx = _band(lams, edges, x, g, M, L, sr, hop, log, **kw)
    kw.pop("sync", None)
    gks = _masked(g, edges)
    ref, ys, dls = _scalar_sum(lams, gks, x, M, L, sr, hop, log, **kw)
    for k, (lo, hi) in enumerate(zip(edges, edges[1:])):
        assert torch.equal(y[:, :, lo:hi], ys[k][:, :, lo:hi]), (k, lams[k])
        if dls[k] is not None:
            d = float(band.lambd.grad[k])
            assert abs(d - dls[k]) <= 1e-6 * abs(dls[k]) + 1e-12, (k, d, dls[k])
    assert torch.isfinite(gx).all()
    assert torch.equal(gx, ref), float((gx - ref).abs().max())
    via_multi = _multi_grad(lams, gks, x, M, L, sr, hop, log, **kw)
    assert torch.equal(gx, via_multi), float((gx - via_multi).abs().max())
    # the forward output and lambd.grad do not depend on whether x requires grad
    if dtype == torch.float32:
        plain, y0, _ = _band(lams, edges, x, g, M, L, sr, hop, log, waveform_grad=False, **kw)
        assert torch.equal(y0, y)
        if band.lambd.grad is not None:
            assert torch.equal(plain.lambd.grad, band.lambd.grad)
    return band, x, g, y, gx


@pytest.mark.parametrize("lams", LAM_SETS)
@pytest.mark.parametrize("log", [False, True])
def test_band_xgrad_equals_scalar_sum_and_multi_window(lams, log):
    _check(lams, log=log, **SHAPE)


@pytest.mark.parametrize("lams,edges,hop", [
    ([300.0, 128.0, 40.0], [0, 1, 63, 64], 128),                 # one-row groups at both ends; row e_hi = M meets the zero row
    ([300.0, 128.0, 40.0], [0, 21, 43, 64], 128),                # no edge a multiple of 4
    ([128.0], [0, 64], 128),                                     # K = 1: the scalar layer's x.grad
    ([300.0, 200.0, 128.0, 100.0, 85.3, 60.0, 40.0, 20.0], None, 128),      # K = 8, default edges
    ([300.0, 128.0, 40.0], None, 200),                           # T = 41, odd: the last pair has only its first frame, the last tile is partial
    ([2000.0, 700.0, 6.0], [0, 21, 43, 64], 200),                # the staging kernel's masks at the same edges
])
def test_band_xgrad_edges(lams, edges, hop):
    _check(lams, 4, 8000, 16000, hop, 64, True, edges=edges)


def test_band_xgrad_all_zero_htk_rows():
    # n_fft 64 (lambd 6) for mel bands 0 ... 7: narrower than a bin, all-zero rows of that bank -- log(eps) in the output, gradient exactly 0
    _check([6.0, 128.0], 4, 8000, 16000, 128, 64, True, edges=[0, 8, 64])


@pytest.mark.parametrize("lams", [[300.0, 128.0, 40.0], [2000.0, 700.0, 6.0]])
def test_band_xgrad_against_oracle(lams):
    B, L, sr, hop, M = 3, 8000, 16000, 200, 48
    edges = _edges(len(lams), M)
    x, g = _inputs(B, L, M, hop, seed=5)
    _, y, gx = _band(lams, edges, x, g, M, L, sr, hop, True)
    x_np, y_np = x.cpu().numpy(), y.cpu().numpy()
    ref = sum(O.backward_x(x_np, lam, hop, sr, np.ascontiguousarray(gk.cpu().numpy()), y_np) for lam, gk in zip(lams, _masked(g, edges)))
    err = float(np.abs(gx.cpu().numpy().astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))
    print(f"band x-gradient against the fp64 oracle, lambd {lams}: max abs error / max |ref| = {err:.3e}")
    assert err <= 1e-4, err


def test_band_xgrad_modes():
    lams, (B, L, sr, hop, M) = [300.0, 128.0, 40.0], SHAPE.values()
    edges = _edges(3, M)
    # bf16 + log: fp32 computed and rounded afterwards -- the same bits as the plain band layer's in-kernel rounding
    _, x, g, y, _ = _check(lams, B, L, sr, hop, M, True, out_dtype=torch.bfloat16)
    plain = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, out_dtype=torch.bfloat16).to(DEV)
    assert torch.equal(plain(x), y)
    # lambd_sync=True (host values, dmel_backward_x_band) gives the bits of the device path
    x, g = _inputs(B, L, M, hop)
    b0, y0, gx0 = _band(lams, edges, x, g, M, L, sr, hop, True)
    b1, y1, gx1 = _band(lams, edges, x, g, M, L, sr, hop, True, sync=True)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1) and torch.equal(b0.lambd.grad, b1.lambd.grad)
    # lambd not trained: the inference-mode forward, still the scalar sum
    _check(lams, B, L, sr, hop, M, True, lambd_grad=False)
    _check(lams, B, L, sr, hop, M, True, normalize=True)


def test_band_xgrad_long_clip_prep_window():
    _check([2000.0, 700.0, 64.0], 2, 40000, 16000, 400, 40, True)      # > 32768 samples: window tables from the prep kernel


@pytest.mark.parametrize("lams", [[300.0, 128.0, 40.0], [2000.0, 700.0, 6.0]])
def test_band_xgrad_unaligned_cotangent(lams):
    (B, L, sr, hop, M) = SHAPE.values()
    edges = [0, 21, 43, 64]
    x, g = _inputs(B, L, M, hop)
    band = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, band_edges=edges, log=True, waveform_grad=True).to(DEV)
    buf = torch.full((g.numel() + 16,), float("nan"), device=DEV)
    view = buf[5:5 + g.numel()].view_as(g)
    view.copy_(g)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and g.data_ptr() % 16 == 0
    res = []
    for cot in (g, view):
        band.lambd.grad = None
        xr = x.clone().requires_grad_(True)
        band(xr).backward(cot)                                 # the view itself reaches the kernels
        res.append((xr.grad, band.lambd.grad.clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ref, _, _ = _scalar_sum(lams, _masked(g, edges), x, M, L, sr, hop, True)
    assert torch.equal(res[1][0], ref)


def test_band_xgrad_deterministic():
    lams, (B, L, sr, hop, M) = [2000.0, 128.0, 6.0], SHAPE.values()
    x, g = _inputs(B, L, M, hop)
    band = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    grads = []
    for _ in range(2):
        xr = x.clone().requires_grad_(True)
        (band(xr) * g).sum().backward()
        grads.append(xr.grad)
    assert torch.equal(grads[0], grads[1])


def test_band_xgrad_uncovered_channel_is_nan_then_named():
    lams, B, L, sr, hop, M = [300.0, 128.0, 40.0], 2, 8000, 16000, 128, 32
    edges = _edges(3, M)
    x, g = _inputs(B, L, M, hop)
    band = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    good = band(x).detach()                                   # the training kernels, as the step below
    with torch.no_grad():
        band(x)                                               # a second observation: guards only near boundaries
    torch.cuda.synchronize()
    band.lambd.data[1] = 1500.0                               # n_fft 16384, far from what the tracking expects; no resync()
    xr = x.clone().requires_grad_(True)
    y = band(xr)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(y[:, :, edges[1]:edges[2]]).all()
    assert torch.equal(y[:, :, :edges[1]], good[:, :, :edges[1]]) and torch.equal(y[:, :, edges[2]:], good[:, :, edges[2]:])
    assert torch.isnan(xr.grad).all()
    with pytest.raises(RuntimeError, match="channel 1"):
        band(x.clone().requires_grad_(True))
    band.resync()
    band.lambd.grad = None
    xr = x.clone().requires_grad_(True)
    (band(xr) * g).sum().backward()
    ref, _, _ = _scalar_sum([300.0, 1500.0, 40.0], _masked(g, edges), x, M, L, sr, hop, True)
    assert torch.equal(xr.grad, ref)


def test_band_xgrad_captured_step_replays_eager():
    B, L, sr, hop, M = 4, 8000, 16000, 128, 32
    lams = [300.0, 128.0, 85.3]                               # channel 2 just below the 512 | 1024 boundary (85.33)
    edges = _edges(3, M)
    x, g = _inputs(B, L, M, hop, seed=7)
    band = BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, log=True, waveform_grad=True).to(DEV)
    band.set_tracking(8, 1)                                   # both neighbours of every channel's n_fft: three candidates each
    xr = x.clone().requires_grad_(True)
    gx_out, dl_out = torch.empty_like(x), torch.empty(3, device=DEV)

    def step():
        y = band(xr)
        gx, dl = torch.autograd.grad(y, (xr, band.lambd), g)
        gx_out.copy_(gx)
        dl_out.copy_(dl)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                # eager: cold start, workspace sized for the neighbours
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_gx, eager_dl = gx_out.clone(), dl_out.clone()
    launches = band._plan_for(torch.device(DEV)).last_multi_launch()
    assert [n for n, _ in launches] == [256, 512, 1024, 2048, 4096]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    gx_out.zero_()
    dl_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gx_out, eager_gx) and torch.equal(dl_out, eager_dl)
    ref, _, _ = _scalar_sum(lams, _masked(g, edges), x, M, L, sr, hop, True)
    assert torch.equal(eager_gx, ref)
    for k in range(3):
        assert band.lambd_status(channel=k)["error"] == 0


def test_default_layer_still_refuses():
    (B, L, sr, hop, M) = SHAPE.values()
    x, _ = _inputs(B, L, M, hop)
    band = BandSplitMelSpectrogram([300.0, 128.0, 40.0], M, L, sr, hop_length=hop, log=True).to(DEV)
    with pytest.raises(RuntimeError, match="has no waveform gradient"):
        band(x.clone().requires_grad_(True))


def test_band_xgrad_argument_checks():
    """behind a live plan: every NULL or malformed argument is DMEL_ERR_INVALID_ARGUMENT and grad_x stays as it was"""
    (B, L, sr, hop, M) = SHAPE.values()
    lib, bad = capi.load(), capi.DMEL_ERR_INVALID_ARGUMENT
    x, g = _inputs(B, L, M, hop)
    band = BandSplitMelSpectrogram([300.0, 128.0, 40.0], M, L, sr, hop_length=hop, waveform_grad=True).to(DEV)
    h = band._plan_for(torch.device(DEV))._h
    gx = torch.full((B * L + 4,), 7.0, device=DEV)
    lam_host = (C.c_float * 3)(300.0, 128.0, 40.0)
    lam_dev = band.lambd.detach().data_ptr()
    good = (C.c_int32 * 4)(0, 21, 42, 64)
    ns, masks = (C.c_int32 * 24)(256, 1024, 2048), (C.c_uint32 * 24)(4, 2, 1)

    def host(x_=x.data_ptr(), lam=lam_host, K=3, ed=good, flags=0, g_=g.data_ptr(), gx_=gx.data_ptr()):
        return lib.dmel_backward_x_band(h, x_, B, lam, K, ed, flags, g_, None, gx_, None)

    def dev(x_=x.data_ptr(), lam=lam_dev, K=3, ed=good, ns_=ns, masks_=masks, count=3, flags=0, g_=g.data_ptr(), gx_=gx.data_ptr()):
        return lib.dmel_backward_x_band_dev(h, x_, B, lam, K, ed, ns_, masks_, count, flags, g_, None, gx_, None)

    for fn in (host, dev):
        for kw in ({"x_": None}, {"g_": None}, {"gx_": None}, {"lam": None}, {"ed": None}, {"flags": capi.DMEL_FLAG_LOG},
                   {"ed": (C.c_int32 * 4)(0, 21, 42, 63)}, {"ed": (C.c_int32 * 4)(0, 21, 21, 64)}, {"gx_": gx.data_ptr() + 4}, {"K": 2}):
            assert fn(**kw) == bad, (fn.__name__, kw)
    for kw in ({"ns_": None}, {"masks_": None}, {"count": 0}, {"masks_": (C.c_uint32 * 24)(4, 2, 0)}, {"masks_": (C.c_uint32 * 24)(4, 2, 2)},
               {"ns_": (C.c_int32 * 24)(256, 2048, 1024)}, {"ns_": (C.c_int32 * 24)(256, 1000, 2048)}):
        assert dev(**kw) == bad, kw
    torch.cuda.synchronize()
    assert bool((gx == 7.0).all())
