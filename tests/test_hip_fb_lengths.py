"""MelSpectrogramLayer(learnable_fb=True, lengths_learnable_fb=True).forward(x, lengths): zero-padded batches through the TRAINED filterbank
(dmel_fwd_fb_len_kernel, the length-aware dmel_fbgrad_lds_kernel; dmel_forward_dev_fixed_lengths, dmel_backward_fb_dev_lengths,
dmel_backward_fb_saved_lengths).  Full lengths give the bits of forward(x); every clip agrees with the fp64 oracle run on that clip alone;
samples past a clip and the cotangent / saved output / spectrogram of pad frames are never read; an invalid length makes its clip's rows
and the whole mel_fb.grad NaN and leaves nothing behind; the step has no host read and replays from a HIP graph with ``lengths`` rewritten
in place.  Unless stated the bank is moved off the HTK values first (dense and positive).  Tolerances: TOL of tests/test_hip_parity.py."""
import numpy as np
import pytest
import torch

from oracle import dmel_oracle as O
from test_hip_parity import TOL, _gfb_err, _rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
EPS = 1e-10


def _layer(lam, L, hop, M, *, log, mfma="fp32", save_spec=True, sync=False, bf16=False, flag=True, perturb=True, **kw):
    from dmel_amd import MelSpectrogramLayer
    lay = MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True,
                              log=log, eps=EPS, learnable_fb=True, out_dtype=torch.bfloat16 if bf16 else torch.float32, lambd_sync=sync,
                              mfma=mfma, save_spec=save_spec, **(dict(lengths_learnable_fb=True) if flag else {}), **kw).to(DEV)
    if perturb:
        gen = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            lay.mel_fb += (0.02 * torch.rand(lay.mel_fb.shape, generator=gen)).to(DEV)
    return lay


def _x(B, L, seed):
    from dmel_amd import synth
    return torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)


def _g(shape, seed):
    from dmel_amd import synth
    return torch.from_numpy(synth.cotangent(tuple(shape), seed=seed)).to(DEV)


def _step(layer, x, g, lengths=None):
    """(out, lambd.grad or None, mel_fb.grad) of one forward and backward"""
    layer.lambd.grad = None
    layer.mel_fb.grad = None
    y = layer(x) if lengths is None else layer(x, lengths)
    y.backward(g.to(y.dtype))
    torch.cuda.synchronize()
    d = None if layer.lambd.grad is None else layer.lambd.grad.detach().clone()
    return y.detach(), d, layer.mel_fb.grad.detach().clone()


def _bits(a):
    return a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _full(B, L):
    return torch.full((B,), L, dtype=torch.int32, device=DEV)


# ---- 1. full lengths are layer(x) bit for bit ---------------------------------------------------------------------------------------
# (lambd, n_points, hop, n_mels, batch): n_fft 32 (no folded row), 64 (the smallest kTrainH), 512, 1024 with two mel column tiles (no rider),
# 2048 with 77 K-blocks per clip (slices cross clip ends), 8192 (beyond kTrainH)
SHAPES = [(5.0, 2000, 100, 24, 3), (10.0, 2000, 100, 24, 3), (80.0, 4000, 160, 40, 3), (128.0, 4000, 100, 130, 3), (300.0, 4000, 25, 40, 7),
          (1200.0, 9000, 500, 32, 3)]
SHAPE_IDS = ["nfft32", "nfft64", "nfft512", "nfft1024_m130", "nfft2048_b7", "nfft8192"]


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("mfma", ["fp32", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_full_lengths_are_the_default_path_bit_for_bit(shape, mfma, log):
    lam, L, hop, M, B = shape
    x, g = _x(B, L, 1), _g((B, 1, M, L // hop + 1), 2)
    for save_spec in (True, False):
        for sync in (False, True):
            lay = _layer(lam, L, hop, M, log=log, mfma=mfma, save_spec=save_spec, sync=sync)
            y0, d0, f0 = _step(lay, x, g)
            y1, d1, f1 = _step(lay, x, g, _full(B, L))
            assert torch.isfinite(f0).all() and torch.isfinite(y0).all()
            assert _same(y0, y1), (save_spec, sync)
            assert torch.equal(d0, d1), (save_spec, sync, float(d0), float(d1))
            assert _same(f0, f1), (save_spec, sync, float((f0 - f1).abs().max()))


@pytest.mark.parametrize("mfma", ["fp32", "bf16x3"])
def test_full_lengths_bf16_output_and_frozen_lambd(mfma):
    lam, L, hop, M, B = SHAPES[2]
    x, g = _x(B, L, 3), _g((B, 1, M, L // hop + 1), 4)
    lay = _layer(lam, L, hop, M, log=True, mfma=mfma, bf16=True)
    y0, d0, f0 = _step(lay, x, g)
    y1, d1, f1 = _step(lay, x, g, _full(B, L))
    assert y1.dtype == torch.bfloat16 and _same(y0, y1) and torch.equal(d0, d1) and _same(f0, f1)
    # lambd frozen: no tangent, the spectrogram is recomputed in the backward
    lay = _layer(lam, L, hop, M, log=True, mfma=mfma)
    lay.lambd.requires_grad_(False)
    y0, d0, f0 = _step(lay, x, g)
    y1, d1, f1 = _step(lay, x, g, _full(B, L))
    assert d0 is None and d1 is None and _same(y0, y1) and _same(f0, f1) and torch.isfinite(f1).all()
    with torch.no_grad():                                                        # and the forward without any gradient
        assert _same(lay(x), lay(x, _full(B, L)))


# ---- 2. clip by clip against the fp64 oracle ----------------------------------------------------------------------------------------
L2, HOP2, M2 = 4000, 100, 40
LENS2 = [1, 150, 250, 399, 400, 1499, 1500, 1650, 3999, 4000]           # Tc = 1, 2, 3, 4, 5, 15, 16, 17, T - 1, T


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("lam", [80.0, 128.0], ids=["nfft512", "nfft1024"])
def test_every_clip_matches_the_oracle_on_that_clip_alone(lam, log):
    from dmel_amd import MelSpectrogramLayer
    B, T = len(LENS2), L2 // HOP2 + 1
    assert sorted(set(n // HOP2 + 1 for n in LENS2)) == [1, 2, 3, 4, 5, 15, 16, 17, T - 1, T]
    x, g = _x(B, L2, 5), _g((B, 1, M2, T), 6)
    lengths = torch.tensor(LENS2, dtype=torch.int32, device=DEV)
    lay = _layer(lam, L2, HOP2, M2, log=log)
    y, d, gfb = _step(lay, x, g, lengths)
    y_np, x_np, g_np, fb_np = y.cpu().numpy(), x.cpu().numpy(), g.cpu().numpy(), lay.mel_fb.detach().cpu().numpy().astype(np.float64)
    silent, _, _ = _step(lay, torch.zeros_like(x), g)                            # a frame of zero mel power: 0, or the layer's log(0 + eps)
    assert torch.isfinite(y).all() and torch.isfinite(gfb).all() and torch.isfinite(d).all()
    ref_fb = np.zeros_like(fb_np)
    ref_d = ref_abs = 0.0
    for b, Lb in enumerate(LENS2):
        Tc = Lb // HOP2 + 1
        spec = O.spectrogram(x_np[b:b + 1, :Lb], lam, HOP2, False, True).astype(np.float64)        # (1, F, Tc), DC removed over the clip
        mel = np.einsum("ft,fm->mt", spec[0], fb_np)
        got = y_np[b, 0, :, :Tc].astype(np.float64)
        if Lb == 1:
            assert _same(y[b, :, :, :1], silent[b, :, :, :1])                     # x - mean(x) = 0 exactly
        else:
            err = _rel_err(np.exp(got), mel + EPS) if log else _rel_err(got, mel)
            print(f"clip {b} (L {Lb}, Tc {Tc}): rel err {err:.3e}")
            assert err <= TOL, (b, Lb, err)
        assert _same(y[b, :, :, Tc:], silent[b, :, :, Tc:]), (b, "pad frames")
        ref_fb += O.backward_fb(x_np[b:b + 1, :Lb], lam, HOP2, g_np[b:b + 1, :, :, :Tc], y_np[b:b + 1, :, :, :Tc] if log else None)
        # lambd.grad of this clip: a fixed-length layer built for n_points = Lb, carrying the same bank
        one = MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M2, n_points=Lb, sample_rate=SR, hop_length=HOP2, device=DEV, optimized=True,
                                  log=log, eps=EPS, learnable_fb=True).to(DEV)
        with torch.no_grad():
            one.mel_fb.copy_(lay.mel_fb)
        one(x[b:b + 1, :Lb].contiguous()).backward(g[b:b + 1, :, :, :Tc].contiguous())
        ref_d += float(one.lambd.grad)
        ref_abs += abs(float(one.lambd.grad))
    e_fb = _gfb_err(gfb.cpu().numpy(), ref_fb)
    print(f"mel_fb.grad err {e_fb:.3e}; lambd.grad {float(d):.6e} against {ref_d:.6e} (sum |.| {ref_abs:.3e})")
    assert e_fb <= TOL
    # ... and element by element over each clip's own frames (tests/fbgrad_cases.py; the inputs: tests/test_fbgrad_restatement_cpu.py)
    from test_hip_parity import _assert_gfb_elementwise
    _assert_gfb_elementwise(f"fbgrad_lengths/{int(lam)}/{'log' if log else 'lin'}", gfb.cpu().numpy(),
                            dict(lambd=lam, hop=HOP2, n_mels=M2, sr=SR, f_min=0.0, f_max=None, normalize_window=False), x_np, g_np,
                            y_np if log else None, lengths=LENS2)
    assert abs(float(d) - ref_d) <= 1e-4 * ref_abs


# ---- 3. never read ------------------------------------------------------------------------------------------------------------------
LENS3 = [4000, 1, 250, 1650, 399, 3100]


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("save_spec", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("mfma", ["fp32", "bf16x3"])
def test_nothing_past_a_clip_or_in_a_pad_frame_is_read(mfma, save_spec, log):
    B, T = len(LENS3), L2 // HOP2 + 1
    x, g = _x(B, L2, 7), _g((B, 1, M2, T), 8)
    lengths = torch.tensor(LENS3, dtype=torch.int32, device=DEV)
    lay = _layer(128.0, L2, HOP2, M2, log=log, mfma=mfma, save_spec=save_spec)
    past = torch.arange(L2, device=DEV)[None, :] >= lengths[:, None].long()
    pad = (torch.arange(T, device=DEV)[None, :] >= lay.frame_lengths(lengths)[:, None].long())[:, None, None, :].expand_as(g)
    y0, d0, f0 = _step(lay, x.masked_fill(past, 0.0), g.masked_fill(pad, 0.0), lengths)
    assert torch.isfinite(f0).all() and torch.isfinite(d0).all()
    for fill in (float("nan"), 1e30):
        y1, d1, f1 = _step(lay, x.masked_fill(past, fill), g.masked_fill(pad, 0.0), lengths)
        assert _same(y0, y1) and torch.equal(d0, d1) and _same(f0, f1), ("x", fill)
        y2, d2, f2 = _step(lay, x, g.masked_fill(pad, fill), lengths)
        assert _same(y0, y2) and _same(f0, f2), ("cotangent", fill)
        if fill == 1e30:
            assert torch.equal(d0, d2), (float(d0), float(d2))


# ---- 4. invalid lengths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("save_spec", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("bad", [0, -5, L2 + 1, 2 ** 32 + 4000])
def test_an_invalid_length_is_nan_for_its_clip_and_the_whole_filterbank_gradient(bad, save_spec):
    B, T = 4, L2 // HOP2 + 1
    x, g = _x(B, L2, 9), _g((B, 1, M2, T), 10)
    good = torch.tensor([4000, 777, 1650, 2500], dtype=torch.int64, device=DEV)
    lay = _layer(128.0, L2, HOP2, M2, log=True, save_spec=save_spec)
    y0, d0, f0 = _step(lay, x, g, good)
    lens = good.clone()
    lens[2] = bad
    y1, d1, f1 = _step(lay, x, g, lens)
    assert torch.isnan(y1[2]).all()
    for b in (0, 1, 3):
        assert _same(y0[b], y1[b]), b
    assert torch.isnan(f1).all()
    y2, d2, f2 = _step(lay, x, g, good)                                          # nothing sticks
    assert _same(y0, y2) and torch.equal(d0, d2) and _same(f0, f2)
    assert lay.lambd_status()["error"] == 0


# ---- 5. sync-free and captured ------------------------------------------------------------------------------------------------------
def test_the_step_is_sync_free_and_replays_with_lengths_rewritten_in_place():
    """forward(x, lengths), backward, Adam on lambd and mel_fb, captured once (a host read inside would fail the capture); every replay sees
    what ``lengths`` holds then.  Compared, as test_trainable_filterbank_step_is_sync_free_and_graph_capturable compares, with the eagerly
    stepped lambd_sync=True layer."""
    B, L, hop, M, steps = 4, 4000, 100, 40, 8
    T = L // hop + 1
    x, g = _x(B, L, 11), _g((B, 1, M, T), 12)
    gen = torch.Generator().manual_seed(5)
    lens = [torch.randint(1, L + 1, (B,), generator=gen, dtype=torch.int32).to(DEV) for _ in range(steps)]

    def run(sync, graphed):
        lay = _layer(80.0, L, hop, M, log=False, sync=sync)
        opt = torch.optim.Adam([{"params": [lay.lambd], "lr": 0.05}, {"params": [lay.mel_fb], "lr": 1e-4}], capturable=True)
        cur = lens[0].clone()

        def step():
            opt.zero_grad(set_to_none=False)
            lay(x, cur).backward(g)
            opt.step()
        if not graphed:
            for i in range(steps):
                cur.copy_(lens[i])
                step()
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for i in range(2):
                    cur.copy_(lens[i])
                    step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            for i in range(2, steps):
                cur.copy_(lens[i])
                graph.replay()
        torch.cuda.synchronize()
        assert lay.lambd_status()["error"] == 0
        return lay.lambd.detach().cpu().numpy().copy(), lay.mel_fb.detach().cpu().numpy().copy()

    lam_e, fb_e = run(True, False)
    lam_g, fb_g = run(False, True)
    assert abs(float(lam_e) - 80.0) > 0.1                                        # the parameters did move
    np.testing.assert_allclose(lam_g, lam_e, rtol=1e-5)
    np.testing.assert_allclose(fb_g, fb_e, rtol=1e-4, atol=1e-6)


# ---- 6. bank and n_fft --------------------------------------------------------------------------------------------------------------
def test_a_bank_update_is_picked_up_and_a_lambd_outside_the_banks_n_fft_is_refused():
    B, T = 3, L2 // HOP2 + 1
    x, g = _x(B, L2, 13), _g((B, 1, M2, T), 14)
    lengths = torch.tensor([4000, 1650, 250], dtype=torch.int32, device=DEV)
    lay = _layer(80.0, L2, HOP2, M2, log=False)
    y0, _, _ = _step(lay, x, g, lengths)
    with torch.no_grad():
        lay.mel_fb.mul_(2.0)
    y1, _, _ = _step(lay, x, g, lengths)
    assert float((y1 - 2.0 * y0).abs().max()) <= 1e-5 * float(y0.abs().max()) and float(y0.abs().max()) > 0
    with torch.no_grad():
        lay.lambd.fill_(200.0)                                                    # n_fft 2048: not the bank's 512
    y2 = lay(x, lengths)
    torch.cuda.synchronize()
    assert torch.isnan(y2).all()
    with pytest.raises(RuntimeError, match="tied to one n_fft"):
        lay(x, lengths)


# ---- 7. addresses -------------------------------------------------------------------------------------------------------------------
def _placed(t, k):
    """`t` copied to element 4 + k of a NaN-filled flat buffer (tests/test_hip_addresses.py)"""
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[4 + k:4 + k + t.numel()].view(t.shape)
    view.copy_(t.detach())
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 + k) * t.element_size() % 16
    return view


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("mfma", ["fp32", "bf16x3"])
def test_cotangent_and_saved_output_at_unaligned_addresses_give_the_aligned_bits(mfma, log):
    """grad_out, the saved log output and the saved spectrogram at 4 + k elements past a 16-byte boundary, through the C ABI (the layer's own
    tensors are always aligned): the GEMM's 16-byte requests are declared 4-byte aligned, so mel_fb.grad keeps its bits."""
    from dmel_amd import capi
    B, T, n = len(LENS3), L2 // HOP2 + 1, 1024
    x, g = _x(B, L2, 15), _g((B, 1, M2, T), 16)
    lengths = torch.tensor(LENS3, dtype=torch.int32, device=DEV)
    lay = _layer(128.0, L2, HOP2, M2, log=log, mfma=mfma)
    plan = capi.Plan(L2, HOP2, M2, SR)
    st = torch.cuda.current_stream().cuda_stream
    fb, lam = lay.mel_fb.detach().contiguous(), lay.lambd.detach().clone()
    plan.set_filterbank_dev(n, fb.data_ptr(), st)
    flags = capi.DMEL_FLAG_MFMA_BF16X3 if mfma == "bf16x3" else 0
    y, tan = torch.empty(B, 1, M2, T, device=DEV), torch.empty(B, 1, M2, T, device=DEV)
    spec = torch.empty(B, n // 2 + 1, T, device=DEV)
    scratch = torch.empty(plan.scratch_bytes(B), dtype=torch.uint8, device=DEV)
    plan.forward_dev_fixed_lengths(x.data_ptr(), lengths.data_ptr(), B, lam.data_ptr(), n, y.data_ptr(), tan.data_ptr(), spec.data_ptr(), log, EPS,
                                   st, scratch.data_ptr(), extra_flags=flags)

    def grads(gk, yk, sk, xk):
        a, b = torch.full_like(fb, float("nan")), torch.full_like(fb, float("nan"))
        plan.backward_fb_saved_lengths(sk.data_ptr(), lengths.data_ptr(), B, n, gk.data_ptr(), yk.data_ptr(), None, a.data_ptr(), None, None, log, st,
                                       extra_flags=flags)
        plan.backward_fb_dev_lengths(xk.data_ptr(), lengths.data_ptr(), B, lam.data_ptr(), n, gk.data_ptr(), yk.data_ptr(), b.data_ptr(), log, st,
                                     extra_flags=flags)
        torch.cuda.synchronize()
        return a, b
    a0, b0 = grads(g, y, spec, x)
    assert torch.isfinite(a0).all() and torch.isfinite(b0).all()
    for k in (1, 2, 3):
        a1, b1 = grads(_placed(g, k), _placed(y, k), _placed(spec, k), x)
        assert _same(a0, a1) and _same(b0, b1), k


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
def test_waveform_at_unaligned_addresses(log):
    """x at 4 + k elements past a 16-byte boundary.  The clip mean adds in another order there by design (tests/test_hip_addresses.py,
    tests/test_clip_mean_orders_cpu.py), so against the aligned run: the project's bar, and the same view twice gives the same bits."""
    B, T = len(LENS3), L2 // HOP2 + 1
    x, g = _x(B, L2, 17), _g((B, 1, M2, T), 18)
    lengths = torch.tensor(LENS3, dtype=torch.int32, device=DEV)
    lay = _layer(128.0, L2, HOP2, M2, log=log)
    y0, d0, f0 = _step(lay, x, g, lengths)
    for k in (1, 2, 3):
        xk = _placed(x, k)
        y1, d1, f1 = _step(lay, xk, g, lengths)
        y2, d2, f2 = _step(lay, xk, g, lengths)
        assert _same(y1, y2) and torch.equal(d1, d2) and _same(f1, f2), k
        a, b = y1.cpu().numpy().astype(np.float64), y0.cpu().numpy().astype(np.float64)
        err = _rel_err(np.exp(a), np.exp(b)) if log else _rel_err(a, b)
        e_fb = _gfb_err(f1.cpu().numpy(), f0.cpu().numpy().astype(np.float64))
        print(f"k {k}: out {err:.3e} mel_fb.grad {e_fb:.3e}")
        assert err <= TOL and e_fb <= TOL, (k, err, e_fb)
