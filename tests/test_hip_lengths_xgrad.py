"""MelSpectrogramLayer(lengths_waveform_grad=True): the waveform gradient of forward(x, lengths) (dmel_xgrad_len.hip).  Bit for bit: full
lengths are the fixed-length path; samples past a clip and the cotangent of pad frames are never read and the gradient past a clip is +0;
a row depends on nothing but its own clip (batch independence, a stale workspace, invalid lengths elsewhere in the batch); sync-free,
lambd_sync and a captured step agree.  Clip by clip against the fp64 oracle at the clip's own length, the error normalised per clip (a mean
of the gradient taken over n_points instead of the clip's length moves a short clip by 1e-2 ... 1e-1 of its maximum)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, SR = 8000, 16000          # rows of 8000 samples everywhere
TOL = 1e-4                   # the project's bar for every x-gradient test
MIXED = [300, 129, 4097, 2500, 1, 8000]


def _layer(lam, hop, M=32, log=True, bf16=False, sync=False, on=True, norm=False):
    from dmel_amd import MelSpectrogramLayer
    return MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True,
                               normalize_window=norm, log=log, out_dtype=torch.bfloat16 if bf16 else torch.float32, lambd_sync=sync,
                               lengths_waveform_grad=on).to(DEV)


def _x(B, seed):
    from dmel_amd import synth
    return torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)


def _g(B, M, hop, seed):
    from dmel_amd import synth
    return torch.from_numpy(synth.cotangent((B, 1, M, L // hop + 1), seed=seed)).to(DEV)


def _len(values, dtype=torch.int32):
    return torch.tensor(values, dtype=dtype, device=DEV)


def _step(layer, x, g, lengths=None):
    """(out, lambd.grad, x.grad) of one forward and backward"""
    layer.lambd.grad = None
    xr = x.detach().clone().requires_grad_(True)
    y = layer(xr) if lengths is None else layer(xr, lengths)
    y.backward(g.to(y.dtype))
    torch.cuda.synchronize()
    return y.detach(), layer.lambd.grad.detach().clone(), xr.grad.detach()


def _bits(a):
    return a.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _zero_past(gx, lens):
    """grad_x[b, Lc:] is +0.0, bit for bit"""
    return all(int(_bits(gx[b, lb:]).abs().max()) == 0 for b, lb in enumerate(lens) if lb < gx.shape[1])


def _oracle_errors(x, lens, lam, hop, g, y, log, gx, norm=False):
    """max |got - ref| / max |ref| per clip, over the clip's own samples (a clip whose reference is zero -- one sample -- must be zero)"""
    from oracle import dmel_oracle as O
    x_np, g_np, y_np, gx_np = x.cpu().numpy(), g.cpu().numpy(), y.float().cpu().numpy(), gx.double().cpu().numpy()
    errs = []
    for b, lb in enumerate(lens):
        tb = lb // hop + 1
        ref = O.backward_x(x_np[b:b + 1, :lb], lam, hop, SR, g_np[b:b + 1, :, :, :tb], y_np[b:b + 1, :, :, :tb] if log else None,
                           normalize_window=norm)
        diff, top = float(np.abs(gx_np[b:b + 1, :lb] - ref).max()), float(np.abs(ref).max())
        errs.append(diff / top if top > 0 else (0.0 if diff == 0 else float("inf")))
    return errs


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [10.0, 40.0, 128.0, 300.0, 700.0, 2000.0], ids=["nfft64", "nfft256", "nfft1024", "nfft2048", "nfft8192", "nfft16384"])
def test_full_lengths_are_the_fixed_length_path(lam):
    B, M = 3, 32
    x = _x(B, 1)
    full = _len([L] * B)
    for hop in (100, 250):                                        # a multiple of 4 (16-byte rows in the combine pass) and one that is not
        g = _g(B, M, hop, 2)
        for log in (True, False):
            for sync in (False, True):
                lay = _layer(lam, hop, M, log=log, sync=sync)
                y0, d0, gx0 = _step(lay, x, g)
                y1, d1, gx1 = _step(lay, x, g, full)
                assert _same(y0, y1) and _same(d0, d1), (hop, log, sync)
                assert _same(gx0, gx1), (hop, log, sync, float((gx0 - gx1).abs().max()))


@pytest.mark.parametrize("lam,log", [(40.0, True), (128.0, False), (700.0, True)], ids=["nfft256", "nfft1024", "nfft8192"])
def test_never_read_and_exactly_zero(lam, log):
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 3), _g(B, M, hop, 4), _len(MIXED)
    lay = _layer(lam, hop, M, log=log)
    y, d, gx = _step(lay, x, g, lengths)
    assert torch.isfinite(gx).all() and _zero_past(gx, MIXED)
    past = torch.arange(L, device=DEV)[None, :] >= lengths[:, None]
    for fill in (float("nan"), float("inf"), 1e30):
        y2, _, gx2 = _step(lay, x.masked_fill(past, fill), g, lengths)
        assert _same(y, y2) and _same(gx, gx2), fill
    pad = torch.arange(L // hop + 1, device=DEV)[None, None, None, :] >= lay.frame_lengths(lengths)[:, None, None, None]
    y3, _, gx3 = _step(lay, x, g.masked_fill(pad, float("nan")), lengths)
    assert _same(y, y3) and _same(gx, gx3) and _zero_past(gx3, MIXED)


@pytest.mark.parametrize("lam", [40.0, 700.0, 2000.0], ids=["nfft256", "nfft8192", "nfft16384"])
def test_a_row_is_the_one_clip_batch(lam):
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 5), _g(B, M, hop, 6), _len(MIXED)
    lay = _layer(lam, hop, M)
    y, _, gx = _step(lay, x, g, lengths)
    for b in range(B):
        yb, _, gxb = _step(lay, x[b:b + 1], g[b:b + 1], lengths[b:b + 1])
        assert _same(y[b:b + 1], yb) and _same(gx[b:b + 1], gxb), b


@pytest.mark.parametrize("lam", [40.0, 700.0], ids=["nfft256", "nfft8192"])
def test_a_stale_workspace_is_not_read(lam):
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 7), _g(B, M, hop, 8), _len(MIXED)
    used = _layer(lam, hop, M)
    _step(used, x, g, _len([L] * B))                               # every tile of the plan's workspace now holds a full-length clip's data
    got = _step(used, x, g, lengths)
    fresh = _step(_layer(lam, hop, M), x, g, lengths)
    assert all(_same(a, b) for a, b in zip(got, fresh))


@pytest.mark.parametrize("lam", [40.0, 700.0], ids=["nfft256", "nfft8192"])
def test_an_invalid_length_poisons_its_own_row_only(lam):
    B, M, hop = 6, 32, 100
    x, g = _x(B, 9), _g(B, M, hop, 10)
    lay = _layer(lam, hop, M)
    _, _, good = _step(lay, x, g, _len([4000, 100, 777, 8000, 3000, 2500]))
    assert torch.isfinite(good).all()
    bad32 = _len([4000, 0, 9000, L + 1, -5, 2500])
    bad64 = _len([4000, 0, 9000, L + 1, 2 ** 32 + 4000, 2500], torch.int64)     # (clamped on the device before the narrowing: no wrap to 4000)
    for bad in (bad32, bad64):
        _, _, gx = _step(lay, x, g, bad)
        for b in (1, 2, 3, 4):
            assert torch.isnan(gx[b]).all(), b
        for b in (0, 5):
            assert _same(gx[b], good[b]), b


def test_sync_paths_agree_and_repeat():
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 11), _g(B, M, hop, 12), _len(MIXED)
    for lam in (40.0, 128.0, 700.0):
        free, sync = _layer(lam, hop, M), _layer(lam, hop, M, sync=True)
        a, a2, b = _step(free, x, g, lengths), _step(free, x, g, lengths), _step(sync, x, g, lengths)
        assert all(_same(u, v) for u, v in zip(a, a2)), lam
        assert all(_same(u, v) for u, v in zip(a, b)), lam


@pytest.mark.parametrize("lam", [85.3, 85.5], ids=["below_the_boundary", "above_the_boundary"])
def test_either_side_of_an_n_fft_boundary_on_the_sync_free_path(lam):
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 13), _g(B, M, hop, 14), _len(MIXED)
    y, _, gx = _step(_layer(lam, hop, M), x, g, lengths)
    assert torch.isfinite(gx).all()
    errs = _oracle_errors(x, MIXED, lam, hop, g, y, True, gx)
    print("boundary", lam, errs)
    assert max(errs) <= TOL, errs


def test_a_lambd_no_launch_covers_gives_nan_and_raises_at_the_next_forward():
    B, M, hop = 3, 32, 100
    x, g, lengths = _x(B, 15), _g(B, M, hop, 16), _len([300, 8000, 4097])
    lay = _layer(40.0, hop, M)
    lay.set_tracking(8, 2)                                        # never guard
    _, _, gx = _step(lay, x, g, lengths)
    assert torch.isfinite(gx).all()
    lay.lambd.data.fill_(700.0)                                   # n_fft 256 -> 8192 behind the host's back
    y, _, gx = _step(lay, x, g, lengths)
    assert torch.isnan(y).all() and torch.isnan(gx).all()
    with pytest.raises(RuntimeError):
        lay(x.clone().requires_grad_(True), lengths)
    _, _, gx = _step(lay, x, g, lengths)                          # tracking was reset: the layer works again
    assert torch.isfinite(gx).all()


def test_a_captured_step_replays_the_eager_step():
    B, M, hop = 4, 32, 512                                        # (n_fft 1024 -> 2048 at hop 512 needs a larger workspace)
    x = _x(B, 17).requires_grad_(True)
    g, lengths = _g(B, M, hop, 18), _len([300, 8000, 4097, 2500])
    lay = _layer(128.0, hop, M)
    plan = lay._plan_for(torch.device(DEV))
    plan.force_launch(1024, 0)                                    # eager: the primary launch alone

    def step():
        if x.grad is not None:
            x.grad.zero_()
        lay.zero_grad(set_to_none=False)
        lay(x, lengths).backward(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(); step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref_gx, ref_dl = x.grad.clone(), lay.lambd.grad.clone()
    assert torch.isfinite(ref_gx).all()
    plan.force_launch(1024, 3)                                    # the graph holds both neighbours, which no eager step has run
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    plan.force_launch(0, 0)
    x.grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(x.grad, ref_gx) and _same(lay.lambd.grad, ref_dl)
    assert lay.lambd_status()["error"] == 0


@pytest.mark.parametrize("lam", [40.0, 700.0], ids=["nfft256", "nfft8192"])
def test_a_clip_of_one_sample_has_a_zero_gradient(lam):
    B, M, hop = 3, 32, 100
    x, g = _x(B, 19), _g(B, M, hop, 20)
    _, _, gx = _step(_layer(lam, hop, M), x, g, _len([1, 8000, 1]))
    for b in (0, 2):
        assert int(_bits(gx[b]).abs().max()) == 0, b              # the clip minus its mean is zero; so is everything past it
    assert float(gx[1].abs().max()) > 0


def test_bf16_output_with_log():
    B, M, hop, lam = len(MIXED), 32, 100, 128.0
    x, g, lengths = _x(B, 21), _g(B, M, hop, 22), _len(MIXED)
    g16 = g.to(torch.bfloat16)
    on, off = _layer(lam, hop, M, bf16=True), _layer(lam, hop, M, bf16=True, on=False)
    y, d, gx = _step(on, x, g16, lengths)
    y_off = off(x, lengths)
    assert y.dtype == torch.bfloat16 and _same(y, y_off.detach())
    y32, _, gx32 = _step(_layer(lam, hop, M), x, g16.float(), lengths)     # the fp32-output run fed the same cotangent, widened
    assert _same(gx, gx32) and _same(y, y32.to(torch.bfloat16))


def test_fp64_waveform():
    B, M, hop, lam = len(MIXED), 32, 100, 40.0
    x, g, lengths = _x(B, 23).double(), _g(B, M, hop, 24), _len(MIXED)
    y, _, gx = _step(_layer(lam, hop, M), x, g, lengths)
    assert gx.dtype == torch.float64 and int(_bits(gx[0, MIXED[0]:]).abs().max()) == 0 and _zero_past(gx, MIXED)
    errs = _oracle_errors(x.float(), MIXED, lam, hop, g, y, True, gx)
    print("fp64", errs)
    assert max(errs) <= TOL, errs


def test_output_and_lambd_grad_are_the_flag_off_path():
    B, M, hop = len(MIXED), 32, 100
    x, g, lengths = _x(B, 25), _g(B, M, hop, 26), _len(MIXED)
    for lam in (40.0, 700.0):
        for sync in (False, True):
            y, d, _ = _step(_layer(lam, hop, M, sync=sync), x, g, lengths)
            off = _layer(lam, hop, M, sync=sync, on=False)
            y0 = off(x, lengths)
            y0.backward(g)
            assert _same(y, y0.detach()) and _same(d, off.lambd.grad), (lam, sync)


def test_uses_outside_the_feature_raise():
    from dmel_amd import MelSpectrogramLayer
    x, ln = _x(2, 27).requires_grad_(True), _len([4000, 8000])
    with pytest.raises(RuntimeError, match="no waveform gradient"):
        _layer(80.0, 160, on=False)(x, ln)                        # the default stays what it was
    fb = MelSpectrogramLayer(torch.tensor(80.0), n_mels=32, n_points=L, sample_rate=SR, hop_length=160, device=DEV, optimized=True,
                             learnable_fb=True, lengths_waveform_grad=True).to(DEV)
    with pytest.raises(RuntimeError, match="HTK bank"):
        fb(x, ln)
    slow = MelSpectrogramLayer(torch.tensor(80.0), n_mels=32, n_points=L, sample_rate=SR, hop_length=160, device=DEV, optimized=False,
                               lengths_waveform_grad=True).to(DEV)
    with pytest.raises(RuntimeError, match="optimized=True"):
        slow(x, ln)


# ---- against the fp64 oracle, clip by clip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,hop", [(40.0, 100), (400.0, 500)], ids=["wave_nfft256", "lds_nfft4096"])
def test_every_frame_count_against_the_oracle(lam, hop):
    """lengths j hop - 1 and j hop for every j: every Tc from 1 to T, so every tile boundary and both parities of the last pair"""
    M = 32
    lens = [v for j in range(1, L // hop + 1) for v in (j * hop - 1, j * hop)]
    assert sorted({lb // hop + 1 for lb in lens}) == list(range(1, L // hop + 2))
    B = len(lens)
    x, g = _x(B, 31), _g(B, M, hop, 32)
    y, _, gx = _step(_layer(lam, hop, M), x, g, _len(lens))
    assert _zero_past(gx, lens)
    errs = _oracle_errors(x, lens, lam, hop, g, y, True, gx)
    print("every_frame_count", lam, max(errs), errs)
    assert max(errs) <= TOL, (max(errs), lens[int(np.argmax(errs))])


@pytest.mark.parametrize("lam", [40.0, 128.0], ids=["nfft256", "nfft1024"])
def test_a_normalised_window_takes_the_partial_sums_in_the_wave_kernel(lam):
    """normalize_window=True: the wave kernel reads its window table and the clip's partial sums from dmel_prep_kernel (stopped at the
    clip's length) instead of evaluating them itself"""
    lens = [300, 8000, 4097, 1, 2500, 129]
    B, M, hop = len(lens), 32, 100
    x, g = _x(B, 35), _g(B, M, hop, 36)
    lay = _layer(lam, hop, M, norm=True)
    y0, d0, gx0 = _step(lay, x, g)
    y1, d1, gx1 = _step(lay, x, g, _len([L] * B))
    assert _same(y0, y1) and _same(d0, d1) and _same(gx0, gx1)    # full lengths: the fixed-length path, bit for bit
    y, _, gx = _step(lay, x, g, _len(lens))
    assert _zero_past(gx, lens)
    errs = _oracle_errors(x, lens, lam, hop, g, y, True, gx, norm=True)
    print("normalised", lam, errs)
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("lam", [20.0, 128.0, 700.0], ids=["nfft128", "nfft1024", "nfft8192"])
def test_a_mixed_batch_against_the_oracle(lam, log):
    lens = [300, 8000, 4097, 1, 2500, 129]
    B, M, hop = len(lens), 32, 100
    x, g = _x(B, 33), _g(B, M, hop, 34)
    y, _, gx = _step(_layer(lam, hop, M, log=log), x, g, _len(lens))
    errs = _oracle_errors(x, lens, lam, hop, g, y, log, gx)
    print("mixed", lam, log, errs)
    assert int(_bits(gx[3]).abs().max()) == 0                     # (the clip of one sample: reference and result are zero)
    assert max(errs) <= TOL, errs
