"""MelSpectrogramLayer.forward(x, lengths): zero-padded batches computed clip by clip (dmel_fwd_len_kernel).  Full lengths give the default
path's bits; samples past a clip are never read; pad frames are those of a silent clip and carry no gradient; clip by clip against the fp64
oracle at the clip's own length; sync-free, lambd_sync, a captured step across an n_fft boundary and a batch handed over by address agree
bit for bit; an invalid length poisons its own clip only; the uses outside the feature raise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(lam, L, hop, M, sr, log=True, bf16=False, sync=False, **kw):
    from dmel_amd import MelSpectrogramLayer
    return MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                               log=log, out_dtype=torch.bfloat16 if bf16 else torch.float32, lambd_sync=sync, **kw).to(DEV)


def _x(B, L, seed):
    from dmel_amd import synth
    return torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)


def _step(layer, x, g, lengths=None, train=True):
    """(out, lambd.grad) of one forward (+ backward to lambd when train)"""
    layer.lambd.grad = None
    if not train:
        with torch.no_grad():
            return (layer(x) if lengths is None else layer(x, lengths)), None
    y = layer(x) if lengths is None else layer(x, lengths)
    (y.float() * g).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), layer.lambd.grad.detach().clone()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                                                                      b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


# (lambd -> n_fft, n_points, hop, log, bf16): n_fft 32 ... 8192 (1024: kTrainW), and a clip longer than 32768 samples
FULL = [(5.0, 4000, 100, True, False), (10.0, 4000, 100, True, False), (20.0, 4000, 100, False, False), (40.0, 4096, 64, True, False),
        (80.0, 8000, 160, False, False), (128.0, 16000, 512, True, True), (300.0, 8000, 256, True, False), (600.0, 12000, 300, False, True),
        (1200.0, 9000, 500, True, False), (128.0, 40000, 512, True, False)]


@pytest.mark.parametrize("lam,L,hop,log,bf16", FULL, ids=["nfft32", "nfft64", "nfft128", "nfft256", "nfft512", "nfft1024", "nfft2048", "nfft4096",
                                                          "nfft8192", "long_clip"])
def test_full_lengths_are_the_default_path_bit_for_bit(lam, L, hop, log, bf16):
    B, M = 3, 40
    x = _x(B, L, 1)
    T = L // hop + 1
    g = torch.randn(B, 1, M, T, device=DEV)
    full = torch.full((B,), L, dtype=torch.int32, device=DEV)
    for sync in (False, True):
        lay = _layer(lam, L, hop, M, 16000, log=log, bf16=bf16, sync=sync)
        for train in (True, False):
            y0, d0 = _step(lay, x, g, train=train)
            y1, d1 = _step(lay, x, g, full, train=train)
            assert _same(y0, y1), (sync, train)
            if train:
                assert torch.equal(d0, d1), (sync, float(d0), float(d1))


@pytest.mark.parametrize("lam,log,train", [(128.0, True, True), (80.0, False, True), (128.0, True, False)])
def test_samples_past_the_clip_are_never_read(lam, log, train):
    B, L, hop, M = 5, 16000, 256, 64
    x = _x(B, L, 2)
    lengths = torch.tensor([16000, 1, 700, 8001, 12345], dtype=torch.int32, device=DEV)
    g = torch.randn(B, 1, M, L // hop + 1, device=DEV)
    lay = _layer(lam, L, hop, M, 16000, log=log)
    mask = torch.arange(L, device=DEV)[None, :] >= lengths[:, None].long()
    ref = _step(lay, x.masked_fill(mask, 0.0), g, lengths, train)
    for fill in (float("nan"), 1e30):
        got = _step(lay, x.masked_fill(mask, fill), g, lengths, train)
        assert _same(ref[0], got[0]), fill
        if train:
            assert torch.equal(ref[1], got[1]), fill


@pytest.mark.parametrize("lam,log,bf16,train", [(128.0, True, False, True), (80.0, False, False, True), (300.0, True, True, True),
                                                (80.0, True, False, False), (128.0, False, True, False)])
def test_pad_frames_are_a_silent_clip_and_carry_no_gradient(lam, log, bf16, train):
    B, L, hop, M = 4, 16000, 160, 48          # (T = 101: odd, the last pair of the inference kernel holds one frame)
    lay = _layer(lam, L, hop, M, 16000, log=log, bf16=bf16)
    x = _x(B, L, 3)
    lengths = torch.tensor([5000, 160, 15999, 2], dtype=torch.int32, device=DEV)
    T = L // hop + 1
    g = torch.randn(B, 1, M, T, device=DEV)
    y, d = _step(lay, x, g, lengths, train)
    y0, _ = _step(lay, torch.zeros_like(x), g, torch.full((B,), L, dtype=torch.int32, device=DEV), train)
    tl = lay.frame_lengths(lengths).tolist()
    for b in range(B):
        assert _same(y[b, :, :, tl[b]:].contiguous(), y0[b, :, :, tl[b]:].contiguous()), b
    if train:
        pad = torch.arange(T, device=DEV)[None, None, None, :] >= lay.frame_lengths(lengths)[:, None, None, None]
        _, d2 = _step(lay, x, g.masked_fill(pad, 0.0), lengths)
        assert torch.equal(d, d2), (float(d), float(d2))


def _rel_err(got, exp, floor=1e-6):
    # plain relative error; bins more than 120 dB below the loudest one are measured against that floor (tests/test_hip_parity.py)
    scale = np.maximum(np.abs(exp), floor * np.abs(exp).max() + 1e-30)
    return float((np.abs(got.astype(np.float64) - exp.astype(np.float64)) / scale).max())


# (lambd, n_points, hop, n_mels, sample rate, lengths): hop <= n_fft / 2 and hop > n_fft / 2; clips of one tile and of many
ORACLE = [
    (80.0, 4000, 160, 40, 16000, [1, 159, 160, 1600, 200, 1001, 4000]),                 # n_fft 512, hop <= n_fft / 2
    (40.0, 3000, 200, 32, 16000, [1, 199, 200, 1000, 100, 2999, 3000]),                 # n_fft 256, hop > n_fft / 2
    (128.0, 6000, 64, 64, 16000, [1, 63, 64, 640, 500, 4097, 6000]),                    # n_fft 1024 (kTrainW), many tiles per clip
]


@pytest.mark.parametrize("case", range(len(ORACLE) + 1), ids=["nfft512", "hop_gt_half", "nfft1024_many_tiles", "audio_mnist"])
def test_against_the_oracle_clip_by_clip(case):
    from oracle import dmel_oracle as O
    from test_hip_parity import assert_parity
    if case < len(ORACLE):
        lam, L, hop, M, sr, lens = ORACLE[case]
    else:
        # the reference's audio_mnist shape (search_spaces.py:64): B 64, 8000 points, 8 kHz, hop 80, 64 mels, lengths 2400 ... 8000
        lam, L, hop, M, sr = 46.67, 8000, 80, 64, 8000
        lens = np.random.default_rng(5).integers(2400, 8001, size=64).tolist()
    B = len(lens)
    x = _x(B, L, 4)
    T = L // hop + 1
    g = torch.randn(B, 1, M, T, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    lay = _layer(lam, L, hop, M, sr, log=False)
    lengths = torch.tensor(lens, dtype=torch.int32)                       # (a CPU tensor: the layer copies it to x's device)
    y, d = _step(lay, x, g, lengths)
    y, x_np, g_np = y.cpu().numpy(), x.cpu().numpy(), g.cpu().numpy()
    d_ref, worst = 0.0, 0.0
    for b, lb in enumerate(lens):
        tb = lb // hop + 1
        yr, tr = O.forward(x_np[b:b + 1, :lb], lam, hop, M, sr)
        worst = max(worst, _rel_err(y[b:b + 1, :, :, :tb], yr))
        assert_parity(f"lengths_oracle/case{case}/b{b}_L{lb}/mel", y[b:b + 1, :, :, :tb], yr, allow_floor=False)     # every element, no floor
        d_ref += O.backward(g_np[b:b + 1, :, :, :tb], tr)
    assert worst <= 1e-4, worst
    assert abs(float(d) - d_ref) <= 1e-4 * abs(d_ref), (float(d), d_ref)


def test_sync_and_sync_free_agree():
    B, L, hop, M = 6, 16000, 256, 64
    x = _x(B, L, 7)
    g = torch.randn(B, 1, M, L // hop + 1, device=DEV)
    lengths = torch.tensor([300, 16000, 4000, 9999, 1, 12000], dtype=torch.int64, device=DEV)       # (int64: converted on the device)
    for lam in (80.0, 128.0, 1200.0):
        a = _step(_layer(lam, L, hop, M, 16000), x, g, lengths)
        b = _step(_layer(lam, L, hop, M, 16000, sync=True), x, g, lengths)
        assert _same(a[0], b[0]) and torch.equal(a[1], b[1]), lam


def test_captured_step_replays_the_eager_steps_across_an_n_fft_boundary():
    from dmel_amd import GraphedStep
    B, L, hop, M, steps = 4, 8000, 100, 40, 12
    T = L // hop + 1
    gen = torch.Generator(DEV).manual_seed(8)
    xs = [_x(B, L, 20 + i) for i in range(steps)]
    lens = [torch.randint(1, L + 1, (B,), device=DEV, generator=gen, dtype=torch.int32) for _ in range(steps)]
    gs = [torch.randn(B, 1, M, T, device=DEV, generator=gen) for _ in range(steps)]

    def run(graphed):
        lay = _layer(84.0, L, hop, M, 8000)                          # n_fft 512; lambd + 0.3 per step crosses 85.33 (-> 1024) at step 5
        hist_y = torch.zeros(steps, B, 1, M, T, device=DEV)
        hist_d = torch.zeros(steps, device=DEV)
        k = torch.zeros(1, dtype=torch.long, device=DEV)

        def step(x, ln, g):
            if lay.lambd.grad is not None:
                lay.lambd.grad.zero_()
            y = lay(x, ln)
            (y * g).sum().backward()
            hist_y.index_copy_(0, k, y.detach().unsqueeze(0))
            hist_d.index_copy_(0, k, lay.lambd.grad.view(1))
            with torch.no_grad():
                lay.lambd.add_(0.3)
            k.add_(1)

        if graphed:
            gs_ = GraphedStep(step, [lay], steps_per_replay=1, inputs=[xs[0], lens[0], gs[0]])
            for i in range(steps):
                gs_.feed(xs[i], lens[i], gs[i])
            gs_.flush()
        else:
            for i in range(steps):
                step(xs[i], lens[i], gs[i])
        torch.cuda.synchronize()
        assert lay.lambd_status()["error"] == 0
        return hist_y, hist_d, (gs_.captures if graphed else 0), float(lay.lambd.detach())

    ye, de, _, lam_e = run(False)
    yg, dg, captures, lam_g = run(True)
    assert lam_e == lam_g and 6 * lam_e > 512
    assert torch.equal(ye, yg) and torch.equal(de, dg)
    assert captures >= 2, captures


def test_batch_by_address():
    from dmel_amd import SlotInput
    B, L, hop, M = 4, 16000, 512, 64
    x = _x(B, L, 9)
    g = torch.randn(B, 1, M, L // hop + 1, device=DEV)
    lengths = torch.tensor([16000, 3000, 512, 7777], dtype=torch.int32, device=DEV)
    lay = _layer(128.0, L, hop, M, 16000)
    cell = torch.tensor([x.data_ptr()], dtype=torch.int64, device=DEV)
    a = _step(lay, x, g, lengths)
    b = _step(lay, SlotInput(cell, x.shape), g, lengths)
    assert _same(a[0], b[0]) and torch.equal(a[1], b[1])


def test_an_invalid_length_poisons_its_own_clip_only():
    B, L, hop, M = 5, 16000, 256, 64
    x = _x(B, L, 10)
    g = torch.randn(B, 1, M, L // hop + 1, device=DEV)
    lay = _layer(128.0, L, hop, M, 16000)
    good = torch.tensor([4000, 16000, 9000, 300, 12000], dtype=torch.int32, device=DEV)
    bad = torch.tensor([4000, 0, 9000, 16001, 12000], dtype=torch.int32, device=DEV)
    for train in (True, False):
        ya, _ = _step(lay, x, g, good, train)
        yb, _ = _step(lay, x, g, bad, train)
        assert torch.isnan(yb[1]).all() and torch.isnan(yb[3]).all()
        for b in (0, 2, 4):
            assert _same(ya[b], yb[b]), (train, b)
    neg = torch.tensor([-5, 16000, 9000, 300, 12000], dtype=torch.int32, device=DEV)
    yc, _ = _step(lay, x, g, neg, False)
    assert torch.isnan(yc[0]).all() and _same(yc[1:], ya[1:])


def test_uses_outside_the_feature_raise():
    from dmel_amd import MelSpectrogramLayer, MultiWindowMelSpectrogram, SpectrogramLayer, dmel_log_mel
    B, L, hop, M = 2, 8000, 160, 32
    x = _x(B, L, 11)
    ln = torch.tensor([4000, 8000], dtype=torch.int32, device=DEV)
    lay = _layer(80.0, L, hop, M, 16000)
    for bad in (ln[:1], ln.view(2, 1), ln.float(), torch.empty(B, dtype=torch.int32, device="meta"), [4000, 8000]):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            lay(x, bad)
    with pytest.raises(RuntimeError, match="waveform gradient"):
        lay(x.clone().requires_grad_(True), ln)
    with pytest.raises(RuntimeError, match="HTK bank"):
        _layer(80.0, L, hop, M, 16000, learnable_fb=True)(x, ln)
    slow = MelSpectrogramLayer(torch.tensor(80.0), n_mels=M, n_points=L, sample_rate=16000, hop_length=hop, device=DEV, optimized=False).to(DEV)
    with pytest.raises(RuntimeError, match="optimized=True"):
        slow(x, ln)
    with pytest.raises(RuntimeError, match="lengths"):
        MultiWindowMelSpectrogram([40.0, 80.0], M, L, 16000, hop_length=hop).to(DEV)(x, ln)
    with pytest.raises(RuntimeError, match="lengths"):
        SpectrogramLayer(torch.tensor(80.0), device=DEV, optimized=True, hop_length=hop).to(DEV)(x, ln)
    with pytest.raises(RuntimeError, match="lengths"):
        dmel_log_mel(x, torch.tensor(80.0, device=DEV), M, 16000, hop, lengths=ln)
    with pytest.raises(RuntimeError, match="16384"):
        _layer(3000.0, L, hop, M, 16000, sync=True)(x, ln)                # n_fft 32768: outside the fused kernel's range
