"""Per-clip lengths on the two K-window layers (``per_clip_lengths=True``; dmel_fwd_multi_len_kernel, dmel_fwd_band_len_kernel) on the MI355X.
Channel k of MultiWindowMelSpectrogram.forward(x, lengths) and rows e_k ... e_{k+1} - 1 of BandSplitMelSpectrogram.forward(x, lengths) are
MelSpectrogramLayer(lambd[k], optimized=True)(x, lengths) bit for bit, lambd.grad[k] is that layer's for the channel's cotangent (1e-6: the
fp64 reductions partition the sum differently); the C entry points give the scalar entry point's out and tangent; full lengths are
forward(x); samples past a clip are never read; pad frames are a silent clip's and carry no gradient; an invalid length poisons its clip in
every channel and nothing else; a band group never writes another group's rows, neither pad rows nor NaN; clips past 32768 samples take the
prep kernel's partial sums; a captured step follows x and lengths rewritten in place; and the fp64 oracle's bars hold clip by clip at the
clip's own length without the cancellation exemption."""
import numpy as np
import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, capi, synth
from oracle import dmel_oracle as O
from test_hip_band_split import UNEVEN
from test_hip_lengths import _same
from test_hip_parity import assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPE = (6, 8000, 16000, 160, 64)                  # T = 51: odd, the last pair of the inference kernel holds one frame
LENS = [8000, 1, 159, 160, 4321, 2560]             # hop - 1 and hop; clips that end inside and at the edge of a tile; whole pad tiles
K8 = [2000.0, 700.0, 300.0, 200.0, 128.0, 85.4, 40.0, 6.0]                 # n_fft 16384, 8192, 2048, 2048, 1024, 512, 256, 64
LAM_SETS = [K8, [600.0, 20.0, 5.0], [128.0, 128.0, 128.0], [-128.0, 85.3, 85.5]]


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _x(B, L, seed):
    return torch.from_numpy(synth.waveforms(B, L, seed=seed)).to(DEV)


def _scalar_layer(lam, shape, log, bf16=False, sync=False):
    B, L, sr, hop, M = shape
    return MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                               log=log, out_dtype=_dt(bf16), lambd_sync=sync).to(DEV)


def _multi(lams, shape, log, bf16=False, sync=False, **kw):
    B, L, sr, hop, M = shape
    return MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=log, out_dtype=_dt(bf16), lambd_sync=sync, per_clip_lengths=True,
                                     **kw).to(DEV)


def _band(lams, edges, shape, log, bf16=False, sync=False, **kw):
    B, L, sr, hop, M = shape
    return BandSplitMelSpectrogram(lams, M, L, sr, hop_length=hop, band_edges=edges, log=log, out_dtype=_dt(bf16), lambd_sync=sync,
                                   per_clip_lengths=True, **kw).to(DEV)


def _edges(K, M, edges=None):
    return list(edges) if edges is not None else [(k * M) // K for k in range(K + 1)]


def _step(layer, x, g, lengths=None, train=True):
    """(out, lambd.grad) of one forward (+ backward to lambd when train)"""
    layer.lambd.grad = None
    if not train:
        with torch.no_grad():
            return (layer(x) if lengths is None else layer(x, lengths)), None
    y = layer(x) if lengths is None else layer(x, lengths)
    (y.float() * g.float()).sum().backward() if y.dtype == torch.float32 else y.backward(g.to(y.dtype).contiguous())
    torch.cuda.synchronize()
    return y.detach(), layer.lambd.grad.detach().clone()


class _Scalar:
    """the scalar lengths layer's outputs (grad mode and no_grad), computed once per (lambd, log, dtype) and left unchanged; its lambd.grad
    for a cotangent on request"""

    def __init__(self, shape, x, lengths):
        self.shape, self.x, self.lengths, self.cache = shape, x, lengths, {}

    def get(self, lam, log, bf16):
        key = (float(lam), bool(log), bool(bf16))
        if key not in self.cache:
            lay = _scalar_layer(lam, self.shape, log, bf16)
            with torch.no_grad():
                y_inf = lay(self.x, self.lengths)
            self.cache[key] = (lay, lay(self.x, self.lengths).detach(), y_inf)
        return self.cache[key]

    def grad(self, lam, log, bf16, g):
        lay = self.get(lam, log, bf16)[0]
        return float(_step(lay, self.x, g, self.lengths)[1])


_REF = {}


def _ref(shape, lens, seed=3):
    key = (shape, tuple(lens), seed)
    if key not in _REF:
        _REF[key] = _Scalar(shape, _x(shape[0], shape[1], seed), torch.tensor(lens, dtype=torch.int32, device=DEV))
    return _REF[key]


def _check_multi(ref, lams, log, bf16, sync, tag=""):
    B, L, sr, hop, M = ref.shape
    T = L // hop + 1
    lay = _multi(lams, ref.shape, log, bf16, sync)
    g = torch.from_numpy(synth.cotangent((B, len(lams), M, T), seed=4)).to(DEV).to(_dt(bf16))
    y, d = _step(lay, ref.x, g, ref.lengths)
    y_inf, _ = _step(lay, ref.x, g, ref.lengths, train=False)
    assert y.shape == (B, len(lams), M, T) and y.dtype == _dt(bf16)
    for k, lam in enumerate(lams):
        _, yk, yk_inf = ref.get(lam, log, bf16)
        assert torch.equal(y[:, k:k + 1], yk), ("train", tag, k, lam)
        assert torch.equal(y_inf[:, k:k + 1], yk_inf), ("no_grad", tag, k, lam)
        dk = ref.grad(lam, log, bf16, g[:, k:k + 1])
        print(f"klen multi lams={lams} log={log} bf16={bf16} sync={sync} k={k}: d={float(d[k])!r} d_k={dk!r}")
        assert abs(float(d[k]) - dk) <= 1e-6 * abs(dk) + 1e-12, (tag, k, float(d[k]), dk)


def _check_band(ref, lams, edges, log, bf16, sync, tag=""):
    B, L, sr, hop, M = ref.shape
    T = L // hop + 1
    e = _edges(len(lams), M, edges)
    lay = _band(lams, edges, ref.shape, log, bf16, sync)
    g = torch.from_numpy(synth.cotangent((B, 1, M, T), seed=4)).to(DEV).to(_dt(bf16))
    y, d = _step(lay, ref.x, g, ref.lengths)
    y_inf, _ = _step(lay, ref.x, g, ref.lengths, train=False)
    assert y.shape == (B, 1, M, T) and y.dtype == _dt(bf16)
    for k, lam in enumerate(lams):
        _, yk, yk_inf = ref.get(lam, log, bf16)
        assert torch.equal(y[:, :, e[k]:e[k + 1]], yk[:, :, e[k]:e[k + 1]]), ("train", tag, k, lam, e)
        assert torch.equal(y_inf[:, :, e[k]:e[k + 1]], yk_inf[:, :, e[k]:e[k + 1]]), ("no_grad", tag, k, lam, e)
        gk = torch.zeros_like(g)
        gk[:, :, e[k]:e[k + 1]] = g[:, :, e[k]:e[k + 1]]
        dk = ref.grad(lam, log, bf16, gk)
        print(f"klen band lams={lams} edges={e} log={log} bf16={bf16} sync={sync} k={k}: d={float(d[k])!r} d_k={dk!r}")
        assert abs(float(d[k]) - dk) <= 1e-6 * abs(dk) + 1e-12, (tag, k, e, float(d[k]), dk)


# ---- 1. bit for bit against the scalar lengths layer -------------------------------------------------------------------------------
@pytest.mark.parametrize("lams", LAM_SETS, ids=["k8", "nfft4096_128_32", "same", "signs"])
@pytest.mark.parametrize("log", [False, True])
def test_channels_and_rows_equal_the_scalar_lengths_layer(lams, log):
    ref = _ref(SHAPE, LENS)
    for bf16 in (False, True):
        for sync in (False, True):
            _check_multi(ref, lams, log, bf16, sync)
            for edges in [None] + UNEVEN[len(lams)]:
                _check_band(ref, lams, edges, log, bf16, sync)


# ---- 2. tangent rows through the C ABI -------------------------------------------------------------------------------------------
SENTINEL = -12345.5
MARGIN = 64          # floats in front of and behind an image: nothing is written outside it


def _framed(shape):
    """a sentinel-filled image with MARGIN floats of sentinel on both sides (16-byte aligned): (flat buffer, the image's view)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * MARGIN,), SENTINEL, device=DEV)
    return flat, flat[MARGIN:MARGIN + n].view(shape)


def _margins_kept(flat):
    return bool((flat[:MARGIN] == SENTINEL).all()) and bool((flat[-MARGIN:] == SENTINEL).all())


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("log", [False, True])
def test_tangent_rows_through_the_c_abi(dev, log):
    """dmel_forward_multi(_dev)_lengths and dmel_forward_band(_dev)_lengths against dmel_forward_lengths per channel: out AND tangent, bit for
    bit (NaN rows of the invalid clip included); nothing outside the images is written"""
    B, L, sr, hop, M = SHAPE
    T = L // hop + 1
    x = _x(B, L, 3)
    lens = torch.tensor([8000, 1, 159, 0, 4321, 2560], dtype=torch.int32, device=DEV)          # (clip 3: invalid, NaN rows)
    st = torch.cuda.current_stream().cuda_stream
    for lams, e in (([300.0, 128.0, 40.0], [0, 5, 30, 64]), ([2000.0, 700.0, 6.0], [0, 21, 42, 64]), ([128.0, 128.0, 128.0], [0, 5, 6, 64])):
        K = len(lams)
        lam_d = torch.tensor(lams, device=DEV)
        ref_plan = capi.Plan(L, hop, M, sr)
        refs = []
        for lam in lams:
            o_k, t_k = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
            ref_plan.forward_lengths(x.data_ptr(), lens.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), log, 1e-10, st)
            refs.append((o_k, t_k))
        # multi
        plan = capi.Plan(L, hop, M, sr)
        fo, out = _framed((B, K, M, T))
        ft, tan = _framed((B, K, M, T))
        scratch = torch.zeros((plan.scratch_bytes_multi(B, K),), dtype=torch.uint8, device=DEV)
        if dev:
            plan.forward_multi_dev(x.data_ptr(), B, lam_d.data_ptr(), K, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr(),
                                   lengths_ptr=lens.data_ptr())
        else:
            plan.forward_multi(x.data_ptr(), B, lams, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr(),
                               lengths_ptr=lens.data_ptr())
        torch.cuda.synchronize()
        assert len(plan.last_multi_launch()) >= len({capi.n_fft(v) for v in lams})          # dmel_plan_last_multi_launch records these calls too
        for k in range(K):
            assert _same(out[:, k:k + 1].contiguous(), refs[k][0]) and _same(tan[:, k:k + 1].contiguous(), refs[k][1]), ("multi", lams, k)
        assert torch.isnan(out[3]).all() and torch.isnan(tan[3]).all()
        assert _margins_kept(fo) and _margins_kept(ft)
        # band
        plan = capi.Plan(L, hop, M, sr)
        fo, out = _framed((B, 1, M, T))
        ft, tan = _framed((B, 1, M, T))
        if dev:
            plan.forward_band_dev(x.data_ptr(), B, lam_d.data_ptr(), e, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr(),
                                  lengths_ptr=lens.data_ptr())
        else:
            plan.forward_band(x.data_ptr(), B, lams, e, out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr(),
                              lengths_ptr=lens.data_ptr())
        torch.cuda.synchronize()
        assert len(plan.last_multi_launch()) >= len({capi.n_fft(v) for v in lams})
        for k in range(K):
            rows = slice(e[k], e[k + 1])
            assert _same(out[:, :, rows].contiguous(), refs[k][0][:, :, rows].contiguous()), ("band out", lams, k)
            assert _same(tan[:, :, rows].contiguous(), refs[k][1][:, :, rows].contiguous()), ("band tangent", lams, k)
        assert _margins_kept(fo) and _margins_kept(ft)


# ---- 3. full lengths equal forward(x) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log,bf16", [(True, False), (False, True)])
def test_full_lengths_are_forward_x_bit_for_bit(log, bf16):
    shape = (3, 9000, 16000, 300, 40)
    B, L, sr, hop, M = shape
    T = L // hop + 1
    lams = [10.0, 40.0, 128.0, 300.0, 1200.0]                       # n_fft 64, 256, 1024, 2048, 8192
    x = _x(B, L, 1)
    full = torch.full((B,), L, dtype=torch.int64)                   # (int64 on the CPU: clamped and copied by the layer)
    for sync in (False, True):
        for lay, gshape in ((_multi(lams, shape, log, bf16, sync), (B, len(lams), M, T)),
                            (_band(lams, [0, 3, 10, 11, 30, 40], shape, log, bf16, sync), (B, 1, M, T))):
            g = torch.from_numpy(synth.cotangent(gshape, seed=2)).to(DEV)
            for train in (True, False):
                y0, d0 = _step(lay, x, g, train=train)
                y1, d1 = _step(lay, x, g, full, train=train)
                assert _same(y0, y1), (type(lay).__name__, sync, train)
                if train:
                    assert torch.equal(d0, d1), (type(lay).__name__, sync, d0, d1)


# ---- 4. samples past the clip are never read --------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
def test_samples_past_the_clip_are_never_read(train):
    shape = (5, 8000, 16000, 128, 64)
    B, L, sr, hop, M = shape
    T = L // hop + 1
    lams, e = [300.0, 128.0, 20.0], [0, 5, 30, 64]
    x = _x(B, L, 2)
    lengths = torch.tensor([8000, 1, 700, 4001, 6173], dtype=torch.int32, device=DEV)
    mask = torch.arange(L, device=DEV)[None, :] >= lengths[:, None].long()
    for lay, gshape in ((_multi(lams, shape, True), (B, 3, M, T)), (_band(lams, e, shape, False), (B, 1, M, T))):
        g = torch.from_numpy(synth.cotangent(gshape, seed=2)).to(DEV)
        ref = _step(lay, x.masked_fill(mask, 0.0), g, lengths, train)
        for fill in (float("nan"), 1e30):
            got = _step(lay, x.masked_fill(mask, fill), g, lengths, train)
            assert _same(ref[0], got[0]), (type(lay).__name__, fill)
            if train:
                assert torch.equal(ref[1], got[1]), (type(lay).__name__, fill)
                assert torch.isfinite(got[1]).all()


# ---- 5. pad frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log,bf16,train", [(True, False, True), (False, False, True), (True, True, True), (True, False, False), (False, True, False)])
def test_pad_frames_are_a_silent_clip_and_carry_no_gradient(log, bf16, train):
    shape = (4, 8000, 16000, 160, 48)                             # T = 51
    B, L, sr, hop, M = shape
    T = L // hop + 1
    lams, e = [300.0, 128.0, 20.0], [0, 5, 30, 48]
    x = _x(B, L, 3)
    lengths = torch.tensor([2500, 160, 7999, 2], dtype=torch.int32, device=DEV)
    full = torch.full((B,), L, dtype=torch.int32, device=DEV)
    for lay, gshape in ((_multi(lams, shape, log, bf16), (B, 3, M, T)), (_band(lams, e, shape, log, bf16), (B, 1, M, T))):
        g = torch.from_numpy(synth.cotangent(gshape, seed=2)).to(DEV)
        y, d = _step(lay, x, g, lengths, train)
        y0, _ = _step(lay, torch.zeros_like(x), g, full, train)
        tl = lay.frame_lengths(lengths).tolist()
        assert tl == [v // hop + 1 for v in lengths.tolist()]
        for b in range(B):
            assert _same(y[b, :, :, tl[b]:].contiguous(), y0[b, :, :, tl[b]:].contiguous()), (type(lay).__name__, b)
        if train:
            pad = torch.arange(T, device=DEV)[None, None, None, :] >= lay.frame_lengths(lengths)[:, None, None, None]
            _, d2 = _step(lay, x, g.masked_fill(pad, 0.0), lengths)
            assert torch.equal(d, d2), (type(lay).__name__, d, d2)


# ---- 6. invalid lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
def test_an_invalid_length_poisons_its_own_clip_in_every_channel(train):
    shape = (4, 8000, 16000, 160, 64)
    B, L, sr, hop, M = shape
    T = L // hop + 1
    lams, e = [300.0, 128.0, 20.0], [0, 5, 30, 64]
    x = _x(B, L, 3)
    good = torch.tensor([4000, 4000, 8000, 8000], dtype=torch.int32, device=DEV)
    bad32 = torch.tensor([4000, 0, 8001, 8000], dtype=torch.int32, device=DEV)
    bad64 = torch.tensor([4000, 2 ** 32 + 4000, -5, 8000], dtype=torch.int64, device=DEV)      # must not wrap into the valid range
    for lay, gshape in ((_multi(lams, shape, True), (B, 3, M, T)), (_band(lams, e, shape, True), (B, 1, M, T))):
        g = torch.from_numpy(synth.cotangent(gshape, seed=2)).to(DEV)
        y_ok, _ = _step(lay, x, g, good, train)
        assert torch.isfinite(y_ok).all()
        for bad in (bad32, bad64):
            y, d = _step(lay, x, g, bad, train)
            assert torch.isnan(y[1]).all() and torch.isnan(y[2]).all(), type(lay).__name__         # every channel / every group's rows
            assert _same(y[0].contiguous(), y_ok[0].contiguous()) and _same(y[3].contiguous(), y_ok[3].contiguous()), type(lay).__name__
            if train:
                assert torch.isnan(d).all()                              # the NaN tangent of the invalid clips reaches every lambd.grad[k]


# ---- 7. band groups do not touch each other -----------------------------------------------------------------------------------------
def test_band_groups_do_not_touch_each_other():
    """an uncovered channel makes ITS rows NaN in every clip -- pad tiles and the invalid clip included: the coverage check comes first --
    and the other groups' rows, written by other launches into the same image, are exact; no pad or NaN fill leaves a channel's rows"""
    B, L, sr, hop, M = SHAPE
    T = L // hop + 1
    lams, e = [128.0, 300.0, 100.0], [0, 5, 30, 64]                    # channels 0 and 2 share n_fft 1024, channel 1 has 2048
    x = _x(B, L, 3)
    lens = torch.tensor([8000, 1, 159, 0, 4321, 2560], dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ref_plan = capi.Plan(L, hop, M, sr)
    refs = []
    for lam in lams:
        o_k, t_k = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
        ref_plan.forward_lengths(x.data_ptr(), lens.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), True, 1e-10, st)
        refs.append((o_k, t_k))
    plan = capi.Plan(L, hop, M, sr)
    scratch = torch.zeros((plan.scratch_bytes_multi(B, 3),), dtype=torch.uint8, device=DEV)
    lam_d = torch.tensor(lams, device=DEV)

    def run():
        fo, out = _framed((B, 1, M, T))
        ft, tan = _framed((B, 1, M, T))
        plan.forward_band_dev(x.data_ptr(), B, lam_d.data_ptr(), e, out.data_ptr(), tan.data_ptr(), True, 1e-10, st, scratch.data_ptr(),
                              lengths_ptr=lens.data_ptr())
        torch.cuda.synchronize()
        assert _margins_kept(fo) and _margins_kept(ft)
        assert not (out == SENTINEL).any() and not (tan == SENTINEL).any()       # every cell belongs to a group and was written by it
        return out, tan

    for _ in range(2):                                                   # cold start, then a second observation: guards only near boundaries
        out, tan = run()
        for k in range(3):
            rows = slice(e[k], e[k + 1])
            assert _same(out[:, :, rows].contiguous(), refs[k][0][:, :, rows].contiguous()), k
            assert _same(tan[:, :, rows].contiguous(), refs[k][1][:, :, rows].contiguous()), k
    lam_d[1] = 6.0                                                       # far from what the host picture covers
    out, tan = run()
    assert torch.isnan(out[:, :, e[1]:e[2]]).all() and torch.isnan(tan[:, :, e[1]:e[2]]).all()      # all clips, pad tiles included
    for k in (0, 2):
        rows = slice(e[k], e[k + 1])
        assert _same(out[:, :, rows].contiguous(), refs[k][0][:, :, rows].contiguous()), k
        assert _same(tan[:, :, rows].contiguous(), refs[k][1][:, :, rows].contiguous()), k
    with pytest.raises(capi.DmelError, match="channel 1"):
        run()

    # the same through the layers: the uncovered channel / group is NaN, the others are the previous forward's, the next forward raises
    for lay, rows_of in ((_multi(lams, SHAPE, True), lambda y, k: y[:, k]), (_band(lams, e, SHAPE, True), lambda y, k: y[:, :, e[k]:e[k + 1]])):
        with torch.no_grad():
            y0 = lay(x, lens)
            lay(x, lens)
            torch.cuda.synchronize()
            lay.lambd.data[1] = 6.0
            y1 = lay(x, lens)
            torch.cuda.synchronize()
            assert torch.isnan(rows_of(y1, 1)).all()
            assert _same(rows_of(y1, 0).contiguous(), rows_of(y0, 0).contiguous()) and _same(rows_of(y1, 2).contiguous(), rows_of(y0, 2).contiguous())
            with pytest.raises(RuntimeError, match="channel 1"):
                lay(x, lens)


# ---- 8. long clip ----------------------------------------------------------------------------------------------------------------
def test_long_clip_takes_the_partial_sums():
    shape = (2, 40000, 16000, 400, 40)                            # > 32768 samples: the clip sums come from the prep kernel, which stops at lengths[b]
    lams = [2000.0, 700.0, 64.0]
    ref = _ref(shape, [40000, 33000])
    for log in (True, False):
        _check_multi(ref, lams, log, False, False, "long")
        _check_band(ref, lams, None, log, False, False, "long")
    _check_multi(ref, lams, True, True, True, "long")
    _check_band(ref, lams, [0, 7, 8, 40], True, True, True, "long")


# ---- 9. captured step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["multi", "band"])
def test_captured_step_follows_x_and_lengths_rewritten_in_place(which):
    shape = (4, 8000, 16000, 128, 32)
    B, L, sr, hop, M = shape
    T = L // hop + 1
    lams, e = [300.0, 128.0, 20.0], [0, 5, 17, 32]

    def make():
        return _multi(lams, shape, True) if which == "multi" else _band(lams, e, shape, True)

    lay, eager = make(), make()
    g = torch.from_numpy(synth.cotangent((B, 3 if which == "multi" else 1, M, T), seed=8)).to(DEV)
    data = [(_x(B, L, 20 + i), torch.tensor(ln, dtype=torch.int32, device=DEV))
            for i, ln in enumerate(([8000, 1, 4000, 127], [128, 8000, 8000, 5000], [3000, 2999, 1, 8000], [8000, 8000, 8000, 8000]))]
    x_s, len_s = data[0][0].clone(), data[0][1].clone()
    y_out = torch.empty((B, 3 if which == "multi" else 1, M, T), device=DEV)
    lay.lambd.grad = torch.zeros_like(lay.lambd)

    def step():
        lay.lambd.grad.zero_()
        y = lay(x_s, len_s)
        y.backward(g)
        y_out.copy_(y.detach())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                      # eager warm-up: the cold start's one read of lambd
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for xi, li in data[1:] + data[:1]:
        x_s.copy_(xi)
        len_s.copy_(li)
        graph.replay()
        torch.cuda.synchronize()
        y_e, d_e = _step(eager, xi, g, li)
        assert _same(y_out, y_e), which
        assert torch.equal(lay.lambd.grad, d_e), (which, lay.lambd.grad, d_e)
    for k in range(3):
        assert lay.lambd_status(channel=k)["error"] == 0


# ---- 10. against the fp64 oracle, clip by clip at the clip's own length ------------------------------------------------------------------
ORACLE_SHAPE = (6, 6000, 16000, 150, 48)
ORACLE_LENS = [1, 149, 150, 1500, 4097, 6000]
# (layer, windows, band edges, waveform seed, cotangent seed): the smallest |d_ref| / sum|g t| over their channels, from the oracle alone, is 5.1e-3
ORACLE_CASES = [("band", [300.0, 128.0, 40.0], [0, 5, 30, 48], 5, 6), ("multi", [300.0, 128.0, 40.0], None, 5, 6),
                ("band", [700.0, 300.0, 128.0, 40.0], [0, 12, 24, 36, 48], 5, 6), ("band", [2000.0, 700.0, 6.0], [0, 16, 32, 48], 11, 12),
                ("multi", [128.0, 128.0], None, 5, 6)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=["band_uneven", "multi3", "band4", "band_wide", "multi_same"])
@pytest.mark.parametrize("log", [False, True])
def test_against_the_oracle_clip_by_clip(case, log):
    """Output: every element of the valid frames within 1e-4 (linear: assert_parity without the floor; log: |dy| / max(|y|, 1)).  Gradient:
    |d - d_ref| <= 1e-4 |d_ref|, d_ref the sum over clips of the oracle's backward on the clip's valid frames (band: over the group's rows).
    The project exempts cancellation-dominated sums (|d_ref| <= 1e-3 sum|g t|); on these cases the exemption must never be taken: asserted."""
    which, lams, edges, xseed, gseed = case
    B, L, sr, hop, M = ORACLE_SHAPE
    T = L // hop + 1
    K = len(lams)
    x_np = synth.waveforms(B, L, seed=xseed)
    g_np = synth.cotangent((B, K if which == "multi" else 1, M, T), seed=gseed)
    lay = _multi(lams, ORACLE_SHAPE, log) if which == "multi" else _band(lams, edges, ORACLE_SHAPE, log)
    y, d = _step(lay, torch.from_numpy(x_np).to(DEV), torch.from_numpy(g_np).to(DEV), torch.tensor(ORACLE_LENS, dtype=torch.int32))
    yv = y.cpu().numpy()
    for k, lam in enumerate(lams):
        c, lo, hi = (k, 0, M) if which == "multi" else (0, edges[k], edges[k + 1])
        d_ref, mag = 0.0, 0.0
        for b, lb in enumerate(ORACLE_LENS):
            tb = lb // hop + 1
            y_ref, t_ref = O.forward(x_np[b:b + 1, :lb], lam, hop, M, sr, apply_log=log)
            got, exp = yv[b:b + 1, c:c + 1, lo:hi, :tb], y_ref[:, :, lo:hi]
            if log:
                rel = np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)
                assert rel.max() <= 1e-4, (k, b, rel.max())
            else:
                assert_parity(f"klen_oracle/{which}/{lams}/k{k}/b{b}_L{lb}/mel", got, exp, allow_floor=False)
            gk = np.zeros_like(t_ref)
            gk[:, :, lo:hi] = g_np[b:b + 1, c:c + 1, lo:hi, :tb]
            d_ref += O.backward(gk, t_ref)
            mag += float(np.abs(gk * t_ref).sum())
        dk = float(d[k])
        print(f"klen oracle {which} lams={lams} edges={edges} log={log} k={k}: d={dk!r} d_ref={d_ref!r} |d_ref|/sum|g t|={abs(d_ref) / mag:.3e}")
        assert abs(d_ref) > 1e-3 * mag, ("the cancellation exemption would be taken", k, d_ref, mag)
        assert abs(dk - d_ref) <= 1e-4 * abs(d_ref), (k, dk, d_ref)
