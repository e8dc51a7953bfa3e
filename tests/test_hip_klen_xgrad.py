"""MultiWindowMelSpectrogram / BandSplitMelSpectrogram(per_clip_lengths=True, lengths_waveform_grad=True): the waveform gradient of
forward(x, lengths) on the K-window layers (dmel_xgrad_klen.hip), on the MI355X.  x.grad is 0 + gx_0 + ... + gx_{K-1} in ascending channel
order, gx_k the x.grad of MelSpectrogramLayer(lambd[k], optimized=True, lengths_waveform_grad=True)(x, lengths) for the channel's cotangent
(multi: g[:, k:k+1]; band: G_k, the one cotangent with the rows outside e_k ... e_{k+1} - 1 set to +0.0), bit for bit, and so are the output
and lambd.grad; full lengths are forward(x) with waveform_grad=True; samples past a clip and the cotangent of pad frames are never read and
x.grad past a clip is +0.0; a stale workspace is not read; an invalid length poisons its own row only; the sync-free step follows lambd
across an n_fft boundary, makes x.grad NaN for an uncovered channel, and replays from a captured graph with the lengths rewritten in place;
unaligned x and cotangent give the aligned bits and an unaligned grad_x is refused; the fp64 oracle's bar holds clip by clip.

fp64 x: x.grad is fp64.  The layer adds the channels' terms in fp32 (one combine launch) and takes that sum back through the fp64
masked-mean conversion of the input, so the reference that holds bit for bit is the K scalar layers' fp32 sum taken through the same
conversion; K scalar layers each fed the fp64 x and summed in fp64 round once per channel in fp64 instead of fp32 and agree to fp32 rounding
(bound below: K + 1 roundings of 2^-24 relative to the largest term)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, capi, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, SR, M, B = 8000, 16000, 32, 6     # rows of 8000 samples everywhere
TOL = 1e-4                           # the project's bar for every x-gradient test (test_hip_lengths_xgrad.py)
MIXED = [300, 129, 4097, 2500, 1, 8000]
WAVE = [40.0, 42.0, 128.0]           # n_fft 256, 256, 1024: two channels share a launch
LDS = [10.0, 300.0, 700.0]           # n_fft 64, 2048 and 8192 (the LDS path)
BIG = [2000.0, 128.0, 20.0]          # n_fft 16384 (LDS path, twiddles from memory), 1024, 128
SETS = [WAVE, LDS, BIG]
SET_IDS = ["wave_256_256_1024", "lds_64_2048_8192", "big_16384_1024_128"]
UNEVEN = [0, 5, 17, 32]
KINDS = ["multi", "band", "band_uneven"]


def _edges(kind, K=3):
    return None if kind == "multi" else (UNEVEN if kind == "band_uneven" else [(k * M) // K for k in range(K + 1)])


def _layer(kind, lams, hop=100, log=True, bf16=False, sync=False, norm=False, on=True, wg=False):
    kw = dict(hop_length=hop, normalize_window=norm, log=log, out_dtype=torch.bfloat16 if bf16 else torch.float32, lambd_sync=sync,
              waveform_grad=wg, per_clip_lengths=True, lengths_waveform_grad=on)
    if kind == "multi":
        return MultiWindowMelSpectrogram(lams, M, L, SR, **kw).to(DEV)
    return BandSplitMelSpectrogram(lams, M, L, SR, band_edges=_edges(kind, len(lams)), **kw).to(DEV)


def _scalar(lam, hop=100, log=True, bf16=False, norm=False):
    return MelSpectrogramLayer(torch.tensor(float(lam)), n_mels=M, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True,
                               normalize_window=norm, log=log, out_dtype=torch.bfloat16 if bf16 else torch.float32,
                               lengths_waveform_grad=True).to(DEV)


def _x(seed, rows=B):
    return torch.from_numpy(synth.waveforms(rows, L, seed=seed)).to(DEV)


def _g(kind, K, hop, seed, rows=B):
    return torch.from_numpy(synth.cotangent((rows, K if kind == "multi" else 1, M, L // hop + 1), seed=seed)).to(DEV)


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


def _channel_cotangents(kind, g, K):
    """what channel k's scalar layer is fed: g[:, k:k+1], or G_k (zeros + slice assignment: the rows outside a group are POSITIVE zeros)"""
    if kind == "multi":
        return [g[:, k:k + 1].contiguous() for k in range(K)]
    e, out = _edges(kind, K), []
    for lo, hi in zip(e, e[1:]):
        gk = torch.zeros_like(g)
        gk[:, :, lo:hi] = g[:, :, lo:hi]
        out.append(gk)
    return out


def _scalar_sum(kind, lams, x, g, lengths, **kw):
    """0 + gx_0 + gx_1 + ... over the K scalar layers in ascending channel order; their outputs and lambd.grad"""
    acc, ys, dls = torch.zeros_like(x), [], []
    for lam, gk in zip(lams, _channel_cotangents(kind, g, len(lams))):
        y, d, gx = _step(_scalar(lam, **kw), x, gk, lengths)
        acc = acc + gx
        ys.append(y)
        dls.append(d)
    return acc, ys, dls


def _part(kind, k, K, t, scalar=False):
    """channel k's part of the K-window output t, or (scalar) the same part of that channel's scalar layer's output"""
    if kind == "multi":
        return t if scalar else t[:, k:k + 1]
    e = _edges(kind, K)
    return t[:, :, e[k]:e[k + 1]]


# ---- 1. equals the K scalar layers --------------------------------------------------------------------------------------------------------
# (hop, log, lambd_sync, bf16 output, normalize_window): every value of every dimension with every value of every other one at least once
COMBOS = [(100, True, False, False, False), (100, False, True, False, True), (250, True, True, False, True), (250, False, False, False, False),
          (100, True, True, True, False), (250, False, False, True, True), (250, True, False, True, False), (100, False, True, True, True)]


@pytest.mark.parametrize("lams", SETS, ids=SET_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_k_scalar_layers(kind, lams):
    K = len(lams)
    x, lengths = _x(1), _len(MIXED)
    for hop, log, sync, bf16, norm in COMBOS:
        tag = (kind, lams, hop, log, sync, bf16, norm)
        g = _g(kind, K, hop, 2)
        if bf16:
            g = g.to(torch.bfloat16)
        y, d, gx = _step(_layer(kind, lams, hop, log, bf16, sync, norm), x, g, lengths)
        ref, ys, dls = _scalar_sum(kind, lams, x, g, lengths, hop=hop, log=log, bf16=bf16, norm=norm)
        assert y.dtype == (torch.bfloat16 if bf16 else torch.float32), tag
        for k in range(K):
            assert _same(_part(kind, k, K, y), _part(kind, k, K, ys[k], scalar=True)), ("out", tag, k)
            print("klen xgrad lambd.grad", tag, k, float(d[k]), float(dls[k]))
            assert _same(d[k].reshape(()), dls[k].reshape(())), ("lambd.grad", tag, k, float(d[k]), float(dls[k]))
        assert torch.isfinite(gx).all() and _zero_past(gx, MIXED), tag
        assert _same(gx, ref), ("x.grad", tag, float((gx - ref).abs().max()))
        # the output and lambd.grad are the flag-off layer's (an x that asks for no gradient): the same kernels
        off = _layer(kind, lams, hop, log, bf16, sync, norm, on=False)
        y0 = off(x, lengths)
        y0.backward(g.to(y0.dtype))
        assert _same(y, y0.detach()) and _same(d, off.lambd.grad), ("flag off", tag)


# ---- 2. full lengths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lams", SETS, ids=SET_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_full_lengths_are_forward_x_with_waveform_grad(kind, lams):
    x, full = _x(3, 3), _len([L] * 3)
    for hop in (100, 250):
        g = _g(kind, len(lams), hop, 4, 3)
        for log, sync, norm in ((True, False, False), (False, True, True)):
            lay = _layer(kind, lams, hop, log, sync=sync, norm=norm, wg=True)
            a, b = _step(lay, x, g), _step(lay, x, g, full)
            assert all(_same(u, v) for u, v in zip(a, b)), (hop, log, sync, norm, float((a[2] - b[2]).abs().max()))


# ---- 3. never read, exactly zero ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lams", [WAVE, LDS], ids=SET_IDS[:2])
@pytest.mark.parametrize("kind", KINDS)
def test_never_read_and_exactly_zero(kind, lams):
    hop = 100
    x, g, lengths = _x(5), _g(kind, len(lams), hop, 6), _len(MIXED)
    lay = _layer(kind, lams, hop)
    y, d, gx = _step(lay, x, g, lengths)
    assert torch.isfinite(gx).all() and _zero_past(gx, MIXED)
    past = torch.arange(L, device=DEV)[None, :] >= lengths[:, None]
    for fill in (float("nan"), float("inf"), 1e30):
        y2, d2, gx2 = _step(lay, x.masked_fill(past, fill), g, lengths)
        assert _same(y, y2) and _same(d, d2) and _same(gx, gx2), fill
    pad = torch.arange(L // hop + 1, device=DEV)[None, None, None, :] >= lay.frame_lengths(lengths)[:, None, None, None]
    y3, _, gx3 = _step(lay, x, g.masked_fill(pad, float("nan")), lengths)           # (lambd.grad is the dot with a zero tangent there: NaN)
    assert _same(y, y3) and _same(gx, gx3) and _zero_past(gx3, MIXED)


# ---- 4. a row is the one-clip batch; a stale workspace is not read ------------------------------------------------------------------------
@pytest.mark.parametrize("lams", [WAVE, LDS], ids=SET_IDS[:2])
@pytest.mark.parametrize("kind", ["multi", "band_uneven"])
def test_a_stale_workspace_is_not_read_and_a_row_is_the_one_clip_batch(kind, lams):
    hop = 100
    x, g, lengths = _x(7), _g(kind, len(lams), hop, 8), _len(MIXED)
    used = _layer(kind, lams, hop)
    _step(used, x, g, _len([L] * B))                               # every tile of the plan's workspace now holds a full-length clip's data
    got = _step(used, x, g, lengths)
    fresh = _step(_layer(kind, lams, hop), x, g, lengths)
    assert all(_same(u, v) for u, v in zip(got, fresh))
    for b in range(B):
        yb, _, gxb = _step(used, x[b:b + 1], g[b:b + 1], lengths[b:b + 1])
        assert _same(got[0][b:b + 1], yb) and _same(got[2][b:b + 1], gxb), b


# ---- 5. invalid lengths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lams", [WAVE, LDS], ids=SET_IDS[:2])
@pytest.mark.parametrize("kind", ["multi", "band"])
def test_an_invalid_length_poisons_its_own_row_only(kind, lams):
    hop = 100
    x, g = _x(9), _g(kind, len(lams), hop, 10)
    lay = _layer(kind, lams, hop)
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


# ---- 6. sync-free near a boundary ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["multi", "band"])
def test_sync_free_across_an_n_fft_boundary_then_an_uncovered_channel(kind):
    hop, below, above = 100, 42.6, 43.0                           # int(6 lambd) = 255 | 258: n_fft 256 | 512
    assert capi.n_fft(below) == 256 and capi.n_fft(above) == 512
    lams = [below, 128.0, 40.0]
    x, g, lengths = _x(11), _g(kind, 3, hop, 12), _len(MIXED)
    lay = _layer(kind, lams, hop)
    _, _, gx = _step(lay, x, g, lengths)
    assert torch.isfinite(gx).all()
    lay.lambd.data[0] = above                                     # across the boundary behind the host's back: no resync()
    got = _step(lay, x, g, lengths)
    cands = [n for n, mask in lay._plan_for(torch.device(DEV)).last_multi_launch() if mask & 1]
    assert 256 in cands and 512 in cands, cands
    want = _step(_layer(kind, [above, 128.0, 40.0], hop, sync=True), x, g, lengths)
    assert torch.isfinite(got[2]).all() and all(_same(u, v) for u, v in zip(got, want))
    ref, _, _ = _scalar_sum(kind, [above, 128.0, 40.0], x, g, lengths, hop=hop)
    assert _same(got[2], ref)
    lay.lambd.data[0] = 700.0                                     # n_fft 8192: no launch covers it
    y, _, gx = _step(lay, x, g, lengths)
    assert torch.isnan(_part(kind, 0, 3, y)).all() and torch.isnan(gx).all()
    with pytest.raises(RuntimeError, match="channel 0"):
        lay(x.clone().requires_grad_(True), lengths)


# ---- 7. captured step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["multi", "band"])
def test_a_captured_step_follows_the_lengths_rewritten_in_place(kind):
    hop, lams = 100, [300.0, 128.0, 85.3]
    x, g = _x(13), _g(kind, 3, hop, 14)
    lay = _layer(kind, lams, hop)
    lay.set_tracking(8, 1)                                        # both neighbours of every channel's n_fft, eagerly and under capture
    lengths = _len(MIXED)
    other = [8000, 1, 777, 4096, 2500, 130]
    xr = x.clone().requires_grad_(True)
    gx_out, dl_out = torch.empty_like(x), torch.empty(3, device=DEV)

    def step():
        gx, dl = torch.autograd.grad(lay(xr, lengths), (xr, lay.lambd), g)
        gx_out.copy_(gx)
        dl_out.copy_(dl)

    eager = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name, vals in (("other", other), ("mixed", MIXED)):
            lengths.copy_(_len(vals))
            step()                                                # eager: the first one sizes the workspace for the neighbours too
            eager[name] = (gx_out.clone(), dl_out.clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not _same(eager["other"][0], eager["mixed"][0]) and all(torch.isfinite(v[0]).all() for v in eager.values())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for name, vals in (("mixed", MIXED), ("other", other), ("mixed", MIXED)):
        lengths.copy_(_len(vals))
        gx_out.fill_(7.0)
        dl_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(gx_out, eager[name][0]) and _same(dl_out, eager[name][1]), name
    ref, _, _ = _scalar_sum(kind, lams, x, g, _len(MIXED), hop=hop)
    assert _same(eager["mixed"][0], ref)
    for k in range(3):
        assert lay.lambd_status(channel=k)["error"] == 0


# ---- 8. addresses -------------------------------------------------------------------------------------------------------------------------
def _off16(t):
    """a contiguous copy of t whose first element lies 4 bytes behind a 16-byte boundary"""
    buf = torch.full((t.numel() + 16,), float("nan"), device=t.device, dtype=t.dtype)
    pad = next(i for i in range(8) if (buf.data_ptr() + 4 * i) % 16 == 4)
    view = buf[pad:pad + t.numel()].view_as(t)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _step_at(layer, x, g, lengths):
    """_step on x and g themselves (no clone): their addresses reach the kernels"""
    layer.lambd.grad = None
    xr = x.requires_grad_(True)
    y = layer(xr, lengths)
    y.backward(g)
    torch.cuda.synchronize()
    return y.detach(), layer.lambd.grad.detach().clone(), xr.grad.detach()


@pytest.mark.parametrize("lams", [WAVE, LDS], ids=SET_IDS[:2])
@pytest.mark.parametrize("kind", ["multi", "band_uneven"])
@pytest.mark.parametrize("hop", [100, 250])
def test_unaligned_x_and_cotangent(kind, lams, hop):
    """The cotangent at a 4-byte offset: the bits of the aligned run.  x at a 4-byte offset as well: the forward kernels and the x-gradient
    kernels' own clip sum add an unaligned clip up in another order (dword loads and one accumulator instead of float4 loads
    and four), so the output itself -- kernels this layer shares with every other one -- differs from the aligned run in the last bits of
    the clip mean (measured: y differs in all 16 cases, x.grad by at most 2.1e-6 of a clip's maximum; printed below).  What holds on bits is the contract:
    the K scalar layers fed the same views; against the aligned run each clip meets the x-gradient bar TOL, both being evaluations of
    the same function that round the clip mean differently."""
    K = len(lams)
    x, g, lengths = _x(15), _g(kind, K, hop, 16), _len(MIXED)
    for norm in (False, True):                                    # the kernel's own clip sum and dmel_prep_kernel's
        lay = _layer(kind, lams, hop, norm=norm)
        want = _step(lay, x, g, lengths)
        gv = _off16(g)
        got = _step_at(lay, x.clone(), gv, lengths)
        assert gv.data_ptr() % 16 == 4 and all(_same(u, v) for u, v in zip(got, want)), norm
        xv = _off16(x)
        y, d, gx = _step_at(lay, xv, gv, lengths)
        assert xv.data_ptr() % 16 == 4 and torch.isfinite(gx).all() and _zero_past(gx, MIXED)
        acc = torch.zeros_like(x)
        for k, (lam, gk) in enumerate(zip(lams, _channel_cotangents(kind, g, K))):
            yk, dk, gxk = _step_at(_scalar(lam, hop, norm=norm), _off16(x), _off16(gk), lengths)
            acc = acc + gxk
            assert _same(_part(kind, k, K, y), _part(kind, k, K, yk, scalar=True)) and _same(d[k].reshape(()), dk.reshape(())), (norm, k)
        assert _same(gx, acc), (norm, float((gx - acc).abs().max()))
        errs = []
        for b, lb in enumerate(MIXED):
            diff, top = float((gx[b, :lb] - want[2][b, :lb]).abs().max()), float(want[2][b, :lb].abs().max())
            errs.append(diff / top if top > 0 else (0.0 if diff == 0 else float("inf")))
        print("klen xgrad unaligned x against aligned x", kind, lams, hop, norm, _same(y, want[0]), errs)
        assert max(errs) <= TOL, errs


def test_argument_checks_behind_a_live_plan():
    """every NULL or malformed argument and a grad_x that is not 16-byte aligned: DMEL_ERR_INVALID_ARGUMENT, and grad_x stays as it was"""
    lib, bad = capi.load(), capi.DMEL_ERR_INVALID_ARGUMENT
    hop = 100
    x, lengths = _x(17), _len(MIXED)
    gx = torch.full((B * L + 4,), 7.0, device=DEV)
    lam_host = (C.c_float * 3)(*WAVE)
    ns, masks = (C.c_int32 * 24)(256, 1024), (C.c_uint32 * 24)(3, 4)
    good = (C.c_int32 * 4)(*_edges("band"))
    for kind in ("multi", "band"):
        lay = _layer(kind, WAVE, hop, log=False)
        g = _g(kind, 3, hop, 18)
        h = lay._plan_for(torch.device(DEV))._h
        lam_dev = lay.lambd.detach().data_ptr()
        ed = () if kind == "multi" else (good,)

        def host(x_=x.data_ptr(), ln=lengths.data_ptr(), lam=lam_host, K=3, ed=ed, flags=0, g_=g.data_ptr(), gx_=gx.data_ptr()):
            fn = lib.dmel_backward_x_multi_lengths if kind == "multi" else lib.dmel_backward_x_band_lengths
            return fn(h, x_, ln, B, lam, K, *ed, flags, g_, None, gx_, None)

        def dev(x_=x.data_ptr(), ln=lengths.data_ptr(), lam=lam_dev, K=3, ed=ed, ns_=ns, masks_=masks, count=2, flags=0, g_=g.data_ptr(),
                gx_=gx.data_ptr()):
            fn = lib.dmel_backward_x_multi_dev_lengths if kind == "multi" else lib.dmel_backward_x_band_dev_lengths
            return fn(h, x_, ln, B, lam, K, *ed, ns_, masks_, count, flags, g_, None, gx_, None)

        for fn in (host, dev):
            assert fn(gx_=gx.data_ptr() + 4) == bad
            msg = (lib.dmel_last_error() or b"").decode("utf-8", "replace")
            assert "grad_x" in msg and "16" in msg, msg
            for kw in ({"x_": None}, {"ln": None}, {"g_": None}, {"gx_": None}, {"lam": None}, {"flags": capi.DMEL_FLAG_LOG},
                       {"flags": capi.DMEL_FLAG_CHECK_NFFT}, {"K": 0}, {"K": 9}):
                assert fn(**kw) == bad, (kind, fn.__name__, kw)
            if kind == "band":
                for e in (None, (C.c_int32 * 4)(0, 10, 21, 31), (C.c_int32 * 4)(0, 21, 21, 32)):
                    assert fn(ed=(e,)) == bad, list(e or [])
        for kw in ({"ns_": None}, {"masks_": None}, {"count": 0}, {"masks_": (C.c_uint32 * 24)(3, 0)}, {"masks_": (C.c_uint32 * 24)(3, 8)},
                   {"masks_": (C.c_uint32 * 24)(1, 4)}, {"ns_": (C.c_int32 * 24)(1024, 256)}, {"ns_": (C.c_int32 * 24)(256, 1000)}):
            assert dev(**kw) == bad, (kind, kw)
    torch.cuda.synchronize()
    assert bool((gx == 7.0).all())


# ---- 9. oracle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lams", SETS, ids=SET_IDS)
@pytest.mark.parametrize("kind", ["multi", "band_uneven"])
def test_clip_by_clip_against_the_oracle(kind, lams):
    """per clip max |got - ref| / max |ref| over the clip's samples, ref the sum over channels of the fp64 oracle's x-gradient at the clip's
    own length and valid frames; the clip of one sample must be exactly zero"""
    from oracle import dmel_oracle as O
    hop, K = 100, len(lams)
    x, g, lengths = _x(19), _g(kind, K, hop, 20), _len(MIXED)
    for log in (True, False):
        y, _, gx = _step(_layer(kind, lams, hop, log), x, g, lengths)
        x_np, gx_np = x.cpu().numpy(), gx.double().cpu().numpy()
        gks = [gk.cpu().numpy() for gk in _channel_cotangents(kind, g, K)]
        y_np = y.float().cpu().numpy()
        errs = []
        for b, lb in enumerate(MIXED):
            tb = lb // hop + 1
            ref = 0.0
            for k, lam in enumerate(lams):
                yk = y_np[b:b + 1, k:k + 1] if kind == "multi" else y_np[b:b + 1]
                ref = ref + O.backward_x(x_np[b:b + 1, :lb], lam, hop, SR, np.ascontiguousarray(gks[k][b:b + 1, :, :, :tb]),
                                         np.ascontiguousarray(yk[:, :, :, :tb]) if log else None)
            diff, top = float(np.abs(gx_np[b:b + 1, :lb] - ref).max()), float(np.abs(ref).max())
            errs.append(diff / top if top > 0 else (0.0 if diff == 0 else float("inf")))
        print("klen xgrad oracle", kind, lams, log, errs)
        assert int(_bits(gx[4]).abs().max()) == 0                 # the clip of one sample: reference and result are zero
        assert errs[4] == 0.0 and max(errs) <= TOL, errs


# ---- 10. fp64 x -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["multi", "band"])
def test_fp64_waveform(kind):
    """see the head of the file: bit for bit against the K scalar layers' sum on the clip the kernels read, taken through the layer's own fp64
    conversion; and within fp32 rounding of K scalar layers each fed the fp64 x"""
    from dmel_amd.layer import _as_f32_contiguous
    hop, lams = 100, WAVE
    x, g, lengths = _x(21).double() + 0.25, _g(kind, 3, hop, 22), _len(MIXED)
    y, d, gx = _step(_layer(kind, lams, hop), x, g, lengths)
    assert gx.dtype == torch.float64 and _zero_past(gx, MIXED) and torch.isfinite(gx).all()
    xr = x.detach().clone().requires_grad_(True)
    xf = _as_f32_contiguous(xr, lengths)
    sum32, ys, dls = _scalar_sum(kind, lams, xf.detach(), g, lengths, hop=hop)
    xf.backward(sum32)
    assert _same(gx, xr.grad), float((gx - xr.grad).abs().max())
    for k in range(3):
        assert _same(_part(kind, k, 3, y), _part(kind, k, 3, ys[k], scalar=True)) and _same(d[k].reshape(()), dls[k].reshape(()))
    sum64, _, _ = _scalar_sum(kind, lams, x, g, lengths, hop=hop)
    assert sum64.dtype == torch.float64
    terms = max(float(_step(_scalar(lam, hop), x, gk, lengths)[2].abs().max()) for lam, gk in zip(lams, _channel_cotangents(kind, g, 3)))
    diff = float((gx - sum64).abs().max())
    print("klen xgrad fp64", kind, diff, terms)
    assert diff <= 4 * 2.0 ** -24 * terms, (diff, terms)
