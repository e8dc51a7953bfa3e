"""The staged epilogue of the wave-local contraction stores its whole 16-byte pieces of `out` and `tangent` as write-through buffer
stores (csrc/dmel_fwd_body.inc, DMEL_WL_WT).  An out-of-range buffer store is dropped without a trace and a wrong offset lands
somewhere else, so every case here runs one forward into outputs PRE-FILLED with NaN that sit inside a larger allocation with
sentinels on both sides, and asserts afterwards: no NaN left, every element of `out` and `tangent` against the fp64 oracle (output:
plain relative 1e-4 on every element, no floor; tangent: 1e-4 of the element's cancellation-free magnitude, tests/tangent_cases.py),
and the sentinels untouched.  The shapes are the smallest that reach every branch of the staged loop (T % 4 == 0, fp32 output,
tangent asked for, n_fft 1024 at 16 frames per tile, n_fft 2048 at one frame per wave); the last test puts the consumer of the
tangent, the d lambd dot product, right behind the kernel boundary thirty times over."""
import functools

import numpy as np
import pytest
import torch

from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from tangent_cases import assert_tangent
from test_hip_parity import TOL, _dlam_tol, assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-10
SR, HOP = 16000, 512
GUARD = 64                     # fp32 elements on each side: two 128-byte lines
SENTINEL = -7777.0


def _guarded(shape):
    """(buffer, view): `view` of `shape`, NaN-filled and 16-byte aligned, inside `buffer` with GUARD sentinels before and behind it"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def _assert_guards(tag, *bufs):
    for buf in bufs:
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), (tag, "a store landed outside the tensor")


def _length(T):
    """a clip of T frames at HOP whose length is no multiple of the hop"""
    return (T - 1) * HOP + 5 if T != 32 else 16000


@functools.lru_cache(maxsize=None)
def _clips(B, L, seed):
    from dmel_amd import synth
    x = synth.waveforms(B, L, seed=seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(B, L, seed, lam, M, log):
    """(out, tangent, scale) of the fp64 oracle (scale: the cancellation-free magnitude of every tangent element); read-only, shared"""
    x = _clips(B, L, seed)
    o, t = O.forward(x, lam, HOP, M, SR, apply_log=log)
    _, _, sc = R.tangent_fp64(x, lam, HOP, M, SR, log=log)
    res = (o, t, np.asarray(sc))
    for a in res:
        a.setflags(write=False)
    return res


def _check(tag, log, o, t, o_ref, t_ref, scale):
    """no NaN left, then every element against the oracle"""
    assert not np.isnan(o).any(), (tag, "out: a piece was not written", np.argwhere(np.isnan(o))[:4])
    assert not np.isnan(t).any(), (tag, "tangent: a piece was not written", np.argwhere(np.isnan(t))[:4])
    if log:
        assert_parity(tag + "/exp_logmel", np.exp(o.astype(np.float64)), np.exp(np.asarray(o_ref, dtype=np.float64)), allow_floor=False)
    else:
        assert_parity(tag + "/mel", o, o_ref, allow_floor=False)
    assert_tangent(tag + "/tangent", t, t_ref, scale, shape=t.shape)


# (B, M, T, lambd): lambd 128 -> n_fft 1024, 16 frames per tile; lambd 256 -> n_fft 2048, one frame per wave
SCALAR = [(3, 128, 4, 128.0), (3, 40, 4, 128.0), (3, 128, 20, 128.0), (3, 40, 20, 128.0), (3, 128, 32, 128.0), (3, 40, 32, 128.0),
          (2, 64, 32, 256.0)]


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("B,M,T,lam", SCALAR, ids=[f"B{b}_M{m}_T{t}_lam{int(l)}" for b, m, t, l in SCALAR])
def test_staged_epilogue_writes_every_piece_and_nothing_else(B, M, T, lam, log):
    from dmel_amd import capi
    L = _length(T)
    assert L // HOP + 1 == T and T % 4 == 0
    tag = f"write_through/B{B}_M{M}_T{T}_lam{int(lam)}/{'log' if log else 'lin'}"
    x = torch.from_numpy(np.array(_clips(B, L, 7))).to(DEV)
    obuf, out = _guarded((B, 1, M, T))
    tbuf, tan = _guarded((B, 1, M, T))
    plan = capi.Plan(L, HOP, M, SR)
    plan.forward(x.data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), log, EPS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    info = plan.info()
    plan.close()
    assert info["n_fft"] == O.n_fft(lam) and info["n_time"] == T and info["kernel_path"] == 0 and info["contraction"] == 1, (tag, info)
    _check(tag, log, out.cpu().numpy(), tan.cpu().numpy(), *_reference(B, L, 7, lam, M, log))
    _assert_guards(tag, obuf, tbuf)


K_LAMS = [128.0, 256.0, 100.0]             # n_fft 1024, 2048, 1024
K_EDGES = [0, 5, 30, 40]                   # a group's rows start inside the shared image


@pytest.mark.parametrize("which", ["multi_window", "band_split"])
def test_multi_window_and_band_split(which):
    """the K-window builds of the same body through the C ABI into guarded outputs (per-channel images; one shared image whose row
    groups belong to different launches), then the layers on the same clips"""
    from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram, capi, synth
    B, M, T, log = 3, 40, 32, True
    L, K = _length(T), len(K_LAMS)
    band = which == "band_split"
    x_np = _clips(B, L, 11)
    x = torch.from_numpy(np.array(x_np)).to(DEV)
    shape = (B, 1 if band else K, M, T)
    obuf, out = _guarded(shape)
    tbuf, tan = _guarded(shape)
    plan = capi.Plan(L, HOP, M, SR)
    scr = torch.zeros((plan.scratch_bytes_multi(B, K),), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if band:
        plan.forward_band(x.data_ptr(), B, K_LAMS, K_EDGES, out.data_ptr(), tan.data_ptr(), log, EPS, st, scr.data_ptr())
    else:
        plan.forward_multi(x.data_ptr(), B, K_LAMS, out.data_ptr(), tan.data_ptr(), log, EPS, st, scr.data_ptr())
    torch.cuda.synchronize()
    plan.close()
    o, t = out.cpu().numpy(), tan.cpu().numpy()
    refs = [_reference(B, L, 11, lam, M, log) for lam in K_LAMS]

    def rows(a, c, own):
        """channel c's part of `a`: the device's layout (own=False) or one oracle image (own=True)"""
        if band:
            return a[:, :, K_EDGES[c]:K_EDGES[c + 1]]
        return a if own else a[:, c:c + 1]

    for c in range(K):
        _check(f"write_through/{which}/c{c}", log, rows(o, c, False), rows(t, c, False), *(rows(np.asarray(r), c, True) for r in refs[c]))
    _assert_guards(which, obuf, tbuf)

    if band:
        lay = BandSplitMelSpectrogram(K_LAMS, M, L, SR, hop_length=HOP, band_edges=K_EDGES, log=log).to(DEV)
    else:
        lay = MultiWindowMelSpectrogram(K_LAMS, M, L, SR, hop_length=HOP, log=log).to(DEV)
    g_np = (synth.cotangent(shape, seed=12) + np.float32(1.0)).astype(np.float32)
    y = lay(x)
    (y * torch.from_numpy(g_np).to(DEV)).sum().backward()
    yo, dl = y.detach().cpu().numpy(), lay.lambd.grad.cpu().numpy().astype(np.float64)
    for c in range(K):
        o_ref, t_ref, _ = refs[c]
        assert_parity(f"write_through/{which}/layer/c{c}", np.exp(rows(yo, c, False).astype(np.float64)),
                      np.exp(rows(np.asarray(o_ref), c, True).astype(np.float64)), allow_floor=False)
        gc = np.zeros((B, 1, M, T), np.float32)
        if band:
            gc[:, :, K_EDGES[c]:K_EDGES[c + 1]] = g_np[:, :, K_EDGES[c]:K_EDGES[c + 1]]
        else:
            gc[:] = g_np[:, c:c + 1]
        exp_d = O.backward(gc, t_ref)
        assert abs(dl[c] - exp_d) <= _dlam_tol(exp_d, gc, t_ref), (which, c, dl[c], exp_d)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
def test_lengths_inside_the_second_tile(log):
    """T = 32 is two tiles of 16 frames; clips that end inside the second one: their pad frames and the write-through pieces of the
    frames before them share 128-byte lines.  Frames of a clip: the oracle at that length.  Pad frames: log(eps) or 0, tangent 0."""
    from dmel_amd import capi
    B, M, T, lam = 3, 128, 32, 128.0
    L = _length(T)
    lens = [20 * HOP + 100, 26 * HOP + 7, L]                 # 21, 27 and all 32 frames
    tag = f"write_through/lengths/{'log' if log else 'lin'}"
    x_np = np.array(_clips(B, L, 13))
    for b, lc in enumerate(lens):
        x_np[b, lc:] = np.nan                                # what lies behind a clip is never read
    x = torch.from_numpy(x_np).to(DEV)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    obuf, out = _guarded((B, 1, M, T))
    tbuf, tan = _guarded((B, 1, M, T))
    plan = capi.Plan(L, HOP, M, SR)
    plan.forward_lengths(x.data_ptr(), lengths.data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), log, EPS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    o, t = out.cpu().numpy(), tan.cpu().numpy()
    assert not np.isnan(o).any() and not np.isnan(t).any(), tag
    for b, lc in enumerate(lens):
        tc = lc // HOP + 1
        assert 16 < tc <= T
        xb = np.ascontiguousarray(_clips(B, L, 13)[b:b + 1, :lc])
        o_ref, t_ref = O.forward(xb, lam, HOP, M, SR, apply_log=log)
        _, _, sc = R.tangent_fp64(xb, lam, HOP, M, SR, log=log)
        _check(f"{tag}/clip{b}", log, o[b:b + 1, :, :, :tc], t[b:b + 1, :, :, :tc], o_ref, t_ref, np.asarray(sc))
        assert (t[b, :, :, tc:] == 0).all(), (tag, b)
        if log:
            assert np.abs(o[b, :, :, tc:].astype(np.float64) - np.log(EPS)).max(initial=0.0) <= TOL, (tag, b)
        else:
            assert (o[b, :, :, tc:] == 0).all(), (tag, b)
    _assert_guards(tag, obuf, tbuf)


def test_the_dot_product_behind_the_boundary_reads_this_iterations_tangent():
    """thirty forwards, each followed on the same stream by the d lambd dot product over the tangent it has just written, two seeded
    batches and cotangents in turn: d lambd of every iteration is the fp64 dot product of THAT iteration's tangent (copied off behind
    the dot product) and cotangent.  The kernel forms every product and the whole sum in fp64 and rounds once to fp32, so the two
    differ by that rounding (2^-24 relative) and by the order of an fp64 sum of n terms (n 2^-53 sum |g t|); a line of the other
    batch's tangent served from a cache would be a gross mismatch."""
    from dmel_amd import capi, synth
    B, M, T, lam, n_it = 3, 128, 32, 128.0, 30
    L = _length(T)
    shape = (B, 1, M, T)
    n = int(np.prod(shape))
    xs = [torch.from_numpy(np.array(_clips(B, L, 21 + i))).to(DEV) for i in range(2)]
    g_np = [(synth.cotangent(shape, seed=31 + i) + np.float32(1.0)).astype(np.float32) for i in range(2)]
    gs = [torch.from_numpy(g).to(DEV) for g in g_np]
    out, tan = torch.empty(shape, device=DEV), torch.full(shape, float("nan"), device=DEV)
    dl = torch.full((n_it, 4), float("nan"), device=DEV)                # one 16-byte cell per iteration
    kept = torch.empty((n_it,) + shape, device=DEV)
    plan = capi.Plan(L, HOP, M, SR)
    st = torch.cuda.current_stream().cuda_stream
    for it in range(n_it):
        plan.forward(xs[it % 2].data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), True, EPS, st)
        plan.backward(gs[it % 2].data_ptr(), tan.data_ptr(), n, dl[it].data_ptr(), st)
        kept[it].copy_(tan)
    torch.cuda.synchronize()
    plan.close()
    d, k = dl[:, 0].cpu().numpy().astype(np.float64), kept.cpu().numpy().astype(np.float64)
    assert np.isfinite(d).all() and np.isfinite(k).all()
    assert not np.array_equal(k[0], k[1]) and np.array_equal(k[0], k[2]) and np.array_equal(k[1], k[3])
    for it in range(n_it):
        prod = g_np[it % 2].astype(np.float64) * k[it]
        want = float(prod.sum())
        tol = 2.0 ** -23 * abs(want) + n * 2.0 ** -53 * float(np.abs(prod).sum())
        assert abs(d[it] - want) <= tol, (it, d[it], want, tol)
    # ... and the tangent itself is the oracle's (both batches)
    for i in range(2):
        _, t_ref, sc = _reference(B, L, 21 + i, lam, M, True)
        assert_tangent(f"write_through/consumer/batch{i}", k[i].astype(np.float32), t_ref, sc, shape=shape)
