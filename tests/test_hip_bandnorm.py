"""BandNorm on the MI355X (dmel_bandnorm_forward / dmel_bandnorm_backward, dmel_amd.BandNorm): the C ABI and the module against the fp64
restatement of tests/bandnorm_cases.py with the fp32 restatement's own error as the yardstick, the exact properties (pad frames, guards,
full lengths, a clip alone, permutations, determinism, invalid lengths), BandNorm behind the mel layers and PCEN against the oracle's tangent,
and a captured step."""
import functools

import numpy as np
import pytest
import torch

import bandnorm_cases as N
import pcen_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -12345.5
IDS = [str(s) for s in N.SHAPES]
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(n):
    """n NaN floats between two runs of GUARD sentinel words; (whole buffer, the n floats as a view)"""
    t = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    t[GUARD:GUARD + n] = NAN
    return t, t[GUARD:GUARD + n]


def _guards_ok(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _poison(t, Tc):
    """a copy with NaN on every pad frame: what the kernels must never load"""
    if Tc is None:
        return t.clone()
    return t.masked_fill(~N.valid_mask(t.shape, Tc).expand(t.shape), NAN)


def _call(s, g, w, b, Tc, stats, ev, running=None, want=(True, True, True)):
    """the C ABI on device tensors (B, C, M, T): dict of y, ds, dweight, dbias, running_mean, running_var, num_batches_tracked (CPU tensors;
    what was not asked for stays NaN) and ``guards``: every sentinel word around the five outputs is intact"""
    from dmel_amd import capi
    B, C, M, T = s.shape
    rows, n = B * C * M, s.numel()
    batch = stats == "batch"
    stream = torch.cuda.current_stream().cuda_stream
    lens = None if Tc is None else Tc.to(DEV).to(torch.int32)
    (ybuf, y), (dsbuf, ds), (dwbuf, dw), (dbbuf, db) = _guarded(n), _guarded(n), _guarded(M), _guarded(M)
    rmbuf, rm = _guarded(M)
    rvbuf, rv = _guarded(M)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    if batch:
        rm.copy_(running[0]), rv.copy_(running[1])
    st = torch.full((M if batch else rows, 2), NAN, dtype=torch.float64, device=DEV)
    scratch = torch.full((capi.bandnorm_scratch_bytes(rows, M) // 8,), NAN, dtype=torch.float64, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    capi.bandnorm_forward(s.data_ptr(), rows, M, C * M, T, ptr(lens), ptr(w), ptr(b), batch, not ev, N.EPS, N.MOMENTUM, ptr(rm) if batch else None,
                          ptr(rv) if batch else None, ptr(nbt) if batch and not ev else None, y.data_ptr(), st.data_ptr(), scratch.data_ptr(), stream)
    if g is not None:
        scratch.fill_(NAN)
        capi.bandnorm_backward(g.data_ptr(), s.data_ptr(), st.data_ptr(), rows, M, C * M, T, ptr(lens), ptr(w), batch, not ev,
                               ptr(ds) if want[0] else None, ptr(dw) if want[1] else None, ptr(db) if want[2] else None, scratch.data_ptr(), stream)
    torch.cuda.synchronize()
    ok = all(_guards_ok(buf, k) for buf, k in ((ybuf, n), (dsbuf, n), (dwbuf, M), (dbbuf, M), (rmbuf, M), (rvbuf, M)))
    return {"y": y.cpu().reshape(s.shape), "ds": ds.cpu().reshape(s.shape), "dweight": dw.cpu(), "dbias": db.cpu(), "running_mean": rm.cpu(),
            "running_var": rv.cpu(), "num_batches_tracked": int(nbt), "guards": ok}


def _inputs(idx, with_lengths):
    shape = N.SHAPES[idx]
    s, g = N.inputs(shape, idx)
    return shape, s, g, N.params(shape[2], idx), (N.frame_lengths(shape, idx) if with_lengths else None)


@functools.lru_cache(maxsize=None)
def _refs(idx, stats, with_lengths, ev):
    """the fp64 and the fp32 restatement of one case (computed once, shared, never changed)"""
    shape, s, g, (w, b, rm, rv), Tc = _inputs(idx, with_lengths)
    d = lambda t: t.double()      # noqa: E731
    ref = N.backward(d(g), d(s), d(w), d(b), Tc, stats, running=(d(rm), d(rv)) if ev else None)
    r32 = N.backward(g, s, w, b, Tc, stats, running=(rm, rv) if ev else None)
    if stats == "batch" and not ev:
        for out, (nm, nv, sm, sv) in ((ref, N.updated_running(d(s), Tc, d(rm), d(rv))), (r32, N.updated_running(s, Tc, rm, rv))):
            out.update(running_mean=nm, running_var=nv, running_mean_scale=sm, running_var_scale=sv)
    return ref, r32


@functools.lru_cache(maxsize=None)
def _case(idx, stats, with_lengths, ev=False):
    """one run of the kernels for SHAPES[idx] through the C ABI, s and g NaN on every pad frame"""
    shape, s, g, (w, b, rm, rv), Tc = _inputs(idx, with_lengths)
    dev = [t.to(DEV) for t in (_poison(s, Tc), _poison(g, Tc), w, b, rm, rv)]
    out = _call(dev[0], dev[1], dev[2], dev[3], Tc, stats, ev, running=(dev[4], dev[5]))
    return dict(shape=shape, Tc=Tc, dev=dev, out=out)


def _against_fp64(idx, stats, with_lengths, ev, got):
    """every element of every quantity within 8 x the fp32 restatement's worst error on this case (capped at 1e-4), in units of the
    cancellation-free scales; returns the ratios kernel / restatement"""
    ref, r32 = _refs(idx, stats, with_lengths, ev)
    names = ["y", "ds", "dweight", "dbias"] + (["running_mean", "running_var"] if stats == "batch" and not ev else [])
    failed, ratios = [], {}
    for k in names:
        scale = ref[k + "_scale"]
        w_kernel, w_fp32 = N.worst(got[k], ref[k], scale), N.worst(r32[k], ref[k], scale)
        bound = min(8.0 * w_fp32, 1e-4)
        ratios[k] = w_kernel / w_fp32 if w_fp32 else (0.0 if w_kernel == 0 else float("inf"))
        print(f"bandnorm {N.SHAPES[idx]} {stats} {'eval' if ev else 'train'} {'lengths' if with_lengths else 'full'} {k}: kernel {w_kernel:.3e} "
              f"fp32 restatement {w_fp32:.3e} ratio {ratios[k]:.2f} bound {bound:.3e}")
        if not w_kernel <= bound:
            failed.append((k, w_kernel, w_fp32))
    assert not failed, (N.SHAPES[idx], stats, ev, with_lengths, failed)
    return ratios


def _pad_frames_and_guards(c):
    """y and ds are +0.0 on every pad frame, sign bit included, finite elsewhere; nothing is written outside the outputs"""
    out, shape = c["out"], c["shape"]
    pad = ~N.valid_mask(shape, c["Tc"]).expand(shape)
    for k in ("y", "ds"):
        assert bool((_bits(out[k])[pad] == 0).all()), k
        assert bool(torch.isfinite(out[k][~pad]).all()), k
    assert bool(torch.isfinite(out["dweight"]).all()) and bool(torch.isfinite(out["dbias"]).all())
    assert out["guards"]


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
@pytest.mark.parametrize("stats", ["clip", "batch"])
@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_c_abi_against_fp64_within_eight_times_the_fp32_restatement(idx, stats, with_lengths):
    """Errors in units of the cancellation-free scales of bandnorm_cases.backward; the bound is PCEN's rule (8 x the fp32 torch restatement's
    worst error for that quantity on that case, never more than 1e-4; an element of zero scale -- every pad frame -- must be exact).
    The worst ratios kernel / restatement are in DESIGN 4.14."""
    c = _case(idx, stats, with_lengths)
    _against_fp64(idx, stats, with_lengths, False, c["out"])
    _pad_frames_and_guards(c)
    assert c["out"]["num_batches_tracked"] == (1 if stats == "batch" else 0)


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_eval_mode_uses_the_running_buffers_and_leaves_them_alone(idx, with_lengths):
    c = _case(idx, "batch", with_lengths, True)
    _against_fp64(idx, "batch", with_lengths, True, c["out"])
    _pad_frames_and_guards(c)
    assert torch.equal(_bits(c["out"]["running_mean"]), _bits(c["dev"][4].cpu())) and torch.equal(_bits(c["out"]["running_var"]), _bits(c["dev"][5].cpu()))
    assert c["out"]["num_batches_tracked"] == 0


def _module(M, stats, prm, ev=False):
    import dmel_amd
    m = dmel_amd.BandNorm(M, stats=stats, eps=N.EPS, momentum=N.MOMENTUM)
    with torch.no_grad():
        m.weight.copy_(prm[0]), m.bias.copy_(prm[1])
        if stats == "batch":
            m.running_mean.copy_(prm[2]), m.running_var.copy_(prm[3])
    return m.to(DEV).train(not ev)


def _module_step(m, s, g, Tc):
    """one forward + backward of the module: the dict _call returns (without the guards)"""
    m.zero_grad()
    x = s.detach().requires_grad_(True)                       # (not a copy: a strided view stays one)
    y = m(x, Tc)
    y.backward(g)
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu(), "ds": x.grad.cpu(), "dweight": m.weight.grad.cpu(), "dbias": m.bias.grad.cpu()}
    if m.stats == "batch":
        out.update(running_mean=m.running_mean.cpu().clone(), running_var=m.running_var.cpu().clone(), num_batches_tracked=int(m.num_batches_tracked))
    return out


SAME = ("y", "ds", "dweight", "dbias", "running_mean", "running_var")


def _same_bits(a, b, names=SAME):
    for k in names:
        if k in a and k in b:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("stats,ev", [("clip", False), ("batch", False), ("batch", True)], ids=["clip", "batch", "batch_eval"])
@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_module_gives_the_c_abi_bits(idx, stats, ev):
    """dmel_amd.BandNorm with int64 frame_lengths (narrowed on the device), a (B, n_mels, T) view where there is one channel, and a
    non-contiguous input: output, gradients and running buffers are those of the C ABI, which the tests above hold to fp64"""
    c = _case(idx, stats, True, ev)
    s, g, w, b, rm, rv = c["dev"]
    B, C, M, T = c["shape"]
    m = _module(M, stats, (w, b, rm, rv), ev)
    Tc = c["Tc"].to(DEV)
    assert Tc.dtype == torch.int64
    got = _module_step(m, s, g, Tc)
    _same_bits(got, c["out"])
    if stats == "batch":
        assert got["num_batches_tracked"] == (0 if ev else 1)
        _module_step(m, s, g, Tc)
        assert int(m.num_batches_tracked) == (0 if ev else 2)
    if C == 1:
        m3 = _module(M, stats, (w, b, rm, rv), ev)
        got3 = _module_step(m3, s.reshape(B, M, T), g.reshape(B, M, T), Tc.to(torch.int32))
        assert got3["y"].shape == (B, M, T)
        _same_bits({k: v.reshape(c["shape"]) if torch.is_tensor(v) and v.dim() == 3 else v for k, v in got3.items()}, c["out"])
    wide = torch.full((B, C, M, T + 3), NAN, device=DEV)
    wide[..., :T] = s
    m4 = _module(M, stats, (w, b, rm, rv), ev)
    _same_bits(_module_step(m4, wide[..., :T], g, Tc), c["out"])


@pytest.mark.parametrize("stats,ev", [("clip", False), ("batch", False), ("batch", True)], ids=["clip", "batch", "batch_eval"])
@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_full_lengths_give_the_bits_of_none(idx, stats, ev):
    c = _case(idx, stats, False, ev)
    s, g, w, b, rm, rv = c["dev"]
    full = torch.full((c["shape"][0],), c["shape"][-1], dtype=torch.int64)
    out = _call(s, g, w, b, full, stats, ev, running=(rm, rv))
    _same_bits(out, c["out"])
    assert out["guards"] and out["num_batches_tracked"] == c["out"]["num_batches_tracked"]


@pytest.mark.parametrize("idx", [2, 4, 6, 8, 9], ids=lambda i: IDS[i])
def test_clip_statistics_are_the_clips_alone(idx):
    """y[b, ..., :Tc] and ds equal, bit for bit, the same clip run alone as a T = Tc tensor (a shorter row sits in the same lanes of the
    same butterfly, the lanes past it add exact zeros); a permuted batch gives permuted bits"""
    c = _case(idx, "clip", True)
    s, g, w, b, rm, rv = c["dev"]
    B = c["shape"][0]
    for bi in range(B):
        tc = int(c["Tc"][bi])
        alone = _call(s[bi:bi + 1, :, :, :tc].contiguous(), g[bi:bi + 1, :, :, :tc].contiguous(), w, b, None, "clip", False)
        for k in ("y", "ds"):
            assert torch.equal(_bits(alone[k][0]), _bits(c["out"][k][bi, :, :, :tc])), (bi, k)
    perm = torch.arange(B - 1, -1, -1)
    out = _call(s[perm.to(DEV)].contiguous(), g[perm.to(DEV)].contiguous(), w, b, c["Tc"][perm], "clip", False)
    for k in ("y", "ds"):
        assert torch.equal(_bits(out[k]), _bits(c["out"][k][perm])), k


@pytest.mark.parametrize("stats", ["clip", "batch"])
@pytest.mark.parametrize("idx", [3, 9, 10, 11, 12], ids=lambda i: IDS[i])
def test_two_runs_give_the_same_bits(idx, stats):
    c = _case(idx, stats, True)
    s, g, w, b, rm, rv = c["dev"]
    again = _call(s, g, w, b, c["Tc"], stats, False, running=(rm, rv))
    _same_bits(again, c["out"])


@pytest.mark.parametrize("stats", ["clip", "batch"])
@pytest.mark.parametrize("idx", [3, 9, 10], ids=lambda i: IDS[i])
def test_null_outputs_leave_the_others_at_their_bits(idx, stats):
    c = _case(idx, stats, True)
    s, g, w, b, rm, rv = c["dev"]
    for want in ((True, False, False), (False, True, True), (False, False, True)):
        out = _call(s, g, w, b, c["Tc"], stats, False, running=(rm, rv), want=want)
        for k, asked in zip(("ds", "dweight", "dbias"), want):
            if asked:
                assert torch.equal(_bits(out[k]), _bits(c["out"][k])), (want, k)
            else:
                assert bool(torch.isnan(out[k]).all()), (want, k)
        assert out["guards"]


@pytest.mark.parametrize("bad_length", ["zero", "T_plus_one"])
@pytest.mark.parametrize("stats", ["clip", "batch"])
@pytest.mark.parametrize("idx", [3, 6, 9, 10], ids=lambda i: IDS[i])
def test_an_invalid_length_poisons_its_own_clip_only(idx, stats, bad_length):
    """The last clip gets a length outside 1 ... T: every frame of its rows is NaN in y and ds, and every other row, the running buffers and
    the parameter gradients have the bits of the batch without that clip.  (The last one: the rows before it keep their places in the fixed
    order of the band sums, and the invalid rows add exact zeros.  An invalid clip in front moves the rows behind it to other lanes of that
    order: the band sums then agree to fp64 rounding, not by construction bit for bit -- the row-wise quantities still do, below.)"""
    shape, s, g, (w, b, rm, rv), Tc = _inputs(idx, True)
    B, T = shape[0], shape[-1]
    Tc = Tc.clone()
    Tc[-1] = 0 if bad_length == "zero" else T + 1
    dev = [t.to(DEV) for t in (_poison(s, Tc.clamp(1, T)), _poison(g, Tc.clamp(1, T)), w, b, rm, rv)]
    out = _call(dev[0], dev[1], dev[2], dev[3], Tc, stats, False, running=(dev[4], dev[5]))
    assert out["guards"]
    assert bool(torch.isnan(out["y"][-1]).all()) and bool(torch.isnan(out["ds"][-1]).all())
    rest = _call(dev[0][:-1].contiguous(), dev[1][:-1].contiguous(), dev[2], dev[3], Tc[:-1], stats, False, running=(dev[4], dev[5]))
    assert bool(torch.isfinite(rest["y"]).all())
    for k in ("y", "ds"):
        assert torch.equal(_bits(out[k][:-1]), _bits(rest[k])), k
    _same_bits(out, rest, ("dweight", "dbias", "running_mean", "running_var"))
    assert out["num_batches_tracked"] == rest["num_batches_tracked"]
    if stats == "clip":
        # the first clip invalid: the rows of the others are the clean run's
        Tc0 = N.frame_lengths(shape, idx)
        clean = _case(idx, "clip", True)
        Tc0[0] = 0 if bad_length == "zero" else T + 1
        front = _call(clean["dev"][0], clean["dev"][1], dev[2], dev[3], Tc0, "clip", False)
        assert bool(torch.isnan(front["y"][0]).all()) and bool(torch.isnan(front["ds"][0]).all())
        for k in ("y", "ds"):
            assert torch.equal(_bits(front[k][1:]), _bits(clean["out"][k][1:])), k


def test_every_clip_invalid_leaves_the_buffers_alone():
    shape, s, g, (w, b, rm, rv), _ = _inputs(3, True)
    Tc = torch.tensor([0, shape[-1] + 1, -7, 0])
    dev = [t.to(DEV) for t in (s, g, w, b, rm, rv)]
    out = _call(dev[0], dev[1], dev[2], dev[3], Tc, "batch", False, running=(dev[4], dev[5]))
    assert bool(torch.isnan(out["y"]).all()) and bool(torch.isnan(out["ds"]).all()) and out["guards"]
    assert torch.equal(_bits(out["running_mean"]), _bits(rm)) and torch.equal(_bits(out["running_var"]), _bits(rv))
    assert bool((out["dweight"] == 0).all()) and bool((out["dbias"] == 0).all())


def test_a_band_with_one_valid_frame_keeps_its_running_var():
    s, g = N.inputs((1, 1, 3, 5), 77)
    w, b, rm, rv = N.params(3, 77)
    dev = [t.to(DEV) for t in (s, g, w, b, rm, rv)]
    out = _call(dev[0], dev[1], dev[2], dev[3], torch.tensor([1]), "batch", False, running=(dev[4], dev[5]))
    assert torch.equal(_bits(out["running_var"]), _bits(rv))
    want = ((1 - N.MOMENTUM) * rm.double() + N.MOMENTUM * s[0, 0, :, 0].double()).float()
    assert torch.allclose(out["running_mean"], want, rtol=1e-6, atol=0.0)
    assert torch.equal(_bits(out["y"][0, 0, :, 0]), _bits(b))            # one frame: yh = 0, y = bias


def test_a_nan_inside_the_valid_frames_spreads_as_through_batch_norm():
    c = _case(9, "batch", True)
    s, g, w, b, rm, rv = c["dev"]
    B, C, M, T = c["shape"]
    bad = s.clone()
    bad[1, 2, 3, 0] = NAN
    out = _call(bad, g, w, b, c["Tc"], "batch", False, running=(rm, rv))
    valid = N.valid_mask(c["shape"], c["Tc"]).expand(c["shape"])
    assert bool(torch.isnan(out["y"][:, :, 3][valid[:, :, 3]]).all()) and bool(torch.isnan(out["running_mean"][3]))
    keep = [m for m in range(M) if m != 3]
    for k in ("y", "ds"):
        assert torch.equal(_bits(out[k][:, :, keep]), _bits(c["out"][k][:, :, keep])), k
        assert bool((_bits(out[k])[~valid] == 0).all()), k
    for k in ("dweight", "dbias", "running_mean", "running_var"):
        assert torch.equal(_bits(out[k][keep]), _bits(c["out"][k][keep])), k
    clip = _call(bad, g, w, b, c["Tc"], "clip", False)
    clean = _case(9, "clip", True)["out"]
    rows = torch.ones(B, C, M, dtype=torch.bool)
    rows[1, 2, 3] = False
    assert bool(torch.isnan(clip["y"][1, 2, 3][valid[1, 2, 3]]).all())
    assert torch.equal(_bits(clip["y"][rows]), _bits(clean["y"][rows])) and torch.equal(_bits(clip["ds"][rows]), _bits(clean["ds"][rows]))


# ---- behind the layers -------------------------------------------------------------------------------------------------------------
SR, M_L, B_L = 16000, 8, 3
LAM, L_L, HOP = 128.0, 4000, 50            # n_fft 1024, 81 frames: two frame tiles (the shape of test_hip_pcen.py's lengths test)
LENS = [L_L, 1234, 50]


def _x():
    from dmel_amd import synth
    return synth.waveforms(B_L, L_L, seed=3)


def _oracle_pieces(x_np, lams, log):
    """(K, B, 1, M, T) outputs and tangents of the oracle, clip by clip at the clip's own length; pad frames 0"""
    from oracle import dmel_oracle as O
    T = L_L // HOP + 1
    out, tan = np.zeros((len(lams), B_L, 1, M_L, T)), np.zeros((len(lams), B_L, 1, M_L, T))
    for k, lam in enumerate(lams):
        for b, lb in enumerate(LENS):
            o, t = O.forward(x_np[b:b + 1, :lb], lam, HOP, M_L, SR, apply_log=log)
            out[k, b, :, :, :lb // HOP + 1], tan[k, b, :, :, :lb // HOP + 1] = o[0], t[0]
    return out, tan


def _check_dlambd(name, grad, d_out, tans):
    for k, t in enumerate(tans):
        prod = d_out[:, k:k + 1] * torch.from_numpy(t).double() if d_out.shape[1] > 1 else d_out * torch.from_numpy(t).double()
        d_ref, mag = float(prod.sum()), float(prod.abs().sum())
        d = float(grad.reshape(-1)[k])
        print(f"bandnorm behind {name} k={k}: d={d!r} d_ref={d_ref!r} |d - d_ref| / sum|dS t| = {abs(d - d_ref) / mag:.3e}")
        assert abs(d - d_ref) <= 1e-4 * mag, (name, k, d, d_ref, mag)


@pytest.mark.parametrize("stats", ["clip", "batch"])
def test_behind_the_scalar_layer_with_the_log(stats):
    from dmel_amd import MelSpectrogramLayer
    x_np = _x()
    T = L_L // HOP + 1
    g = torch.randn(B_L, 1, M_L, T, generator=torch.Generator().manual_seed(1))
    prm = N.params(M_L, 60)
    lay = MelSpectrogramLayer(torch.tensor(LAM), n_mels=M_L, n_points=L_L, sample_rate=SR, hop_length=HOP, device=DEV, optimized=True,
                              log=True).to(DEV)
    norm = _module(M_L, stats, prm)
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    frames = lay.frame_lengths(lengths)
    s_gpu = lay(torch.from_numpy(x_np).to(DEV), lengths)
    y = norm(s_gpu, frames)
    assert y.shape == (B_L, 1, M_L, T) and y.dtype == torch.float32
    (y * g.to(DEV)).sum().backward()
    out, tan = _oracle_pieces(x_np, [LAM], True)
    Tc = frames.cpu().long()
    S = torch.from_numpy(out[0]).double().requires_grad_(True)
    w64, b64 = prm[0].double(), prm[1].double()
    y_ref = N.forward(S, w64, b64, Tc, stats)
    (dS,) = torch.autograd.grad((y_ref * g.double()).sum(), [S])
    _check_dlambd(f"MelSpectrogramLayer/{stats}", lay.lambd.grad, dS, [tan[0]])
    pad = ~N.valid_mask(y.shape, Tc).expand(y.shape)
    assert bool((_bits(y.detach().cpu())[pad] == 0).all())
    # the stage itself on the layer's own output (pad frames hold log(1e-10) there and are never read)
    own = N.backward(g.double(), s_gpu.detach().cpu().double(), w64, b64, Tc, stats)
    assert N.worst(y.detach().cpu(), own["y"], own["y_scale"]) <= 1e-4
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in norm.parameters())


def test_behind_pcen_behind_the_multi_window_layer():
    import dmel_amd
    lams = [10.0, 40.0, 128.0]
    x_np = _x()
    T = L_L // HOP + 1
    g = torch.randn(B_L, 3, M_L, T, generator=torch.Generator().manual_seed(2))
    prm = N.params(M_L, 61)
    multi = dmel_amd.MultiWindowMelSpectrogram(lams, M_L, L_L, SR, hop_length=HOP, log=False, per_clip_lengths=True).to(DEV)
    pcen = dmel_amd.PCEN(M_L)
    with torch.no_grad():
        for p, v in zip((pcen.alpha, pcen.delta, pcen.r, pcen.s), P.params(M_L, 51)):
            p.copy_(v)
        pcen.alpha[0], pcen.delta[0], pcen.r[0], pcen.s[0] = 0.9, 1.0, 0.5, 0.05
    pcen = pcen.to(DEV)
    norm = _module(M_L, "batch", prm)
    lengths = torch.tensor(LENS, dtype=torch.int64, device=DEV)
    frames = multi.frame_lengths(lengths)
    y = norm(pcen(multi(torch.from_numpy(x_np).to(DEV), lengths)), frames)
    assert y.shape == (B_L, 3, M_L, T)
    (y * g.to(DEV)).sum().backward()
    out, tan = _oracle_pieces(x_np, lams, False)
    E = torch.from_numpy(np.concatenate(list(out), axis=1)).double().requires_grad_(True)          # (B, K, M, T)
    z, _ = P.forward(E, *[p.detach().cpu().double() for p in (pcen.alpha, pcen.delta, pcen.r, pcen.s)], eps=pcen.eps)
    y_ref = N.forward(z, prm[0].double(), prm[1].double(), frames.cpu().long(), "batch")
    (dE,) = torch.autograd.grad((y_ref * g.double()).sum(), [E])
    _check_dlambd("PCEN/MultiWindowMelSpectrogram", multi.lambd.grad, dE, list(tan))
    pad = ~N.valid_mask(y.shape, frames.cpu().long()).expand(y.shape)
    assert bool((_bits(y.detach().cpu())[pad] == 0).all())
    assert int(norm.num_batches_tracked) == 1


@pytest.mark.parametrize("stats", ["clip", "batch"])
def test_captured_step_replays_the_eager_bits(stats):
    """forward + backward captured into a graph (frame_lengths is read on the device only): every replay gives the eager bits, and the
    running buffers and num_batches_tracked advance once per replay"""
    idx = 9
    shape, s, g, prm, Tc = _inputs(idx, True)
    s, g, Tc = _poison(s, Tc).to(DEV), _poison(g, Tc).to(DEV), Tc.to(DEV)

    def fresh():
        return _module(shape[2], stats, prm)

    def step(m, x):
        y = m(x, Tc)
        return y, torch.autograd.grad(y, [x] + list(m.parameters()), g)

    eager_mod, x_e = fresh(), s.clone().requires_grad_(True)
    eager = []
    for _ in range(3):
        y, grads = step(eager_mod, x_e)
        torch.cuda.synchronize()
        eager.append([t.detach().clone() for t in (y, *grads)] + ([eager_mod.running_mean.clone(), eager_mod.running_var.clone()] if stats == "batch" else []))
    del y, grads
    # The captured step gets a leaf of its own, first used on the side stream, and no autograd graph outlives the warm-up: a leaf's
    # AccumulateGrad node keeps the stream it was created on for as long as a graph holds it, and one made on the default stream (the eager
    # steps above) would have the engine synchronise the default stream from inside the capture, which breaks it.
    m, x_c = fresh(), s.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(m, x_c)                                              # warm-up: the allocator (one training forward: eager[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, grads_c = step(m, x_c)
    for r in (1, 2):
        for t in (y_c, *grads_c):
            t.detach().fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        got = [y_c, *grads_c] + ([m.running_mean, m.running_var] if stats == "batch" else [])
        for a, b in zip(eager[r], got):
            assert torch.equal(_bits(a), _bits(b.detach())), r
        if stats == "batch":
            assert int(m.num_batches_tracked) == r + 1
