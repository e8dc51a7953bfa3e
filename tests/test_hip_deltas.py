"""Deltas on the MI355X (dmel_deltas_forward / dmel_deltas_backward, dmel_amd.Deltas) against the fp64 restatement of tests/deltas_cases.py.
Every run goes through the C ABI into NaN-filled outputs between guards.

Against fp64, every element, in units of its cancellation-free scale, with u = 2^-24 and m = 2 n + n (n + 1) / 2:
    d  <= (3 n + 1) u       dd <= 2 (3 n + 1) u       ds <= (2 m + 6) u
(the rounding count of the specified fp32 arithmetic; the kernel takes its differences and sums in fp64 and rounds d, dd, h and ds once each,
so it sits well inside: the worst ratios are printed by the tests and quoted in DESIGN 4.16).  Where the scale is 0 the result is an exact
zero.  Everything else is bit for bit, without a tolerance."""
import functools

import numpy as np
import pytest
import torch

import deltas_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = 0x5EA15EA1
NAN_BITS = 0x7FC00000
IDS = [D.case_id(c) for c in D.CASES]
GIVEN = [c for c in D.CASES if c["Tc"] is not None]
GIVEN_IDS = [D.case_id(c) for c in GIVEN]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _guarded(n, offset=0):
    """n fp32 elements of NaN bits, ``offset`` elements behind a 16-byte boundary, between sentinel words: (the n elements, check)"""
    buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=torch.int32, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.fill_(NAN_BITS)

    def intact():
        return bool((buf[:GUARD + offset] == SENTINEL).all()) and bool((buf[GUARD + offset + n:] == SENTINEL).all())

    return view, intact


def _placed(t, offset=0):
    """the device copy of the fp32 tensor t starting ``offset`` elements behind a 16-byte boundary, sentinel words on both sides"""
    view, _ = _guarded(t.numel(), offset)
    view.copy_(_bits(t).reshape(-1).to(DEV))
    return view


def _lens(Tc):
    return None if Tc is None else torch.tensor(list(Tc), dtype=torch.int32, device=DEV)


def _forward(s, Tc, win, order, static, offset=0):
    """dmel_deltas_forward on the CPU tensor s (B, C, M, T): y (B, G C, M, T) as a CPU fp32 tensor, the guards checked"""
    from dmel_amd import capi
    B, C, M, T = s.shape
    G = int(static) + order
    sv, lens = _placed(s, offset), _lens(Tc)
    y, intact = _guarded(B * G * C * M * T)
    capi.deltas_forward(sv.data_ptr(), B * C * M, C * M, T, None if lens is None else lens.data_ptr(), win, order, static, y.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact()
    return y.cpu().view(torch.float32).reshape(B, G * C, M, T)


def _backward(g, Tc, win, order, static, offset=0):
    """dmel_deltas_backward on the CPU tensor g (B, G C, M, T): ds (B, C, M, T) as a CPU fp32 tensor, the guards checked"""
    from dmel_amd import capi
    G = int(static) + order
    B, GC, M, T = g.shape
    C = GC // G
    gv, lens = _placed(g, offset), _lens(Tc)
    ds, intact = _guarded(B * C * M * T)
    capi.deltas_backward(gv.data_ptr(), B * C * M, C * M, T, None if lens is None else lens.data_ptr(), win, order, static, ds.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact()
    return ds.cpu().view(torch.float32).reshape(B, C, M, T)


def _args(c):
    return c["win_length"], c["order"], c["include_static"]


def _planted_g(c, g):
    """g with the pad pattern in every group's pad frames"""
    return D.planted(g, c["Tc"], pattern=D.PAD_PATTERN[::-1])


@functools.lru_cache(maxsize=None)
def _run(index):
    """case ``index`` through the C ABI, once: from the clean inputs and from inputs with NaN payloads, -0.0, an infinity and a denormal
    planted in every pad frame"""
    c = D.CASES[index]
    s, g, _ = D.case_reference(index)
    sp, gp = D.planted(s, c["Tc"]), _planted_g(c, g)
    return dict(y=_forward(s, c["Tc"], *_args(c)), ds=_backward(g, c["Tc"], *_args(c)), sp=sp, gp=gp,
                yp=_forward(sp, c["Tc"], *_args(c)), dsp=_backward(gp, c["Tc"], *_args(c)))


WORST = {}


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_c_abi_against_fp64_within_the_rounding_count(c):
    s, g, ref = D.case_reference(c["index"])
    r = _run(c["index"])
    b = D.bounds(c["win_length"])
    B, C, M, T = c["shape"]
    assert r["y"].shape == (B, D.groups(c) * C, M, T) and r["ds"].shape == c["shape"]
    _, d64, dd64 = D.split(ref["y"], c)
    _, dsc, ddsc = D.split(ref["y_scale"], c)
    _, d, dd = D.split(r["y"], c)
    ratios = dict(d=D.worst(d, d64, dsc) / D.U, ds=D.worst(r["ds"], ref["ds"], ref["ds_scale"]) / D.U)
    if c["order"] == 2:
        ratios["dd"] = D.worst(dd, dd64, ddsc) / D.U
    print(D.case_id(c), "worst error / scale in units of u:", {k: round(v, 3) for k, v in ratios.items()}, "bounds:", {k: round(v / D.U) for k, v in b.items()})
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v * D.U <= b[k], (k, v, b[k] / D.U)


def test_worst_ratios_over_the_cases():
    """(prints what the cases above measured; DESIGN 4.16 quotes it)"""
    print("worst error / scale in units of u = 2^-24 over all cases:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_static_group_pad_frames_and_planted_pad_frames_bit_for_bit(c):
    """the static group is s on every frame (NaN payloads, -0.0, an infinity, a denormal in the pad frames); the delta groups are +0.0 on
    pad frames; what the pad frames of s, g_d and g_dd hold changes no valid delta and no ds; ds on pad frames is g_static's bits, or +0.0
    without the static group; Tc = 1 gives +0.0"""
    r = _run(c["index"])
    s, g, _ = D.case_reference(c["index"])
    B, C, M, T = c["shape"]
    valid = D.valid_mask(c["shape"], c["Tc"]).expand(c["shape"])
    for y, src in ((r["y"], s), (r["yp"], r["sp"])):
        st, d, dd = D.split(y, c)
        if st is not None:
            assert torch.equal(_bits(st), _bits(src))
        for grp in (d, dd):
            if grp is not None:
                assert not bool(_bits(grp)[~valid].any())
    assert torch.equal(_bits(r["yp"][:, int(c["include_static"]) * C:]), _bits(r["y"][:, int(c["include_static"]) * C:]))
    assert torch.equal(_bits(r["dsp"])[valid], _bits(r["ds"])[valid])
    for ds, src in ((r["ds"], g), (r["dsp"], r["gp"])):
        if c["include_static"]:
            assert torch.equal(_bits(ds)[~valid], _bits(src[:, :C])[~valid])
        else:
            assert not bool(_bits(ds)[~valid].any())
    if c["Tc"] is not None and any(C * M * (T - tc) >= len(D.PAD_PATTERN) for tc in c["Tc"]):      # a clip with that many pad frames holds the whole pattern
        assert set(D.PAD_PATTERN) <= {int(v) & 0xFFFFFFFF for v in _bits(r["sp"])[~valid].tolist()}
    for bi, tc in enumerate(D.lengths_of(c)):
        if tc == 1:
            assert not bool(_bits(r["y"][bi, int(c["include_static"]) * C:]).any())


@pytest.mark.parametrize("c", GIVEN[::3], ids=GIVEN_IDS[::3])
def test_constant_rows_give_exact_zeros(c):
    """rows that are constant over their valid frames (silence under the log, -23.03; another constant per row) with NaN behind them"""
    B, C, M, T = c["shape"]
    rows = torch.randn(B, C, M, 1, generator=torch.Generator().manual_seed(c["index"])).expand(c["shape"]).clone()
    rows[0, 0, 0] = float(np.float32(np.log(1e-10)))
    s = D.planted(rows, c["Tc"])
    y = _forward(s, c["Tc"], *_args(c))
    assert not bool(_bits(y[:, int(c["include_static"]) * C:]).any())


@pytest.mark.parametrize("c", [c for c in D.CASES if c["Tc"] is None], ids=[i for c, i in zip(D.CASES, IDS) if c["Tc"] is None])
def test_full_lengths_give_the_bits_of_none(c):
    s, g, _ = D.case_reference(c["index"])
    r = _run(c["index"])
    full = [c["shape"][3]] * c["shape"][0]
    assert torch.equal(_bits(_forward(s, full, *_args(c))), _bits(r["y"]))
    assert torch.equal(_bits(_backward(g, full, *_args(c))), _bits(r["ds"]))


@pytest.mark.parametrize("c", [c for c in GIVEN if c["shape"][0] > 1], ids=[D.case_id(c) for c in GIVEN if c["shape"][0] > 1])
def test_a_clip_alone_gives_the_bits_it_has_inside_the_batch(c):
    s, g, _ = D.case_reference(c["index"])
    r = _run(c["index"])
    for b in {0, c["shape"][0] - 1, c["shape"][0] // 2}:
        assert torch.equal(_bits(_forward(s[b:b + 1], c["Tc"][b:b + 1], *_args(c))), _bits(r["y"][b:b + 1])), b
        assert torch.equal(_bits(_backward(g[b:b + 1], c["Tc"][b:b + 1], *_args(c))), _bits(r["ds"][b:b + 1])), b


@pytest.mark.parametrize("c", [c for c in D.CASES if c["order"] == 2], ids=[i for c, i in zip(D.CASES, IDS) if c["order"] == 2])
def test_dd_is_the_kernel_applied_to_its_own_stored_d(c):
    """the dd group of order 2 equals the d group of order 1 run on the stored d group with the same lengths"""
    r = _run(c["index"])
    _, d, dd = D.split(r["y"], c)
    again = _forward(d.contiguous(), c["Tc"], c["win_length"], 1, False)
    assert torch.equal(_bits(again), _bits(dd))


@pytest.mark.parametrize("c", D.CASES[::5], ids=IDS[::5])
def test_two_runs_give_the_same_bits(c):
    r = _run(c["index"])
    assert torch.equal(_bits(_forward(r["sp"], c["Tc"], *_args(c))), _bits(r["yp"]))
    assert torch.equal(_bits(_backward(r["gp"], c["Tc"], *_args(c))), _bits(r["dsp"]))


INVALID = [i for i, c in enumerate(D.CASES) if c["shape"] in ((3, 1, 5, 2), (4, 1, 4, 32), (2, 1, 3, 65), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5))
           and c["win_length"] == 5]


@pytest.mark.parametrize("bad_length", ["zero", "T_plus_one"])
@pytest.mark.parametrize("idx", INVALID, ids=lambda i: IDS[i])
def test_an_invalid_length_poisons_its_own_clip_only(idx, bad_length):
    c = D.CASES[idx]
    s, g, _ = D.case_reference(idx)
    r = _run(idx)
    B, T = c["shape"][0], c["shape"][3]
    for which in (0, B - 1):
        Tc = D.lengths_of(c)
        Tc[which] = 0 if bad_length == "zero" else T + 1
        y, ds = _forward(s, Tc, *_args(c)), _backward(g, Tc, *_args(c))
        assert bool((_bits(y[which]) == NAN_BITS).all()) and bool((_bits(ds[which]) == NAN_BITS).all())
        others = [b for b in range(B) if b != which]
        assert torch.equal(_bits(y[others]), _bits(r["y"][others])) and torch.equal(_bits(ds[others]), _bits(r["ds"][others]))


ODD = [i for i, c in enumerate(D.CASES) if c["shape"] in ((3, 1, 5, 2), (2, 1, 3, 33), (2, 1, 3, 65), (2, 3, 5, 40)) and c["win_length"] == 5 and c["Tc"] is not None]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("idx", ODD, ids=lambda i: IDS[i])
def test_inputs_at_odd_element_offsets_give_the_aligned_bits(idx, k):
    """s and g start 4 + k elements behind a 16-byte boundary; y and ds are 16-byte aligned as the contract asks"""
    c = D.CASES[idx]
    r = _run(idx)
    assert torch.equal(_bits(_forward(r["sp"], c["Tc"], *_args(c), offset=4 + k)), _bits(r["yp"]))
    assert torch.equal(_bits(_backward(r["gp"], c["Tc"], *_args(c), offset=4 + k)), _bits(r["dsp"]))


def test_misaligned_outputs_are_refused():
    from dmel_amd import capi
    sv = _placed(torch.rand(9, 5))
    for fn, word in ((capi.deltas_forward, "y must be a 16-byte aligned"), (capi.deltas_backward, "ds must be a 16-byte aligned")):
        out, intact = _guarded(3 * 9 * 5, 1)
        with pytest.raises(capi.DmelError, match=word):
            fn(sv.data_ptr(), 9, 3, 5, None, 5, 1, False, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert intact() and bool((out == NAN_BITS).all())


# ---- the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.CASES[::2], ids=IDS[::2])
def test_module_gives_the_c_abi_bits(c):
    """dmel_amd.Deltas with int64 frame_lengths (narrowed on the device): y and the gradient torch.autograd reaches are the C ABI's; a
    (B, n_mels, T) view where there is one channel, int32 lengths and a non-contiguous input give the same bits"""
    import dmel_amd
    r = _run(c["index"])
    B, C, M, T = c["shape"]
    m = dmel_amd.Deltas(*_args(c))
    Tc = None if c["Tc"] is None else torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    x = r["sp"].to(DEV).requires_grad_(True)
    y = m(x, Tc)
    y.backward(r["gp"].to(DEV))
    torch.cuda.synchronize()
    assert y.shape == (B, D.groups(c) * C, M, T) and y.dtype == torch.float32 and x.grad.shape == x.shape
    assert torch.equal(_bits(y).cpu(), _bits(r["yp"])) and torch.equal(_bits(x.grad).cpu(), _bits(r["dsp"]))
    if C == 1:
        y3 = m.eval()(r["sp"].to(DEV).reshape(B, M, T), None if Tc is None else Tc.to(torch.int32))
        assert y3.shape == y.shape and torch.equal(_bits(y3).cpu(), _bits(r["yp"]))
    wide = torch.zeros((B, C, M, T + 3), device=DEV)
    wide[..., :T] = r["sp"].to(DEV)
    assert torch.equal(_bits(m(wide[..., :T], Tc)).cpu(), _bits(r["yp"]))


def test_module_with_an_int64_length_beyond_32_bits_gives_a_nan_clip():
    import dmel_amd
    s = torch.rand(2, 1, 3, 9, device=DEV)
    y = dmel_amd.Deltas()(s, torch.tensor([(1 << 32) + 5, 9], dtype=torch.int64, device=DEV))
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isfinite(y[1]).all())
    with pytest.raises(RuntimeError, match="frame_lengths is on cpu"):
        dmel_amd.Deltas()(s, torch.tensor([9, 9]))
    with pytest.raises(RuntimeError, match="bfloat16"):
        dmel_amd.Deltas()(s.to(torch.bfloat16))


def test_captured_step_replays_the_eager_bits():
    """forward + backward captured into a graph (frame_lengths is read on the device only): every replay gives the eager bits"""
    import dmel_amd
    c = next(c for c in D.CASES if c["shape"] == (2, 3, 5, 40) and c["win_length"] == 5 and c["Tc"] is not None and c["order"] == 2)
    r = _run(c["index"])
    s, g, Tc = r["sp"].to(DEV), r["gp"].to(DEV), torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    m = dmel_amd.Deltas(*_args(c))

    def step(x):
        y = m(x, Tc)
        return y, torch.autograd.grad(y, [x], g)[0]

    # (a leaf of its own, first used on the side stream, and no autograd graph outliving the warm-up: see tests/test_hip_bandnorm.py)
    x_c = s.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x_c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, ds_c = step(x_c)
    for _ in range(2):
        y_c.detach().fill_(float("nan")), ds_c.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y_c).cpu(), _bits(r["yp"])) and torch.equal(_bits(ds_c).cpu(), _bits(r["dsp"]))


# ---- behind the layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front", ["layer", "bandnorm_clip", "multi_window"])
def test_behind_the_layers_lambd_grad_follows_the_oracles_chain(front):
    """deltas([norm](layer(x, lengths)[, fl]), fl) with the log, n_fft 1024, 81 frames, lengths 4000 / 1234 / 50 (81 / 25 / 2 frames):
    lambd.grad against the oracle's chain -- clip by clip at the clip's own length, then the fp64 adjoint of the restatement -- within 1e-4
    of sum |dS64 tangent64|, the project's bar; behind the multi-window layer C = 3 goes in and 9 channels come out"""
    import dmel_amd
    import bandnorm_cases as N
    from test_hip_bandnorm import B_L, HOP, LAM, LENS, L_L, M_L, SR, _check_dlambd, _oracle_pieces, _x
    x_np = _x()
    T = L_L // HOP + 1
    lams = [10.0, 40.0, 128.0] if front == "multi_window" else [LAM]
    K = len(lams)
    g = torch.randn(B_L, 3 * K, M_L, T, generator=torch.Generator().manual_seed(4))
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    if front == "multi_window":
        lay = dmel_amd.MultiWindowMelSpectrogram(lams, M_L, L_L, SR, hop_length=HOP, log=True, per_clip_lengths=True).to(DEV)
    else:
        lay = dmel_amd.MelSpectrogramLayer(torch.tensor(LAM), n_mels=M_L, n_points=L_L, sample_rate=SR, hop_length=HOP, device=DEV, optimized=True,
                                           log=True).to(DEV)
    fl = lay.frame_lengths(lengths)
    Tc = fl.cpu().long()
    assert Tc.tolist() == [81, 25, 2]
    z = lay(torch.from_numpy(x_np).to(DEV), lengths)
    prm = N.params(M_L, 60)
    if front == "bandnorm_clip":
        norm = dmel_amd.BandNorm(M_L, stats="clip", eps=N.EPS, momentum=N.MOMENTUM)
        with torch.no_grad():
            norm.weight.copy_(prm[0]), norm.bias.copy_(prm[1])
        z = norm.to(DEV)(z, fl)
    y = dmel_amd.Deltas(5, 2, True)(z, fl)
    assert y.shape == (B_L, 3 * K, M_L, T) and y.dtype == torch.float32
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out, tan = _oracle_pieces(x_np, lams, True)
    S = torch.from_numpy(np.concatenate(list(out), axis=1)).double().requires_grad_(True)          # (B, K, M, T)
    z_ref = N.forward(S, prm[0].double(), prm[1].double(), Tc, "clip") if front == "bandnorm_clip" else S
    y_ref = D.forward(z_ref, Tc.tolist(), 5, 2, True)
    (dS,) = torch.autograd.grad((y_ref * g.double()).sum(), [S])
    _check_dlambd(f"Deltas/{front}", lay.lambd.grad, dS, list(tan))
    pad = ~D.valid_mask((B_L, K, M_L, T), Tc.tolist()).expand(B_L, 2 * K, M_L, T)
    assert not bool(_bits(y[:, K:]).cpu()[pad].any())
    # the stage itself on what stands in front of it (pad frames hold log(1e-10), or BandNorm's +0.0, and are never read for the deltas)
    own = D.reference(z.detach().cpu(), g, Tc.tolist(), 5, 2, True)
    b = D.bounds(5)
    assert D.worst(y[:, K:2 * K].detach().cpu(), own["y"][:, K:2 * K], own["y_scale"][:, K:2 * K]) <= b["d"]
    assert D.worst(y[:, 2 * K:].detach().cpu(), own["y"][:, 2 * K:], own["y_scale"][:, 2 * K:]) <= b["dd"]
    assert torch.equal(_bits(y[:, :K]), _bits(z))
