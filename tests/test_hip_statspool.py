"""StatsPool on the MI355X (dmel_statspool_forward / dmel_statspool_backward, dmel_amd.StatsPool, nets.MelPoolNet) against the fp64
restatement of tests/statspool_cases.py.  Every run goes through the C ABI into NaN-filled outputs between guard words.

Against fp64, every element of mean, std and ds in units of its cancellation-free scale: per case and per quantity within 8 x the worst error
of the fp32 torch restatement on the same case, capped at 1e-4 (BandNorm's rule; the worst ratios kernel / restatement are printed and quoted
in DESIGN 4.17).  Where the scale is 0 the result compares equal to 0.  The maximum, its index and everything else is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import statspool_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = 0x5EA15EA1
NAN_BITS = 0x7FC00000
IDS = [P.case_id(c) for c in P.CASES]
GIVEN = [c for c in P.CASES if c["Tc"] is not None]
GIVEN_IDS = [P.case_id(c) for c in GIVEN]
STD_BITS = int(np.float32(np.sqrt(np.float64(P.EPS))).view(np.int32))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _guarded(n, offset=0):
    """n 4-byte words of NaN bits, ``offset`` words behind a 16-byte boundary, between sentinel words: (the n words, check)"""
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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _forward(s, Tc, which, eps=P.EPS, offset=0, keep=True):
    """dmel_statspool_forward on the CPU tensor s (B, C, M, T): y (B, S C, M) fp32, stats (rows, 2) fp64 and argmax (rows,) int32 on the
    CPU, the device buffers the backward reads, the guards checked"""
    from dmel_amd import capi
    B, C, M, T = s.shape
    S, rows = len(P.selected(which)), B * C * M
    sv, lens = _placed(s, offset), _lens(Tc)
    y, y_ok = _guarded(B * S * C * M)
    st, st_ok = _guarded(4 * rows) if keep else (None, lambda: True)
    am, am_ok = _guarded(rows) if keep else (None, lambda: True)
    capi.statspool_forward(sv.data_ptr(), rows, C * M, T, _ptr(lens), which, eps, y.data_ptr(), _ptr(st), _ptr(am),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert y_ok() and st_ok() and am_ok()
    return dict(y=y.cpu().view(torch.float32).reshape(B, S * C, M), stats=None if st is None else st.cpu().view(torch.float64).reshape(rows, 2),
                am=None if am is None else am.cpu(), dev=(sv, st, am))


def _backward(g, f, shape, Tc, which, offset=0):
    """dmel_statspool_backward on the CPU tensor g (B, S C, M) and what the forward ``f`` left on the device: ds (B, C, M, T) on the CPU"""
    from dmel_amd import capi
    B, C, M, T = shape
    gv, lens = _placed(g, offset), _lens(Tc)
    sv, st, am = f["dev"]
    ds, intact = _guarded(B * C * M * T)
    capi.statspool_backward(gv.data_ptr(), sv.data_ptr() if which & 2 else None, _ptr(st) if which & 2 else None, _ptr(am) if which & 4 else None,
                            B * C * M, C * M, T, _ptr(lens), which, ds.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact()
    return ds.cpu().view(torch.float32).reshape(B, C, M, T)


def _both(s, g, Tc, which, offset=0):
    f = _forward(s, Tc, which, offset=offset)
    return dict(y=f["y"], stats=f["stats"], am=f["am"], ds=_backward(g, f, tuple(s.shape), Tc, which, offset=offset))


SAME = ("y", "stats", "am", "ds")


def _same(a, b, names=SAME, rows=None):
    """bit for bit; ``rows``: (clips, B) compares those clips only"""
    for k in names:
        x, y = a[k], b[k]
        if rows is not None:
            clips, B = rows
            x, y = x.reshape(B, -1)[clips], y.reshape(B, -1)[clips]
        xb, yb = (x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 else (_bits(x), _bits(y)) if x.dtype == torch.float32 else (x, y)
        assert torch.equal(xb, yb), k


@functools.lru_cache(maxsize=None)
def _run(index):
    """case ``index`` through the C ABI, once: from the clean inputs and from inputs with NaN payloads, -0.0, an infinity and a denormal
    planted in every pad frame of s"""
    c = P.CASES[index]
    s, g, _, _ = P.case_reference(index)
    sp = P.planted(s, c["Tc"])
    return dict(clean=_both(s, g, c["Tc"], c["which"]), planted=_both(sp, g, c["Tc"], c["which"]), sp=sp)


WORST = {}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_c_abi_against_fp64_within_eight_times_the_fp32_restatement(c):
    s, g, ref, r32 = P.case_reference(c["index"])
    r = _run(c["index"])["clean"]
    B, C, M, T = c["shape"]
    assert r["y"].shape == (B, len(P.selected(c["which"])) * C, M) and r["ds"].shape == c["shape"]
    b, w32 = P.bounds(r32, ref, c)
    got = P.errors(r["y"], r["ds"], ref, c)                        # (an element of zero scale -- every pad frame of ds -- must compare equal to 0)
    failed = []
    for k, v in got.items():
        ratio = v / w32[k] if w32[k] else (0.0 if v == 0 else float("inf"))
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        print(f"statspool {P.case_id(c)} {k}: kernel {v:.3e} fp32 restatement {w32[k]:.3e} ratio {ratio:.2f} bound {b[k]:.3e}")
        if not v <= b[k]:
            failed.append((k, v, w32[k]))
    assert not failed, (P.case_id(c), failed)
    # the unrounded pairs: y's mean and std are their roundings
    parts = P.split(r["y"], c["which"], C)
    for i, k in enumerate(("mean", "std")):
        if k in parts:
            assert torch.equal(_bits(r["stats"][:, i].to(torch.float32)), _bits(parts[k].reshape(-1))), k


def test_worst_ratios_over_the_cases():
    """(prints what the cases above measured; DESIGN 4.17 quotes it)"""
    print("statspool worst kernel / fp32 restatement ratio over all cases:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_max_argmax_pad_frames_and_planted_pad_frames_bit_for_bit(c):
    """max is s[am] as words and am is the restatement's index (the tie row and the row whose valid maximum is negative included); what the
    pad frames of s hold -- NaN payloads, -0.0, an infinity, a denormal -- changes no bit of y, stats, argmax or ds; ds is +0.0 on pad
    frames; the planted constant row gives mean == c, std == float32(sqrt(float64(eps))), argmax == 0"""
    s, g, ref, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r, rp = run["clean"], run["planted"]
    B, C, M, T = c["shape"]
    _same(rp, r)
    valid = P.valid_mask(c["shape"], c["Tc"]).expand(c["shape"])
    assert not bool(_bits(r["ds"])[~valid].any())
    if c["Tc"] is not None and any(C * M * (T - tc) >= len(P.PAD_PATTERN) for tc in c["Tc"]):      # a clip with that many pad frames holds the whole pattern
        assert set(P.PAD_PATTERN) <= {int(v) & 0xFFFFFFFF for v in _bits(run["sp"])[~valid].tolist()}
    am = r["am"].long()
    assert torch.equal(am, ref["am"].reshape(-1))
    parts = P.split(r["y"], c["which"], C)
    if "max" in parts:
        assert torch.equal(_bits(parts["max"]).reshape(-1), _bits(s).reshape(-1, T).gather(1, am[:, None])[:, 0])
    k = c["rows"]["const"]
    if "mean" in parts:
        assert _bits(parts["mean"]).reshape(-1)[k] == _bits(s).reshape(-1, T)[k, 0]
    if "std" in parts:
        assert int(_bits(parts["std"]).reshape(-1)[k]) == STD_BITS
    assert int(am[k]) == 0


@pytest.mark.parametrize("c", GIVEN[::3], ids=GIVEN_IDS[::3])
def test_constant_rows_of_full_precision_are_exact(c):
    """every row a constant of its own over its valid frames (silence under the log, -23.03, among them) with the pad pattern behind it:
    mean == c and std == float32(sqrt(float64(eps))) bit for bit, argmax == 0, and the std-only ds is 0 everywhere"""
    B, C, M, T = c["shape"]
    rows = torch.randn(B, C, M, 1, generator=torch.Generator().manual_seed(c["index"])).mul(10.0).expand(c["shape"]).clone()
    rows[0, 0, 0] = float(np.float32(np.log(1e-10)))
    s = P.planted(rows, c["Tc"])
    g = torch.randn(B, 3 * C, M, generator=torch.Generator().manual_seed(c["index"] + 1))
    f = _forward(s, c["Tc"], 7)
    parts = P.split(f["y"], 7, C)
    assert torch.equal(_bits(parts["mean"]), _bits(rows[..., 0]))
    assert bool((_bits(parts["std"]) == STD_BITS).all()) and torch.equal(_bits(parts["max"]), _bits(rows[..., 0]))
    assert not bool(f["am"].any())
    assert torch.equal(f["stats"][:, 0], rows[..., 0].reshape(-1).double()) and bool((_bits(f["stats"][:, 1].float()) == STD_BITS).all())
    ds = _backward(g[:, C:2 * C].contiguous(), _forward(s, c["Tc"], 2), c["shape"], c["Tc"], 2)
    assert bool((ds == 0).all())


@pytest.mark.parametrize("c", [c for c in P.CASES if c["Tc"] is None], ids=[i for c, i in zip(P.CASES, IDS) if c["Tc"] is None])
def test_full_lengths_give_the_bits_of_none(c):
    s, g, _, _ = P.case_reference(c["index"])
    full = [c["shape"][3]] * c["shape"][0]
    _same(_both(s, g, full, c["which"]), _run(c["index"])["clean"])


@pytest.mark.parametrize("c", [c for c in GIVEN if c["shape"][0] > 1], ids=[P.case_id(c) for c in GIVEN if c["shape"][0] > 1])
def test_a_clip_alone_gives_the_bits_it_has_inside_the_batch(c):
    s, g, _, _ = P.case_reference(c["index"])
    r = _run(c["index"])["clean"]
    B = c["shape"][0]
    for b in sorted({0, B - 1, B // 2}):
        alone = _both(s[b:b + 1], g[b:b + 1], c["Tc"][b:b + 1], c["which"])
        for k in SAME:
            x, y = alone[k].reshape(1, -1), r[k].reshape(B, -1)[b:b + 1]
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else _bits(x), y.view(torch.int64) if y.dtype == torch.float64 else _bits(y)), (b, k)


@pytest.mark.parametrize("c", P.CASES[::5], ids=IDS[::5])
def test_two_runs_give_the_same_bits(c):
    _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    _same(_both(run["sp"], g, c["Tc"], c["which"]), run["planted"])


@pytest.mark.parametrize("c", [c for c in GIVEN if c["which"] == 7][::2], ids=[P.case_id(c) for c in GIVEN if c["which"] == 7][::2])
def test_a_single_statistic_equals_its_group_of_all_three(c):
    """every other selection's y is the matching groups of which = 7, and its stats and argmax are the same words; without the buffers the
    backward reads (what the module passes under no_grad) y keeps its bits"""
    r = _run(c["index"])
    C = c["shape"][1]
    all3 = P.split(r["planted"]["y"], 7, C)
    for which in (1, 2, 3, 4, 5, 6):
        f = _forward(r["sp"], c["Tc"], which)
        for k, v in P.split(f["y"], which, C).items():
            assert torch.equal(_bits(v), _bits(all3[k])), (which, k)
        assert torch.equal(f["am"], r["planted"]["am"]) and torch.equal(f["stats"].view(torch.int64), r["planted"]["stats"].view(torch.int64)), which
    assert torch.equal(_bits(_forward(r["sp"], c["Tc"], 7, keep=False)["y"]), _bits(r["planted"]["y"]))


INVALID = [i for i, c in enumerate(P.CASES) if c["shape"] in ((3, 1, 5, 2), (4, 1, 4, 32), (2, 1, 3, 65), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5))
           and c["which"] == 7 and c["Tc"] is not None]


@pytest.mark.parametrize("bad_length", ["zero", "T_plus_one"])
@pytest.mark.parametrize("idx", INVALID, ids=lambda i: IDS[i])
def test_an_invalid_length_poisons_its_own_clip_only(idx, bad_length):
    c = P.CASES[idx]
    s, g, _, _ = P.case_reference(idx)
    r = _run(idx)["clean"]
    B, T = c["shape"][0], c["shape"][3]
    for which in (0, B - 1):
        Tc = P.lengths_of(c)
        Tc[which] = 0 if bad_length == "zero" else T + 1
        got = _both(s, g, Tc, 7)
        assert bool((_bits(got["y"][which]) == NAN_BITS).all()) and bool((_bits(got["ds"][which]) == NAN_BITS).all())
        assert bool((got["am"].reshape(B, -1)[which] == -1).all()) and bool(torch.isnan(got["stats"].reshape(B, -1)[which]).all())
        _same(got, r, rows=([b for b in range(B) if b != which], B))


ODD = [i for i, c in enumerate(P.CASES) if c["shape"] in ((3, 1, 5, 2), (2, 1, 3, 33), (2, 1, 3, 65), (2, 3, 5, 40)) and c["which"] == 7 and c["Tc"] is not None]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("idx", ODD, ids=lambda i: IDS[i])
def test_inputs_at_odd_element_offsets_give_the_aligned_bits(idx, k):
    """s and g start 4 + k elements behind a 16-byte boundary"""
    c = P.CASES[idx]
    _, g, _, _ = P.case_reference(idx)
    run = _run(idx)
    _same(_both(run["sp"], g, c["Tc"], 7, offset=4 + k), run["planted"])


# ---- the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CASES[::2], ids=IDS[::2])
def test_module_gives_the_c_abi_bits(c):
    """dmel_amd.StatsPool with int64 frame_lengths (narrowed on the device): y and the gradient torch.autograd reaches are the C ABI's; a
    (B, n_mels, T) view where there is one channel, int32 lengths and a non-contiguous input give the same bits"""
    import dmel_amd
    _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r = run["planted"]
    B, C, M, T = c["shape"]
    m = dmel_amd.StatsPool(P.selected(c["which"])[::-1], eps=P.EPS)
    Tc = None if c["Tc"] is None else torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    x = run["sp"].to(DEV).requires_grad_(True)
    y = m(x, Tc)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert y.shape == r["y"].shape and y.dtype == torch.float32 and x.grad.shape == x.shape
    assert torch.equal(_bits(y).cpu(), _bits(r["y"])) and torch.equal(_bits(x.grad).cpu(), _bits(r["ds"]))
    if C == 1:
        y3 = m.eval()(run["sp"].to(DEV).reshape(B, M, T), None if Tc is None else Tc.to(torch.int32))
        assert y3.shape == y.shape and torch.equal(_bits(y3).cpu(), _bits(r["y"]))
    wide = torch.zeros((B, C, M, T + 3), device=DEV)
    wide[..., :T] = run["sp"].to(DEV)
    assert torch.equal(_bits(m(wide[..., :T], Tc)).cpu(), _bits(r["y"]))


def test_module_saves_only_what_the_selected_statistics_need(monkeypatch):
    """what reaches dmel_statspool_forward: the fp64 pairs with std, the argmax with max, neither under no_grad or for an input that needs
    no gradient"""
    import dmel_amd
    from dmel_amd import capi
    seen = []
    real = capi.statspool_forward

    def spy(*a):
        seen.append((a[8] is not None, a[9] is not None))
        return real(*a)

    monkeypatch.setattr(capi, "statspool_forward", spy)
    s = torch.rand(2, 1, 3, 9, device=DEV)
    for stats, want in ((("mean",), (False, False)), (("std",), (True, False)), (("max", "mean"), (False, True)), (("mean", "std", "max"), (True, True))):
        m = dmel_amd.StatsPool(stats)
        x = s.clone().requires_grad_(True)
        y = m(x)
        saved = [t for t in y.grad_fn.saved_tensors if t is not None]
        assert seen[-1] == want and len(saved) == sum(want) + int(want[0]), stats           # (s itself is kept with std only)
        y.sum().backward()
        with torch.no_grad():
            z = m(x)
        assert seen[-1] == (False, False) and z.grad_fn is None and torch.equal(_bits(z), _bits(y))
        m(s)
        assert seen[-1] == (False, False)


def test_module_with_an_int64_length_beyond_32_bits_gives_a_nan_clip():
    import dmel_amd
    s = torch.rand(2, 1, 3, 9, device=DEV).requires_grad_(True)
    y = dmel_amd.StatsPool()(s, torch.tensor([(1 << 32) + 5, 9], dtype=torch.int64, device=DEV))
    y.sum().backward()
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isfinite(y[1]).all())
    assert bool(torch.isnan(s.grad[0]).all()) and bool(torch.isfinite(s.grad[1]).all())
    with pytest.raises(RuntimeError, match="frame_lengths is on cpu"):
        dmel_amd.StatsPool()(s, torch.tensor([9, 9]))
    with pytest.raises(RuntimeError, match="bfloat16"):
        dmel_amd.StatsPool()(s.detach().to(torch.bfloat16))


def test_captured_step_replays_the_eager_bits():
    """forward + backward captured into a graph (frame_lengths is read on the device only): three replays give the eager bits"""
    import dmel_amd
    c = next(c for c in P.CASES if c["shape"] == (2, 3, 5, 40) and c["which"] == 7 and c["Tc"] is not None)
    _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r = run["planted"]
    s, g, Tc = run["sp"].to(DEV), g.to(DEV), torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    m = dmel_amd.StatsPool()

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
    for _ in range(3):
        y_c.detach().fill_(float("nan")), ds_c.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y_c).cpu(), _bits(r["y"])) and torch.equal(_bits(ds_c).cpu(), _bits(r["ds"]))


# ---- behind the layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front", ["layer", "bandnorm_clip"])
def test_behind_the_layers_lambd_grad_follows_the_oracles_chain(front):
    """pool([norm](layer(x, lengths)[, fl]), fl) with the log, n_fft 1024, 81 frames, lengths 4000 / 1234 / 50 (81 / 25 / 2 frames):
    lambd.grad against the oracle's chain -- clip by clip at the clip's own length, then the fp64 adjoint of the restatement -- within 1e-4
    of sum |dS64 tangent64|, the project's bar (the measured distance is printed)"""
    import dmel_amd
    import bandnorm_cases as N
    from test_hip_bandnorm import B_L, HOP, LAM, LENS, L_L, M_L, SR, _check_dlambd, _oracle_pieces, _x
    x_np = _x()
    T = L_L // HOP + 1
    g = torch.randn(B_L, 3, M_L, generator=torch.Generator().manual_seed(4))
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
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
    y = dmel_amd.StatsPool(eps=P.EPS)(z, fl)
    assert y.shape == (B_L, 3, M_L) and y.dtype == torch.float32
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out, tan = _oracle_pieces(x_np, [LAM], True)
    S = torch.from_numpy(out[0]).double().requires_grad_(True)                                      # (B, 1, M, T)
    z_ref = N.forward(S, prm[0].double(), prm[1].double(), Tc, "clip") if front == "bandnorm_clip" else S
    y_ref, _ = P.forward(z_ref, Tc.tolist(), 7)
    (dS,) = torch.autograd.grad((y_ref * g.double()).sum(), [S])
    _check_dlambd(f"StatsPool/{front}", lay.lambd.grad, dS, [tan[0]])
    # the stage itself on what stands in front of it (pad frames hold log(1e-10), or BandNorm's +0.0, and are never read)
    zc = z.detach().cpu()
    own = P.reference(zc, g, Tc.tolist(), 7)
    c = dict(shape=tuple(zc.shape), which=7)
    assert all(v <= 1e-4 for v in P.errors(y.detach().cpu(), None, own, c).values())
    assert torch.equal(_bits(P.split(y.detach().cpu(), 7, 1)["max"]), _bits(P.split(own["y"].float(), 7, 1)["max"]))


# ---- nets.MelPoolNet ----------------------------------------------------------------------------------------------------------------------
N_POINTS, HOP_N, MELS, CLIP = 4000, 64, 40, 1234


def _net(seed=0, **kw):
    from dmel_amd import nets
    torch.manual_seed(seed)
    return nets.MelPoolNet(5, 128.0, DEV, MELS, 16000, N_POINTS, hop_length=HOP_N, **kw).to(DEV)


def _batch(lengths, where, clip):
    """a zero-padded batch with ``clip`` at row ``where``; the other rows are clips of their own"""
    from dmel_amd import synth
    x = torch.from_numpy(synth.waveforms(len(lengths), N_POINTS, seed=11)).clone()
    x[where] = clip
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
    return x.to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)


def test_mel_pool_net_logits_do_not_depend_on_the_batch():
    from dmel_amd import synth
    net = _net().eval()
    clip = torch.zeros(N_POINTS)
    clip[:CLIP] = torch.from_numpy(synth.waveforms(1, N_POINTS, seed=5))[0, :CLIP]
    with torch.no_grad():
        alone, s = net(*_batch([CLIP], 0, clip))
        assert alone.shape == (1, 5) and s.shape == (1, 1, MELS, N_POINTS // HOP_N + 1) and bool(torch.isfinite(alone).all())
        for lengths, where in (([CLIP, N_POINTS, 50], 0), ([N_POINTS, 50, CLIP], 2), ([777, CLIP, 3000], 1), ([1, CLIP, N_POINTS - 1], 1)):
            logits, _ = net(*_batch(lengths, where, clip))
            assert torch.equal(_bits(logits[where]), _bits(alone[0])), (lengths, where)
        x, _ = _batch([N_POINTS, N_POINTS], 0, torch.from_numpy(synth.waveforms(1, N_POINTS, seed=6))[0])
        full, s_full = net(x, torch.tensor([N_POINTS, N_POINTS], dtype=torch.int32, device=DEV))
        none, s_none = net(x)
        assert torch.equal(_bits(none), _bits(full)) and torch.equal(_bits(s_none), _bits(s_full))


def test_mel_pool_net_trains_with_and_without_the_opt_in_stages():
    import dmel_amd
    from dmel_amd import nets, synth
    clip = torch.from_numpy(synth.waveforms(1, N_POINTS, seed=5))[0]
    x, lengths = _batch([CLIP, N_POINTS, 50], 0, clip)
    labels = torch.tensor([0, 3, 1], device=DEV)
    for staged in (False, True):
        net = _net(seed=1)
        if staged:
            net.normalization = dmel_amd.BandNorm(MELS, stats="clip").to(DEV)
            net.augmentation = dmel_amd.SpecMask(8, 4, seed=3).to(DEV)
        opt = nets.make_optimizer(net, 1e-2, 1.0)
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        logits, _ = net.train()(x, lengths)
        torch.nn.functional.cross_entropy(logits, labels).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        opt.step()
        torch.cuda.synchronize()
        for name in ("spectrogram_layer.lambd", "fc.weight"):
            assert not torch.equal(dict(net.named_parameters())[name].detach(), before[name]), (staged, name)
        if staged:                                                 # eval() ignores the augmentation: what the net returns is the normalised image
            with torch.no_grad():
                _, s_eval = net.eval()(x, lengths)
                fl = net.spectrogram_layer.frame_lengths(lengths)
                want = net.normalization(net.spectrogram_layer(x, lengths), fl)
                a, _ = net(x, lengths)
                b, _ = net(x, lengths)
            assert torch.equal(_bits(s_eval), _bits(want)) and torch.equal(_bits(a), _bits(b))
