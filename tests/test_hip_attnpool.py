"""AttentivePool on the MI355X (dmel_attnpool_forward / dmel_attnpool_backward, dmel_amd.AttentivePool, nets.MelAttnPoolNet) against the
fp64 restatement of tests/attnpool_cases.py.  Every run goes through the C ABI into NaN-filled outputs between guard words.

Against fp64, every element of mean, std, ds and da in units of its cancellation-free scale: per case and per quantity within 8 x the worst
error of the fp32 torch restatement on the same case, capped at 1e-4 (BandNorm's and StatsPool's rule; the worst ratios kernel / restatement
are printed and quoted in DESIGN 4.18).  Where the scale is 0 the result compares equal to 0.  Everything else is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import attnpool_cases as P

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


def _words(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else _bits(t)


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


def _forward(s, a, Tc, which, eps=P.EPS, offset=0, keep=True):
    """dmel_attnpool_forward on the CPU tensors s (B, C, M, T) and a (B, A, T): y (B, S C, M) fp32, stats (rows, 2) and norm (B A, 2) fp64
    on the CPU, the device buffers the backward reads, the guards checked"""
    from dmel_amd import capi
    B, C, M, T = s.shape
    A = a.shape[1]
    S, rows = len(P.selected(which)), B * C * M
    sv, av, lens = _placed(s, offset), _placed(a, offset), _lens(Tc)
    y, y_ok = _guarded(B * S * C * M)
    st, st_ok = _guarded(4 * rows) if keep else (None, lambda: True)
    nm, nm_ok = _guarded(4 * B * A) if keep else (None, lambda: True)
    capi.attnpool_forward(sv.data_ptr(), av.data_ptr(), rows, C * M, A, T, _ptr(lens), which, eps, y.data_ptr(), _ptr(st), _ptr(nm),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert y_ok() and st_ok() and nm_ok()
    return dict(y=y.cpu().view(torch.float32).reshape(B, S * C, M), stats=None if st is None else st.cpu().view(torch.float64).reshape(rows, 2),
                norm=None if nm is None else nm.cpu().view(torch.float64).reshape(B * A, 2), dev=(sv, av, st, nm), A=A)


def _backward(g, f, shape, Tc, which, eps=P.EPS, offset=0):
    """dmel_attnpool_backward on the CPU tensor g (B, S C, M) and what the forward ``f`` left on the device: ds (B, C, M, T), da (B, A, T)"""
    from dmel_amd import capi
    B, C, M, T = shape
    gv, lens = _placed(g, offset), _lens(Tc)
    sv, av, st, nm = f["dev"]
    ds, ds_ok = _guarded(B * C * M * T)
    da, da_ok = _guarded(B * f["A"] * T)
    capi.attnpool_backward(gv.data_ptr(), sv.data_ptr(), av.data_ptr(), st.data_ptr(), nm.data_ptr(), B * C * M, C * M, f["A"], T, _ptr(lens), which,
                           eps, ds.data_ptr(), da.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ds_ok() and da_ok()
    return ds.cpu().view(torch.float32).reshape(B, C, M, T), da.cpu().view(torch.float32).reshape(B, f["A"], T)


def _both(s, a, g, Tc, which, offset=0):
    f = _forward(s, a, Tc, which, offset=offset)
    ds, da = _backward(g, f, tuple(s.shape), Tc, which, offset=offset)
    return dict(y=f["y"], stats=f["stats"], norm=f["norm"], ds=ds, da=da)


SAME = ("y", "stats", "norm", "ds", "da")


def _same(a, b, names=SAME, rows=None):
    """bit for bit; ``rows``: (clips, B) compares those clips only"""
    for k in names:
        x, y = a[k], b[k]
        if rows is not None:
            clips, B = rows
            x, y = x.reshape(B, -1)[clips], y.reshape(B, -1)[clips]
        assert torch.equal(_words(x), _words(y)), k


def _planted(c, s, a):
    """NaN payloads, -0.0, an infinity and a denormal in every pad frame of s and of a"""
    return P.planted(s, c["Tc"]), P.planted(a.unsqueeze(1), c["Tc"]).squeeze(1)


@functools.lru_cache(maxsize=None)
def _run(index):
    """case ``index`` through the C ABI, once: from the clean inputs and from inputs with the pad pattern planted in s and a"""
    c = P.CASES[index]
    s, a, g, _, _ = P.case_reference(index)
    sp, ap = _planted(c, s, a)
    return dict(clean=_both(s, a, g, c["Tc"], c["which"]), planted=_both(sp, ap, g, c["Tc"], c["which"]), sp=sp, ap=ap)


WORST = {}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_c_abi_against_fp64_within_eight_times_the_fp32_restatement(c):
    s, a, g, ref, r32 = P.case_reference(c["index"])
    r = _run(c["index"])["clean"]
    B, C, M, T = c["shape"]
    assert r["y"].shape == (B, len(P.selected(c["which"])) * C, M) and r["ds"].shape == c["shape"] and r["da"].shape == (B, c["A"], T)
    b, w32 = P.bounds(r32, ref, c)
    got = P.errors(r["y"], r["ds"], r["da"], ref, c)               # (an element of zero scale -- every pad frame, the -inf frame -- must compare equal to 0)
    failed = []
    for k, v in got.items():
        ratio = v / w32[k] if w32[k] else (0.0 if v == 0 else float("inf"))
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        WORST[k + "_err"] = max(WORST.get(k + "_err", 0.0), v)
        print(f"attnpool {P.case_id(c)} {k}: kernel {v:.3e} fp32 restatement {w32[k]:.3e} ratio {ratio:.2f} bound {b[k]:.3e}")
        if not v <= b[k]:
            failed.append((k, v, w32[k]))
    assert not failed, (P.case_id(c), failed)
    # the unrounded pairs: y's groups are their roundings (sqrt(var + eps) for the std); they are the reference's to fp64 accuracy
    parts = P.split(r["y"], c["which"], C)
    if "mean" in parts:
        assert torch.equal(_bits(r["stats"][:, 0].to(torch.float32)), _bits(parts["mean"].reshape(-1)))
    if "std" in parts:
        assert torch.equal(_bits(torch.sqrt(r["stats"][:, 1] + P.EPS).to(torch.float32)), _bits(parts["std"].reshape(-1)))
    assert torch.equal(r["norm"][:, 0], ref["norm"][:, 0])                             # the maximum of fp32 logits is exact
    assert torch.allclose(r["norm"][:, 1], ref["norm"][:, 1], rtol=1e-12, atol=0)


def test_worst_ratios_over_the_cases():
    """(prints what the cases above measured; DESIGN 4.18 quotes it)"""
    print("attnpool worst kernel / fp32 restatement ratio and worst kernel error over all cases:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_pad_frames_planted_pad_frames_the_constant_row_and_the_minus_infinity_frame_bit_for_bit(c):
    """what the pad frames of s and a hold -- NaN payloads, -0.0, an infinity, a denormal -- changes no bit of y, stats, norm, ds or da; ds
    and da are +0.0 words on pad frames; the planted constant row gives mean == c and std == float32(sqrt(float64(eps))); the frame whose
    logit is -inf gets ds == 0 and da == 0"""
    s, a, g, ref, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r, rp = run["clean"], run["planted"]
    B, C, M, T = c["shape"]
    _same(rp, r)
    valid = P.valid_mask(c["shape"], c["Tc"])
    assert not bool(_bits(r["ds"])[~valid.expand(c["shape"])].any()) and not bool(_bits(r["da"])[~valid[:, 0].expand(B, c["A"], T)].any())
    if c["Tc"] is not None and any(C * M * (T - tc) >= len(P.PAD_PATTERN) for tc in c["Tc"]):      # a clip with that many pad frames holds the whole pattern
        assert set(P.PAD_PATTERN) <= {int(v) & 0xFFFFFFFF for v in _bits(run["sp"])[~valid.expand(c["shape"])].tolist()}
    parts = P.split(r["y"], c["which"], C)
    k = c["const"]
    if "mean" in parts:
        assert _bits(parts["mean"]).reshape(-1)[k] == _bits(s).reshape(-1, T)[k, 0]
    if "std" in parts:
        assert int(_bits(parts["std"]).reshape(-1)[k]) == STD_BITS
    assert r["stats"][k].tolist() == [float(s.reshape(-1, T)[k, 0]), 0.0]
    if c["ninf"] is not None:
        b, lr, t = c["ninf"]
        group = C * M // c["A"]
        assert float(r["da"][b, lr, t]) == 0.0 and not bool(r["ds"].reshape(B, c["A"], group, T)[b, lr, :, t].any())


@pytest.mark.parametrize("c", GIVEN[::3], ids=GIVEN_IDS[::3])
def test_constant_rows_of_full_precision_are_exact(c):
    """every row a constant of its own over its valid frames (silence under the log, -23.03, among them) with the pad pattern behind it, under
    the case's logits: mean == c and std == float32(sqrt(float64(eps))) bit for bit, the pairs are (c, 0), and with the std alone ds == 0"""
    B, C, M, T = c["shape"]
    _, a, _, _, _ = P.case_reference(c["index"])
    rows = torch.randn(B, C, M, 1, generator=torch.Generator().manual_seed(c["index"])).mul(10.0).expand(c["shape"]).clone()
    rows[0, 0, 0] = float(np.float32(np.log(1e-10)))
    s = P.planted(rows, c["Tc"])
    g = torch.randn(B, 2 * C, M, generator=torch.Generator().manual_seed(c["index"] + 1))
    f = _forward(s, a, c["Tc"], 3)
    parts = P.split(f["y"], 3, C)
    assert torch.equal(_bits(parts["mean"]), _bits(rows[..., 0])) and bool((_bits(parts["std"]) == STD_BITS).all())
    assert torch.equal(f["stats"][:, 0], rows[..., 0].reshape(-1).double()) and not bool(f["stats"][:, 1].any())
    ds, da = _backward(g[:, C:].contiguous(), _forward(s, a, c["Tc"], 2), c["shape"], c["Tc"], 2)
    assert bool((ds == 0).all()) and bool((da == 0).all())


@pytest.mark.parametrize("c", [c for c in P.CASES if c["Tc"] is None], ids=[i for c, i in zip(P.CASES, IDS) if c["Tc"] is None])
def test_full_lengths_give_the_bits_of_none(c):
    s, a, g, _, _ = P.case_reference(c["index"])
    full = [c["shape"][3]] * c["shape"][0]
    _same(_both(s, a, g, full, c["which"]), _run(c["index"])["clean"])


@pytest.mark.parametrize("c", [c for c in GIVEN if c["shape"][0] > 1], ids=[P.case_id(c) for c in GIVEN if c["shape"][0] > 1])
def test_a_clip_alone_gives_the_bits_it_has_inside_the_batch(c):
    s, a, g, _, _ = P.case_reference(c["index"])
    r = _run(c["index"])["clean"]
    B = c["shape"][0]
    for b in sorted({0, B - 1, B // 2}):
        alone = _both(s[b:b + 1], a[b:b + 1], g[b:b + 1], c["Tc"][b:b + 1], c["which"])
        for k in SAME:
            assert torch.equal(_words(alone[k].reshape(1, -1)), _words(r[k].reshape(B, -1)[b:b + 1])), (b, k)


@pytest.mark.parametrize("c", P.CASES[::5], ids=IDS[::5])
def test_two_runs_give_the_same_bits(c):
    _, _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    _same(_both(run["sp"], run["ap"], g, c["Tc"], c["which"]), run["planted"])


@pytest.mark.parametrize("c", [c for c in GIVEN if c["which"] == 3][::2], ids=[P.case_id(c) for c in GIVEN if c["which"] == 3][::2])
def test_a_single_statistic_equals_its_group_of_both(c):
    """a single statistic's y is the matching group of which = 3, with the same pairs; without the buffers the backward reads (what the
    module passes under no_grad) y keeps its bits"""
    r = _run(c["index"])
    C = c["shape"][1]
    both = P.split(r["planted"]["y"], 3, C)
    for which in (1, 2):
        f = _forward(r["sp"], r["ap"], c["Tc"], which)
        for k, v in P.split(f["y"], which, C).items():
            assert torch.equal(_bits(v), _bits(both[k])), (which, k)
        assert torch.equal(_words(f["stats"]), _words(r["planted"]["stats"])) and torch.equal(_words(f["norm"]), _words(r["planted"]["norm"])), which
    assert torch.equal(_bits(_forward(r["sp"], r["ap"], c["Tc"], 3, keep=False)["y"]), _bits(r["planted"]["y"]))


INVALID = [i for i, c in enumerate(P.CASES) if c["shape"] in ((3, 1, 5, 2), (4, 1, 4, 32), (2, 1, 3, 65), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5))
           and c["which"] == 3 and c["Tc"] is not None]


@pytest.mark.parametrize("bad_length", ["zero", "T_plus_one"])
@pytest.mark.parametrize("idx", INVALID, ids=lambda i: IDS[i])
def test_an_invalid_length_poisons_its_own_clip_only(idx, bad_length):
    c = P.CASES[idx]
    s, a, g, _, _ = P.case_reference(idx)
    r = _run(idx)["clean"]
    B, T = c["shape"][0], c["shape"][3]
    for which in (0, B - 1):
        Tc = P.lengths_of(c)
        Tc[which] = 0 if bad_length == "zero" else T + 1
        got = _both(s, a, g, Tc, 3)
        for k in ("y", "ds", "da"):
            assert bool((_bits(got[k][which]) == NAN_BITS).all()), k
        assert bool(torch.isnan(got["stats"].reshape(B, -1)[which]).all()) and bool(torch.isnan(got["norm"].reshape(B, -1)[which]).all())
        _same(got, r, rows=([b for b in range(B) if b != which], B))


ODD = [i for i, c in enumerate(P.CASES) if c["shape"] in ((3, 1, 5, 2), (2, 1, 3, 33), (2, 1, 3, 65), (2, 3, 5, 40)) and c["which"] == 3 and c["Tc"] is not None]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("idx", ODD, ids=lambda i: IDS[i])
def test_inputs_at_odd_element_offsets_give_the_aligned_bits(idx, k):
    """s, a and g start 4 + k elements behind a 16-byte boundary"""
    c = P.CASES[idx]
    _, _, g, _, _ = P.case_reference(idx)
    run = _run(idx)
    _same(_both(run["sp"], run["ap"], g, c["Tc"], 3, offset=4 + k), run["planted"])


# ---- the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CASES[::2], ids=IDS[::2])
def test_module_gives_the_c_abi_bits(c):
    """dmel_amd.AttentivePool with int64 frame_lengths (narrowed on the device): y and the gradients torch.autograd reaches for s and the
    logits are the C ABI's; every shape of the logits the case allows, a (B, n_mels, T) view where there is one channel, int32 lengths and
    non-contiguous inputs give the same bits"""
    import dmel_amd
    _, _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r = run["planted"]
    B, C, M, T = c["shape"]
    m = dmel_amd.AttentivePool(P.selected(c["which"])[::-1], eps=P.EPS)
    Tc = None if c["Tc"] is None else torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    x, l = run["sp"].to(DEV).requires_grad_(True), run["ap"].to(DEV).requires_grad_(True)
    y = m(x, l, Tc)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert y.shape == r["y"].shape and y.dtype == torch.float32 and x.grad.shape == x.shape and l.grad.shape == l.shape
    assert torch.equal(_bits(y).cpu(), _bits(r["y"])) and torch.equal(_bits(x.grad).cpu(), _bits(r["ds"])) and torch.equal(_bits(l.grad).cpu(), _bits(r["da"]))
    shaped = []
    if c["A"] == 1:
        shaped.append(run["ap"].to(DEV).reshape(B, T))
    if c["A"] == C * M:
        shaped.append(run["ap"].to(DEV).reshape(B, C, M, T))
    for l2 in shaped:
        l2.requires_grad_(True)
        y2 = m(run["sp"].to(DEV), l2, Tc)
        y2.backward(g.to(DEV))
        assert torch.equal(_bits(y2).cpu(), _bits(r["y"])) and l2.grad.shape == l2.shape and torch.equal(_bits(l2.grad).cpu().reshape(-1), _bits(r["da"]).reshape(-1))
    if C == 1:
        y3 = m.eval()(run["sp"].to(DEV).reshape(B, M, T), run["ap"].to(DEV), None if Tc is None else Tc.to(torch.int32))
        assert y3.shape == y.shape and torch.equal(_bits(y3).cpu(), _bits(r["y"]))
    wide, lwide = torch.zeros((B, C, M, T + 3), device=DEV), torch.zeros((B, c["A"], T + 2), device=DEV)
    wide[..., :T], lwide[..., :T] = run["sp"].to(DEV), run["ap"].to(DEV)
    assert torch.equal(_bits(m(wide[..., :T], lwide[..., :T], Tc)).cpu(), _bits(r["y"]))


def test_module_saves_stats_and_norm_only_when_a_gradient_is_wanted(monkeypatch):
    """what reaches dmel_attnpool_forward: the fp64 pairs when s or the logits need a gradient, neither under no_grad or for inputs that
    need none; a gradient comes back for the input that asked only"""
    import dmel_amd
    from dmel_amd import capi
    seen = []
    real = capi.attnpool_forward

    def spy(*args):
        seen.append((args[10] is not None, args[11] is not None))
        return real(*args)

    monkeypatch.setattr(capi, "attnpool_forward", spy)
    s, a = torch.rand(2, 1, 3, 9, device=DEV), torch.rand(2, 9, device=DEV)
    for stats in (("mean",), ("std",), ("mean", "std")):
        m = dmel_amd.AttentivePool(stats)
        for need_s, need_a in ((True, True), (True, False), (False, True)):
            x, l = s.clone().requires_grad_(need_s), a.clone().requires_grad_(need_a)
            y = m(x, l)
            assert seen[-1] == (True, True) and len([t for t in y.grad_fn.saved_tensors if t is not None]) == 4
            y.sum().backward()
            assert (x.grad is not None) == need_s and (l.grad is not None) == need_a
            with torch.no_grad():
                z = m(x, l)
            assert seen[-1] == (False, False) and z.grad_fn is None and torch.equal(_bits(z), _bits(y))
        m(s, a)
        assert seen[-1] == (False, False)


def test_module_with_an_int64_length_beyond_32_bits_gives_a_nan_clip():
    import dmel_amd
    s, a = torch.rand(2, 1, 3, 9, device=DEV).requires_grad_(True), torch.rand(2, 3, 9, device=DEV).requires_grad_(True)
    y = dmel_amd.AttentivePool()(s, a, torch.tensor([(1 << 32) + 5, 9], dtype=torch.int64, device=DEV))
    y.sum().backward()
    for t in (y, s.grad, a.grad):
        assert bool(torch.isnan(t[0]).all()) and bool(torch.isfinite(t[1]).all())
    with pytest.raises(RuntimeError, match="frame_lengths is on cpu"):
        dmel_amd.AttentivePool()(s, a, torch.tensor([9, 9]))
    with pytest.raises(RuntimeError, match="logits are on cpu"):
        dmel_amd.AttentivePool()(s, a.detach().cpu())
    with pytest.raises(RuntimeError, match="bfloat16"):
        dmel_amd.AttentivePool()(s.detach().to(torch.bfloat16), a)


def test_captured_step_replays_the_eager_bits():
    """forward + backward captured into a graph (frame_lengths is read on the device only): three replays give the eager bits"""
    import dmel_amd
    c = next(c for c in P.CASES if c["shape"] == (2, 3, 5, 40) and c["A"] == 3)
    _, _, g, _, _ = P.case_reference(c["index"])
    run = _run(c["index"])
    r = run["planted"]
    s, a, g, Tc = run["sp"].to(DEV), run["ap"].to(DEV), g.to(DEV), torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    m = dmel_amd.AttentivePool()

    def step(x, l):
        y = m(x, l, Tc)
        return (y,) + torch.autograd.grad(y, [x, l], g)

    # (leaves of their own, first used on the side stream, and no autograd graph outliving the warm-up: see tests/test_hip_bandnorm.py)
    x_c, l_c = s.clone().requires_grad_(True), a.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x_c, l_c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, ds_c, da_c = step(x_c, l_c)
    for _ in range(3):
        for t in (y_c, ds_c, da_c):
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y_c).cpu(), _bits(r["y"])) and torch.equal(_bits(ds_c).cpu(), _bits(r["ds"])) and torch.equal(_bits(da_c).cpu(), _bits(r["da"]))


# ---- behind the layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", ["fixed", "from_the_image"])
@pytest.mark.parametrize("front", ["layer", "bandnorm_clip"])
def test_behind_the_layers_lambd_grad_follows_the_oracles_chain(front, logits):
    """pool([norm](layer(x, lengths)[, fl]), a, fl) with the log, n_fft 1024, 81 frames, lengths 4000 / 1234 / 50 (81 / 25 / 2 frames):
    lambd.grad against the oracle's chain -- clip by clip at the clip's own length, then the fp64 adjoint of the restatement -- within 1e-4
    of sum |dS64 tangent64|, the project's bar (the measured distance is printed).  Once with fixed random logits, once with logits computed
    from the image, a = (z v).sum(bands), so that both paths of the gradient carry weight"""
    import dmel_amd
    import bandnorm_cases as N
    from test_hip_bandnorm import B_L, HOP, LAM, LENS, L_L, M_L, SR, _check_dlambd, _oracle_pieces, _x
    x_np = _x()
    T = L_L // HOP + 1
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(B_L, 2, M_L, generator=gen)
    a_fixed = 2.0 * torch.randn(B_L, 1, T, generator=gen)
    v = 0.05 * torch.randn(M_L, 1, generator=gen)
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
    a = a_fixed.to(DEV) if logits == "fixed" else (z[:, 0] * v.to(DEV)).sum(1, keepdim=True)
    y = dmel_amd.AttentivePool(eps=P.EPS)(z, a, fl)
    assert y.shape == (B_L, 2, M_L) and y.dtype == torch.float32
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out, tan = _oracle_pieces(x_np, [LAM], True)
    S = torch.from_numpy(out[0]).double().requires_grad_(True)                                      # (B, 1, M, T)
    z_ref = N.forward(S, prm[0].double(), prm[1].double(), Tc, "clip") if front == "bandnorm_clip" else S
    a_ref = a_fixed.double() if logits == "fixed" else (z_ref[:, 0] * v.double()).sum(1, keepdim=True)
    y_ref, _, _ = P.forward(z_ref, a_ref, Tc.tolist(), 3)
    (dS,) = torch.autograd.grad((y_ref * g.double()).sum(), [S])
    _check_dlambd(f"AttentivePool/{front}/{logits}", lay.lambd.grad, dS, [tan[0]])
    # the stage itself on what stands in front of it (pad frames hold log(1e-10), or BandNorm's +0.0, and are never read)
    zc, ac = z.detach().cpu(), a.detach().cpu()
    own = P.reference(zc, ac, g, Tc.tolist(), 3)
    assert all(e <= 1e-4 for e in P.errors(y.detach().cpu(), None, None, own, dict(shape=tuple(zc.shape), which=3)).values())


# ---- nets.MelAttnPoolNet ------------------------------------------------------------------------------------------------------------------
N_POINTS, HOP_N, MELS, CLIP = 4000, 64, 40, 1234


def _net(seed=0, **kw):
    from dmel_amd import nets
    torch.manual_seed(seed)
    return nets.MelAttnPoolNet(5, 128.0, DEV, MELS, 16000, N_POINTS, hop_length=HOP_N, **kw).to(DEV)


def _batch(lengths, where, clip):
    """a zero-padded batch with ``clip`` at row ``where``; the other rows are clips of their own"""
    from dmel_amd import synth
    x = torch.from_numpy(synth.waveforms(len(lengths), N_POINTS, seed=11)).clone()
    x[where] = clip
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
    return x.to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)


class _SoftmaxOverAllFrames(torch.nn.Module):
    """the torch spelling in the stage's place: the softmax and the statistics over all T frames of the batch"""

    def forward(self, s, a, fl=None):
        w = torch.softmax(a, -1).unsqueeze(1) if a.shape[1] == 1 else torch.softmax(a, -1).reshape(s.shape)
        mu = (w * s).sum(-1)
        sd = torch.sqrt((w * (s - mu.unsqueeze(-1)) ** 2).sum(-1) + 1e-5)
        return torch.cat([mu, sd], dim=1)


@pytest.mark.parametrize("attention", ["shared", "band"])
def test_mel_attn_pool_net_logits_do_not_depend_on_the_batch(attention):
    """a clip of 1234 samples alone and inside batches of other lengths and positions: its logits stay within 1e-4 max|logits| (the scorer
    and the head are rocBLAS / MIOpen, whose tiling may differ with the batch size: bits are not demanded; the measured difference is
    printed); with torch.softmax over all T frames in the stage's place they move by more than that"""
    from dmel_amd import synth
    net = _net(attention=attention).eval()
    clip = torch.zeros(N_POINTS)
    clip[:CLIP] = torch.from_numpy(synth.waveforms(1, N_POINTS, seed=5))[0, :CLIP]
    arrangements = (([CLIP, N_POINTS, 50], 0), ([N_POINTS, 50, CLIP], 2), ([777, CLIP, 3000], 1), ([1, CLIP, N_POINTS - 1], 1))
    with torch.no_grad():
        alone, s = net(*_batch([CLIP], 0, clip))
        assert alone.shape == (1, 5) and s.shape == (1, 1, MELS, N_POINTS // HOP_N + 1) and bool(torch.isfinite(alone).all())
        bar = 1e-4 * float(alone.abs().max())
        worst = 0.0
        for lengths, where in arrangements:
            logits, _ = net(*_batch(lengths, where, clip))
            worst = max(worst, float((logits[where] - alone[0]).abs().max()))
        print(f"MelAttnPoolNet/{attention}: max |logits in a batch - logits alone| = {worst:.3e}, bar {bar:.3e} (max|logits| {float(alone.abs().max()):.3e})")
        assert worst <= bar
        # the same net with the softmax over all T frames: the clip alone (T = 63 frames, 20 of them valid) against the stage
        net.pool = _SoftmaxOverAllFrames()
        wrong, _ = net(*_batch([CLIP], 0, clip))
        moved = float((wrong[0] - alone[0]).abs().max())
        print(f"MelAttnPoolNet/{attention}: with torch.softmax over all T frames the short clip's logits move by {moved:.3e}")
        assert moved > bar


def test_mel_attn_pool_net_none_gives_the_bits_of_full_lengths():
    from dmel_amd import synth
    net = _net().eval()
    with torch.no_grad():
        x, _ = _batch([N_POINTS, N_POINTS], 0, torch.from_numpy(synth.waveforms(1, N_POINTS, seed=6))[0])
        full, s_full = net(x, torch.tensor([N_POINTS, N_POINTS], dtype=torch.int32, device=DEV))
        none, s_none = net(x)
        assert torch.equal(_bits(none), _bits(full)) and torch.equal(_bits(s_none), _bits(s_full))


def test_mel_attn_pool_net_trains_with_and_without_the_opt_in_stages():
    import dmel_amd
    from dmel_amd import nets, synth
    clip = torch.from_numpy(synth.waveforms(1, N_POINTS, seed=5))[0]
    x, lengths = _batch([CLIP, N_POINTS, 50], 0, clip)
    labels = torch.tensor([0, 3, 1], device=DEV)
    for staged in (False, True):
        net = _net(seed=1, attention="band" if staged else "shared")
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
        for name in ("spectrogram_layer.lambd", "attention_fc1.weight", "fc.weight"):
            assert not torch.equal(dict(net.named_parameters())[name].detach(), before[name]), (staged, name)
