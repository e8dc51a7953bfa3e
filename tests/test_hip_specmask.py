"""SpecMask on the MI355X (dmel_specmask_draw / dmel_specmask_apply, dmel_amd.SpecMask) against the integer restatement of
tests/specmask_cases.py: the stripe table integer for integer, y and ds bit for bit (fp32 and bf16, NaN-filled outputs between guards), pad
frames, invalid lengths, every address path, the call counter, the module, a captured step, and the stage behind the scalar layer and
BandNorm and behind the small nets.  The stage only selects: no tolerance appears anywhere."""
import numpy as np
import pytest
import torch

import bandnorm_cases as N
import specmask_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                   # elements: a multiple of 16 bytes for both element sizes
IDS = [S.case_id(c) for c in S.CASES]
INT = {4: torch.int32, 2: torch.int16}
UINT = {4: np.uint32, 2: np.uint16}
FLOAT = {4: torch.float32, 2: torch.bfloat16}
SENTINEL = {4: 0x5EA15EA1, 2: 0x5EA1}


def _to_dev(bits):
    """a numpy array of element bits as a device tensor of the signed integer type of that width"""
    return torch.from_numpy(bits.view(np.int32 if bits.dtype.itemsize == 4 else np.int16).copy()).to(DEV)


def _to_bits(t, elem_bytes):
    return t.detach().contiguous().view(INT[elem_bytes]).cpu().numpy().view(UINT[elem_bytes])


def _guarded(n, elem_bytes, offset=0):
    """n elements of NaN bits, ``offset`` elements behind a 16-byte boundary, between sentinel words: (whole buffer, the n elements, check)"""
    buf = torch.full((n + 2 * GUARD + offset,), SENTINEL[elem_bytes], dtype=INT[elem_bytes], device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.fill_(S.NAN_BITS[elem_bytes])

    def intact():
        return bool((buf[:GUARD + offset] == SENTINEL[elem_bytes]).all()) and bool((buf[GUARD + offset + n:] == SENTINEL[elem_bytes]).all())

    return buf, view, intact


def _placed(bits, offset):
    """the device copy of ``bits`` starting ``offset`` elements behind a 16-byte boundary, sentinel words on both sides"""
    eb = bits.dtype.itemsize
    buf, view, _ = _guarded(bits.size, eb, offset)
    view.copy_(_to_dev(bits).reshape(-1))
    return buf, view


def _signed(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def _state(seed, calls):
    return torch.tensor([_signed(seed), _signed(calls)], dtype=torch.int64, device=DEV)


def _draw(c, Tc, state, advance):
    """dmel_specmask_draw for case ``c``: (the table as numpy between intact guards, the device table)"""
    from dmel_amd import capi
    B, Cn, M, T = c["shape"]
    n = c["n_time"] + c["n_freq"]
    tbuf = torch.full((B * Cn * n * 2 + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    tab = tbuf[GUARD:GUARD + B * Cn * n * 2]
    lens = None if Tc is None else torch.tensor(Tc, dtype=torch.int32, device=DEV)
    capi.specmask_draw(B * Cn, Cn, M, T, None if lens is None else lens.data_ptr(), c["time_param"], c["time_permille"], c["n_time"], c["freq_param"],
                       c["n_freq"], state.data_ptr(), advance, tab.data_ptr() if n else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((tbuf[:GUARD] == -77).all()) and bool((tbuf[GUARD + tab.numel():] == -77).all())
    return tab.cpu().numpy().reshape(B * Cn, n, 2), tab, lens


def _apply(c, view, tab, lens, elem_bytes, fill, y_offset=0):
    """dmel_specmask_apply from the device elements ``view`` into a NaN-filled guarded output: its bits as a (B, C, n_mels, T) numpy array"""
    from dmel_amd import capi
    B, Cn, M, T = c["shape"]
    n = c["n_time"] + c["n_freq"]
    ybuf, y, intact = _guarded(view.numel(), elem_bytes, y_offset)
    capi.specmask_apply(view.data_ptr(), B * Cn * M, M, Cn * M, T, None if lens is None else lens.data_ptr(), tab.data_ptr() if n else None,
                        c["n_time"], c["n_freq"], elem_bytes == 2, fill, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact()
    return _to_bits(y, elem_bytes).reshape(c["shape"])


def _check_case(c, elem_bytes, Tc, s_offset=0):
    s_bits, g_bits = S.input_bits(c["shape"], Tc, c["seed"], elem_bytes)
    state = _state(c["seed"], c["calls"])
    got_tab, tab, lens = _draw(c, Tc, state, True)
    want_tab = S.table(c["shape"], Tc, c["time_param"], c["time_permille"], c["n_time"], c["freq_param"], c["n_freq"], c["seed"], c["calls"])
    assert got_tab.dtype == want_tab.dtype and np.array_equal(got_tab, want_tab)
    moved = 1 if c["n_time"] + c["n_freq"] else 0
    assert state.tolist() == [_signed(c["seed"]), _signed(c["calls"] + moved)]
    (_, s_view), (_, g_view) = _placed(s_bits, s_offset), _placed(g_bits, s_offset)
    y = _apply(c, s_view, tab, lens, elem_bytes, c["fill"])
    ds = _apply(c, g_view, tab, lens, elem_bytes, 0.0)
    assert np.array_equal(y, S.apply(s_bits, Tc, want_tab, c["n_time"], c["fill"]))
    assert np.array_equal(ds, S.apply(g_bits, Tc, want_tab, c["n_time"], 0.0))
    return s_bits, g_bits, y, ds, want_tab


@pytest.mark.parametrize("elem_bytes", [4, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_c_abi_table_integer_for_integer_and_outputs_bit_for_bit(c, elem_bytes):
    _check_case(c, elem_bytes, c["Tc"])


@pytest.mark.parametrize("elem_bytes", [4, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [c for c in S.CASES if c["Tc"] is not None], ids=[i for c, i in zip(S.CASES, IDS) if c["Tc"] is not None])
def test_pad_frames_keep_the_inputs_bits(c, elem_bytes):
    """every pad frame of y and ds holds what s and g hold there: a NaN with its payload, -0.0, an infinity, a denormal"""
    s_bits, g_bits, y, ds, _ = _check_case(c, elem_bytes, c["Tc"])
    B, Cn, M, T = c["shape"]
    pad = np.broadcast_to(np.arange(T)[None, None, None, :] >= np.asarray(c["Tc"]).reshape(B, 1, 1, 1), c["shape"])
    assert np.array_equal(y[pad], s_bits[pad]) and np.array_equal(ds[pad], g_bits[pad])
    if elem_bytes == 4 and any(T - t >= len(S.PAD_PATTERN) for t in c["Tc"]):      # a run of pad frames that long holds the whole pattern
        assert set(S.PAD_PATTERN) <= set(int(v) for v in y[pad])


@pytest.mark.parametrize("bad_length", ["zero", "T_plus_one"])
@pytest.mark.parametrize("elem_bytes", [4, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("idx", [5, 9, 24, 25], ids=lambda i: IDS[i])
def test_an_invalid_length_poisons_its_own_clip_only(idx, elem_bytes, bad_length):
    """one clip gets a length outside 1 ... T: every element of its rows is NaN in y and ds and its table rows are zero; the other clips have
    the bits of the restatement (which draws per image: they are the clean run's)"""
    c = S.CASES[idx]
    B, Cn, M, T = c["shape"]
    clean = list(c["Tc"]) if c["Tc"] is not None else [T] * B
    for which in (0, B - 1):
        Tc = list(clean)
        Tc[which] = 0 if bad_length == "zero" else T + 1
        s_bits, g_bits, y, ds, tab = _check_case(c, elem_bytes, Tc)
        nan = S.NAN_BITS[elem_bytes]
        assert bool((y[which] == nan).all()) and bool((ds[which] == nan).all())
        assert not tab[which * Cn:(which + 1) * Cn].any()
        others = [b for b in range(B) if b != which]
        clean_tab = S.table(c["shape"], clean, c["time_param"], c["time_permille"], c["n_time"], c["freq_param"], c["n_freq"], c["seed"], c["calls"])
        want = S.apply(s_bits, clean, clean_tab, c["n_time"], c["fill"])
        assert np.array_equal(y[others], want[others])


ODD = dict(shape=(2, 3, 7, 33), Tc=[33, 16], n_time=2, n_freq=2, time_param=20, freq_param=4, time_permille=1000, calls=5, seed=S.SEED + 99, fill=-1.5)
ODD_SMALL = dict(ODD, shape=(3, 1, 3, 5), Tc=[5, 2, 3], time_param=4, freq_param=2)


@pytest.mark.parametrize("c", [ODD, ODD_SMALL], ids=["2x3x7x33", "3x1x3x5"])
@pytest.mark.parametrize("elem_bytes,k", [(4, k) for k in range(4)] + [(2, k) for k in range(8)], ids=lambda v: str(v))
def test_every_address_path_gives_the_bits(c, elem_bytes, k):
    """s and g start 4 + k elements behind a 16-byte boundary (every residue of the element inside a granule), y is 16-byte aligned as the
    contract asks, T and n_mels * T are odd: images whose s and y sit alike in a granule take the 16-byte path with partial granules at both
    ends, the others the element-wide one -- both inside one call"""
    _check_case(c, elem_bytes, c["Tc"], s_offset=4 + k)


def test_misaligned_output_is_refused():
    from dmel_amd import capi
    c = ODD_SMALL
    s_bits, _ = S.input_bits(c["shape"], c["Tc"], 1, 4)
    _, s_view = _placed(s_bits, 0)
    _, tab, lens = _draw(c, c["Tc"], _state(1, 0), False)
    ybuf, y, intact = _guarded(s_bits.size, 4, 1)
    with pytest.raises(capi.DmelError, match="y must be a 16-byte aligned"):
        capi.specmask_apply(s_view.data_ptr(), 9, 3, 3, 5, lens.data_ptr(), tab.data_ptr(), 2, 2, False, 0.0, y.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert intact() and bool((y == S.NAN_BITS[4]).all())


def test_the_counter_moves_by_one_per_advancing_call():
    c = S.CASES[25]                                                                # (2, 1, 64, 81), four and four stripes
    for calls in (0, (1 << 32) - 1, (1 << 64) - 1):                                # the carries into the high word and around
        state = _state(c["seed"], calls)
        tabs = [_draw(c, c["Tc"], state, True)[0] for _ in range(2)]
        assert state.tolist() == [_signed(c["seed"]), _signed(calls + 2)]
        for j, got in enumerate(tabs):
            assert np.array_equal(got, S.case_table(c, calls=(calls + j) & 0xFFFFFFFFFFFFFFFF)), (calls, j)
        assert not np.array_equal(tabs[0], tabs[1])
        pinned = [_draw(c, c["Tc"], state, False)[0] for _ in range(2)]
        assert state.tolist() == [_signed(c["seed"]), _signed(calls + 2)]
        assert np.array_equal(pinned[0], pinned[1]) and np.array_equal(pinned[0], S.case_table(c, calls=(calls + 2) & 0xFFFFFFFFFFFFFFFF))


# ---- the module -------------------------------------------------------------------------------------------------------------------------
def _module(c, seed=None, calls=None):
    import dmel_amd
    m = dmel_amd.SpecMask(c["time_param"], c["freq_param"], time_stripes=c["n_time"], freq_stripes=c["n_freq"],
                          max_time_fraction=c["time_permille"] / 1000.0, fill_value=c["fill"], seed=c["seed"] if seed is None else seed).to(DEV)
    return m.manual_seed(c["seed"] if seed is None else seed, c["calls"] if calls is None else calls)


def _tensors(c, elem_bytes):
    s_bits, g_bits = S.input_bits(c["shape"], c["Tc"], c["seed"], elem_bytes)
    s = _to_dev(s_bits).view(FLOAT[elem_bytes]).reshape(c["shape"])
    g = _to_dev(g_bits).view(FLOAT[elem_bytes]).reshape(c["shape"])
    Tc = None if c["Tc"] is None else torch.tensor(c["Tc"], dtype=torch.int64, device=DEV)
    return s_bits, g_bits, s, g, Tc


@pytest.mark.parametrize("elem_bytes", [4, 2], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_module_gives_the_restatements_bits(c, elem_bytes):
    """dmel_amd.SpecMask with int64 frame_lengths (narrowed on the device): y, the gradient and last_stripes() are the restatement's -- which the
    C ABI's are, above; a (B, n_mels, T) view where there is one channel and a non-contiguous input give the same bits"""
    s_bits, g_bits, s, g, Tc = _tensors(c, elem_bytes)
    n = c["n_time"] + c["n_freq"]
    want_tab = S.case_table(c)
    want_y, want_ds = S.apply(s_bits, c["Tc"], want_tab, c["n_time"], c["fill"]), S.apply(g_bits, c["Tc"], want_tab, c["n_time"], 0.0)
    m = _module(c)
    x = s.clone().requires_grad_(True)
    y = m(x, Tc)
    if n == 0:
        assert y is x and m.last_stripes() is None and m.rng_state.tolist() == [_signed(c["seed"]), _signed(c["calls"])]
        return
    y.backward(g)
    torch.cuda.synchronize()
    assert y.dtype == s.dtype and y.shape == s.shape
    assert np.array_equal(m.last_stripes().cpu().numpy(), want_tab)
    assert np.array_equal(_to_bits(y, elem_bytes).reshape(c["shape"]), want_y)
    assert np.array_equal(_to_bits(x.grad, elem_bytes).reshape(c["shape"]), want_ds)
    assert m.rng_state.tolist() == [_signed(c["seed"]), _signed(c["calls"] + 1)]
    B, Cn, M, T = c["shape"]
    if Cn == 1:
        m3 = _module(c)
        y3 = m3(s.reshape(B, M, T), None if Tc is None else Tc.to(torch.int32))
        assert y3.shape == (B, M, T) and np.array_equal(_to_bits(y3, elem_bytes).reshape(c["shape"]), want_y)
    wide = torch.zeros((B, Cn, M, T + 3), dtype=s.dtype, device=DEV)
    wide[..., :T] = s
    assert np.array_equal(_to_bits(_module(c)(wide[..., :T], Tc), elem_bytes).reshape(c["shape"]), want_y)


def test_eval_launches_nothing_and_returns_its_argument():
    c = S.CASES[25]
    _, _, s, _, Tc = _tensors(c, 4)
    m = _module(c).eval()
    assert m(s, Tc) is s and m.last_stripes() is None
    assert m.rng_state.tolist() == [_signed(c["seed"]), _signed(c["calls"])]       # no draw: the counter stays
    assert m.train()(s, Tc) is not s and m.rng_state.tolist() == [_signed(c["seed"]), _signed(c["calls"] + 1)]


def test_manual_seed_and_a_state_dict_round_trip_reproduce_the_next_tables():
    import dmel_amd
    c = S.CASES[25]
    _, _, s, _, Tc = _tensors(c, 4)
    m = _module(c, seed=77, calls=9)
    m(s, Tc)                                                                       # call 9
    saved = {k: v.clone() for k, v in m.state_dict().items()}
    ahead = []
    for _ in range(3):                                                             # calls 10, 11, 12
        m(s, Tc)
        ahead.append(m.last_stripes().cpu().numpy())
    for j, got in enumerate(ahead):
        assert np.array_equal(got, S.table(c["shape"], c["Tc"], c["time_param"], c["time_permille"], c["n_time"], c["freq_param"], c["n_freq"], 77, 10 + j))
    resumed = dmel_amd.SpecMask(c["time_param"], c["freq_param"], time_stripes=c["n_time"], freq_stripes=c["n_freq"],
                                max_time_fraction=c["time_permille"] / 1000.0, seed=0).to(DEV)
    resumed.load_state_dict(saved)
    again = m.manual_seed(77, calls=10)
    for j in range(3):
        resumed(s, Tc), again(s, Tc)
        assert np.array_equal(resumed.last_stripes().cpu().numpy(), ahead[j]) and np.array_equal(again.last_stripes().cpu().numpy(), ahead[j])


def test_refusals_on_the_device():
    c = S.CASES[25]
    _, _, s, _, Tc = _tensors(c, 4)
    import dmel_amd
    m = dmel_amd.SpecMask(seed=1)                                                  # its buffer stays on the CPU
    with pytest.raises(RuntimeError, match="rng_state is on cpu"):
        m(s, Tc)
    with pytest.raises(RuntimeError, match="frame_lengths is on cpu"):
        m.to(DEV)(s, Tc.cpu())
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        m(s.half(), Tc)


def test_captured_step_draws_fresh_stripes_on_every_replay():
    """forward + backward captured into a graph: the counter lives on the device, so replay r draws call number calls + r -- the
    restatement's table for it, and the eager bits of that call number in y and ds"""
    c = S.CASES[25]
    s_bits, g_bits, s, g, Tc = _tensors(c, 4)
    calls = (1 << 32) - 2                                                          # the carry into the high word happens inside the replays

    def step(m, x):
        y = m(x, Tc)
        return y, torch.autograd.grad(y, [x], g)[0]

    eager_mod, x_e = _module(c, calls=calls), s.clone().requires_grad_(True)
    eager = []
    for r in range(3):
        y, ds = step(eager_mod, x_e)
        torch.cuda.synchronize()
        eager.append((_to_bits(y, 4), _to_bits(ds, 4), eager_mod.last_stripes().cpu().numpy()))
        want_tab = S.case_table(c, calls=calls + r)
        assert np.array_equal(eager[r][2], want_tab)
        assert np.array_equal(eager[r][0].reshape(c["shape"]), S.apply(s_bits, c["Tc"], want_tab, c["n_time"], c["fill"]))
    del y, ds
    # (a leaf of its own, first used on the side stream, and no autograd graph outliving the warm-up: see tests/test_hip_bandnorm.py)
    m, x_c = _module(c, calls=calls), s.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(m, x_c)                                                               # warm-up: the allocator; it draws one call
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.manual_seed(c["seed"], calls)                                                # ... which is taken back before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_c, ds_c = step(m, x_c)
    for r in range(3):
        y_c.detach().fill_(float("nan")), ds_c.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(m.last_stripes().cpu().numpy(), eager[r][2]), r
        assert np.array_equal(_to_bits(y_c, 4), eager[r][0]) and np.array_equal(_to_bits(ds_c, 4), eager[r][1]), r
    assert m.rng_state.tolist() == [_signed(c["seed"]), _signed(calls + 3)]


# ---- behind the layers ------------------------------------------------------------------------------------------------------------------
SR, M_L, B_L = 16000, 8, 3
LAM, L_L, HOP = 128.0, 4000, 50            # n_fft 1024, 81 frames (the shape of test_hip_bandnorm.py's chain)
LENS = [L_L, 1234, 50]


@pytest.mark.parametrize("stats", ["clip", "batch"])
def test_behind_the_scalar_layer_and_bandnorm_the_gradient_is_an_exact_selection(stats):
    """mask(norm(layer(x, lengths), fl), fl): lambd.grad equals, bit for bit, that of the chain without the mask fed the cotangent g where the
    mask kept the element and +0.0 where it filled it (built on the host from last_stripes())"""
    import dmel_amd
    from dmel_amd import MelSpectrogramLayer, synth
    x = torch.from_numpy(synth.waveforms(B_L, L_L, seed=3)).to(DEV)
    T = L_L // HOP + 1
    g = torch.randn(B_L, 1, M_L, T, generator=torch.Generator().manual_seed(1)).to(DEV)
    prm = N.params(M_L, 60)
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)

    def chain(mask, cotangent):
        lay = MelSpectrogramLayer(torch.tensor(LAM), n_mels=M_L, n_points=L_L, sample_rate=SR, hop_length=HOP, device=DEV, optimized=True,
                                  log=True).to(DEV)
        norm = dmel_amd.BandNorm(M_L, stats=stats, eps=N.EPS, momentum=N.MOMENTUM)
        with torch.no_grad():
            norm.weight.copy_(prm[0]), norm.bias.copy_(prm[1])
        norm = norm.to(DEV)
        fl = lay.frame_lengths(lengths)
        z = norm(lay(x, lengths), fl)
        y = z if mask is None else mask(z, fl)
        y.backward(cotangent(y))
        torch.cuda.synchronize()
        return lay.lambd.grad.detach().cpu().clone(), z.detach().cpu(), y.detach().cpu(), fl.cpu().tolist()

    mask = dmel_amd.SpecMask(20, 3, time_stripes=2, freq_stripes=2, fill_value=0.0, seed=11).to(DEV)
    got, z, y, fl = chain(mask, lambda y: g)
    assert fl == [81, 25, 2]
    tab = mask.last_stripes().cpu().numpy()
    assert np.array_equal(tab, S.table((B_L, 1, M_L, T), fl, 20, 1000, 2, 3, 2, 11, 0))
    filled = torch.from_numpy(S.filled((B_L, 1, M_L, T), fl, tab, 2))
    assert bool(filled.any()) and bool(filled[0].any()) and not bool(filled[:, :, :, 25:][1].any())
    zb, yb = z.view(torch.int32), y.view(torch.int32)
    assert bool((yb[filled] == 0).all()) and torch.equal(yb[~filled], zb[~filled])          # pad frames keep BandNorm's +0.0 as they are
    want, z2, _, _ = chain(None, lambda y: torch.where(filled.to(DEV), torch.zeros((), device=DEV), g))
    assert torch.equal(z2.view(torch.int32), zb)
    assert bool(torch.isfinite(got).all()) and float(got.abs().sum()) > 0.0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got, want)


def test_behind_the_small_net_training_masks_and_eval_is_the_net_without_the_hook():
    import dmel_amd
    from dmel_amd import nets, synth
    n_points, hop, n_mels = 800, 80, 8
    x = torch.from_numpy(synth.waveforms(4, n_points, seed=5)).to(DEV)

    def build():
        torch.manual_seed(0)
        return nets.MelLinearNet(3, torch.tensor(10.0), DEV, n_mels, 8000, n_points, hop_length=hop, optimized=True, energy_normalize=True).to(DEV)

    plain, net = build(), build()
    net.augmentation = dmel_amd.SpecMask(6, 3, time_stripes=2, freq_stripes=2, fill_value=0.0, seed=5).to(DEV)
    with torch.no_grad():
        _, s_plain = plain.eval()(x)
        _, s_eval = net.eval()(x)
        _, s_train = net.train()(x)
    torch.cuda.synchronize()
    assert s_eval.shape == (4, 1, n_mels, n_points // hop + 1)
    assert torch.equal(s_eval.view(torch.int32), s_plain.view(torch.int32))
    tab = net.augmentation.last_stripes().cpu().numpy()
    filled = torch.from_numpy(S.filled(tuple(s_train.shape), None, tab, 2)).to(DEV)
    assert np.array_equal(tab, S.table(tuple(s_train.shape), None, 6, 1000, 2, 3, 2, 5, 0)) and bool(filled.any())
    assert bool((s_train[filled] == 0).all()) and torch.equal(s_train[~filled].view(torch.int32), s_plain[~filled].view(torch.int32))
    assert not torch.equal(s_train, s_eval)                                        # log mel power is never 0: a filled element differs
    assert list(net.state_dict().keys()) == list(plain.state_dict().keys()) + ["augmentation.rng_state"]
