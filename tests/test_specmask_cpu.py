"""SpecMask without a GPU: the numpy restatement the GPU tests compare bits with (tests/specmask_cases.py) gives Philox4x32-10's known
answers, keeps every stripe inside its support and covers, over the case list, everything the GPU equality tests need in order not to pass
vacuously; dmel_amd.SpecMask constructs, refuses and returns its argument in eval() on the CPU; the nets apply ``augmentation`` only when
asked and only in training; the two C entry points are exported, check their arguments on the host and are loud without a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import specmask_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_specmask_draw", "dmel_specmask_apply")
IDS = [S.case_id(c) for c in S.CASES]


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert _hex(S.philox(counter, key)) == want
    # the same words from uint64 arrays (what the statistics test below draws with)
    arr = S.philox([np.array([c, c], dtype=np.uint64) for c in counter], [np.array([k, k], dtype=np.uint64) for k in key])
    assert _hex(w[1] for w in arr) == want


def test_case_list_is_what_the_issue_asks_for():
    assert len(S.CASES) == len(IDS) == len(set(IDS))
    for shape in S.SHAPES:
        assert {c["Tc"] is None for c in S.CASES if c["shape"] == shape} == {True, False}, shape
    assert {(c["n_time"], c["n_freq"]) for c in S.CASES} >= set(S.STRIPES)
    assert {c["calls"] for c in S.CASES} == {0, 1, (1 << 32) + 3}
    assert {c["time_permille"] for c in S.CASES} == {1000, 200}
    assert any(c["time_param"] == 0 and c["n_time"] for c in S.CASES) and any(c["freq_param"] == 0 and c["n_freq"] for c in S.CASES)
    assert any(c["time_param"] > c["shape"][3] and c["n_time"] for c in S.CASES) and any(c["freq_param"] > c["shape"][2] and c["n_freq"] for c in S.CASES)
    lens = [(t, c["shape"][3]) for c in S.CASES if c["Tc"] is not None for t in c["Tc"]]
    assert any(t == 1 and T > 1 for t, T in lens) and any(t == T for t, T in lens) and any(1 < t < T for t, T in lens)
    assert all(c["n_time"] + c["n_freq"] <= 8 for c in S.CASES)


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_stripes_stay_inside_their_support(c):
    """0 <= lo <= hi <= size - 1 and hi - lo <= cap - 1 (no stripe at all where the cap is 0)"""
    B, Cn, M, T = c["shape"]
    tab = S.case_table(c)
    assert tab.dtype == np.int32 and tab.shape == (B * Cn, c["n_time"] + c["n_freq"], 2)
    for i in range(B * Cn):
        tc = T if c["Tc"] is None else c["Tc"][i // Cn]
        for k, (lo, hi) in enumerate(tab[i]):
            size, param = (tc, S.time_param_of(c["time_param"], c["time_permille"], tc)) if k < c["n_time"] else (M, c["freq_param"])
            cap = min(param, size)
            assert 0 <= lo <= hi <= size - 1, (i, k, lo, hi, size)
            assert hi - lo <= max(cap - 1, 0), (i, k, lo, hi, cap)


def test_the_cases_cannot_pass_vacuously():
    """Over the case list: an image with a non-empty time stripe, one with a non-empty frequency stripe, one with two overlapping stripes on
    an axis, a time stripe that reaches the last position it can (hi == Tc - 1), a clip whose cap was lowered by time_permille -- and a call
    whose table depends on the high counter word"""
    seen = dict(time=0, freq=0, overlap=0, last=0, lowered=0, filled=0)
    for c in S.CASES:
        B, Cn, M, T = c["shape"]
        tab = S.case_table(c)
        seen["filled"] += int(S.filled(c["shape"], c["Tc"], tab, c["n_time"]).any())
        for i in range(B * Cn):
            tc = T if c["Tc"] is None else c["Tc"][i // Cn]
            t_str = [(lo, hi) for lo, hi in tab[i, :c["n_time"]] if hi > lo]
            f_str = [(lo, hi) for lo, hi in tab[i, c["n_time"]:] if hi > lo]
            seen["time"] += bool(t_str)
            seen["freq"] += bool(f_str)
            for group in (t_str, f_str):
                seen["overlap"] += any(a[0] < b[1] and b[0] < a[1] for x, a in enumerate(group) for b in group[x + 1:])
            seen["last"] += any(hi == tc - 1 for _, hi in t_str)
            if c["n_time"] and tc * c["time_permille"] // 1000 < min(c["time_param"], tc):
                seen["lowered"] += any(hi > lo for lo, hi in tab[i, :c["n_time"]]) or 0
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    high = next(c for c in S.CASES if c["calls"] >> 32 and c["n_time"] + c["n_freq"])
    assert not np.array_equal(S.case_table(high), S.case_table(high, calls=high["calls"] & 0xFFFFFFFF))


@pytest.mark.parametrize("cap,size", [(8, 128), (64, 81), (16, 16), (1, 5)])
def test_widths_are_uniform_over_their_support(cap, size):
    """1e5 draws: the mean width within five standard errors of (cap - 1) / 2, every width in 0 ... cap - 1 and every start where the stripe fits"""
    n = 100000
    u64 = lambda v: np.full(n, v, dtype=np.uint64)      # noqa: E731
    w = S.philox([u64(7), u64(0), np.arange(n, dtype=np.uint64), u64(0)], [u64(S.SEED & S.MASK32), u64(S.SEED >> 32)])
    width = (w[0] * np.uint64(cap)) >> np.uint64(32)
    lo = (w[1] * (np.uint64(size) - width)) >> np.uint64(32)
    assert int(width.min()) >= 0 and int(width.max()) <= cap - 1
    assert bool((lo + width <= size - 1).all())
    assert (int(lo[5]), int(lo[5] + width[5])) == S.stripe(int(w[0][5]), int(w[1][5]), cap, size)
    sigma = np.sqrt((cap * cap - 1) / 12.0)
    assert abs(float(width.mean()) - (cap - 1) / 2.0) <= 5.0 * sigma / np.sqrt(n) + 1e-12, (width.mean(), cap)
    assert set(np.unique(width)) == set(range(cap))


def test_apply_restatement_on_a_hand_made_table():
    shape, Tc = (2, 1, 3, 6), [4, 7]
    bits = np.arange(36, dtype=np.uint32).reshape(shape) + 100
    tab = np.array([[[1, 3], [2, 3]], [[0, 1], [0, 1]]], dtype=np.int32)          # clip 0: frames 1, 2 and band 2; clip 1 is invalid
    y = S.apply(bits, Tc, tab, 1, -1.5)
    f = S.fill_bits(-1.5, 4)
    assert f == 0xBFC00000 and S.fill_bits(-1.5, 2) == 0xBFC0 and S.fill_bits(1.00390625, 2) == 0x3F80 and S.fill_bits(float("nan"), 2) == 0x7FC0
    want = bits.copy()
    want[0, 0, :, 1:3] = f
    want[0, 0, 2, :4] = f                                                          # frames 4 and 5 are pad frames: s's bits
    want[1] = 0x7FC00000
    assert np.array_equal(y, want)
    assert np.array_equal(S.apply(bits.astype(np.uint16), Tc, tab, 1, 0.0)[0, 0, 2], np.array([0, 0, 0, 0, 116, 117], dtype=np.uint16))


# ---- the module on the CPU ------------------------------------------------------------------------------------------------------------
def test_constructor_buffer_and_manual_seed():
    import dmel_amd
    assert "SpecMask" in dmel_amd.__all__
    torch.manual_seed(4242)
    m = dmel_amd.SpecMask()
    assert (m.time_mask_param, m.freq_mask_param, m.time_stripes, m.freq_stripes, m.time_permille, m.fill_value) == (64, 8, 1, 1, 1000, 0.0)
    assert list(m.state_dict().keys()) == ["rng_state"] and m.rng_state.dtype == torch.int64 and m.rng_state.tolist() == [4242, 0]
    assert not list(m.parameters()) and m.last_stripes() is None
    m2 = dmel_amd.SpecMask(20, 4, time_stripes=2, freq_stripes=3, max_time_fraction=0.2, fill_value=-1.0, seed=(1 << 64) - 1)
    assert m2.time_permille == 200 and m2.rng_state.tolist() == [-1, 0]          # the same 64 bits
    ptr = m2.rng_state.data_ptr()
    assert m2.manual_seed(7, calls=(1 << 32) + 3) is m2 and m2.rng_state.tolist() == [7, (1 << 32) + 3] and m2.rng_state.data_ptr() == ptr
    m3 = dmel_amd.SpecMask()
    m3.load_state_dict(m2.state_dict())
    assert m3.rng_state.tolist() == [7, (1 << 32) + 3]
    for kw in (dict(time_stripes=5, freq_stripes=4), dict(time_mask_param=-1), dict(freq_mask_param=1.5), dict(max_time_fraction=1.5),
               dict(max_time_fraction=-0.1), dict(time_stripes=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError, match="SpecMask"):
            dmel_amd.SpecMask(**kw)


def test_eval_and_zero_counts_return_the_argument_and_training_refuses_on_the_cpu():
    import dmel_amd
    m = dmel_amd.SpecMask(seed=1)
    s = torch.rand(2, 1, 4, 6)
    assert m.eval()(s) is s and m(s, torch.tensor([6, 3])) is s
    assert dmel_amd.SpecMask(time_stripes=0, freq_stripes=0, seed=1).train()(s) is s
    m.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(s.to(torch.bfloat16))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m(torch.rand(4, 6))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m([1.0])
    for dt in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="fp32 or bf16"):
            m(s.to(dt))
    with pytest.raises(TypeError, match="1-D integer tensor"):
        m(s, [6, 3])
    with pytest.raises(TypeError, match="int32 or int64"):
        m(s, torch.tensor([6.0, 3.0]))
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        m(s, torch.tensor([6, 3, 1]))
    assert m.rng_state.tolist() == [1, 0] and m.last_stripes() is None


def test_features_apply_augmentation_only_when_set_and_only_in_training():
    from dmel_amd import nets
    net = nets.MelLinearNet(3, torch.tensor(10.0), "cpu", 8, 8000, 800, hop_length=80, optimized=True)
    assert not hasattr(net, "augmentation")
    keys = list(net.state_dict().keys())
    s = torch.rand(2, 1, 8, 11)
    net.spectrogram_layer.forward = lambda x: s               # the front end needs the GPU
    assert net._features(torch.zeros(2, 800)) is s
    seen = []

    class Twice(torch.nn.Module):
        def forward(self, e):
            seen.append(e)
            return 2 * e

    net.compression = Twice()
    net.augmentation = Twice()
    out = net.train()._features(torch.zeros(2, 800))
    assert len(seen) == 2 and seen[0] is s and torch.equal(seen[1], 2 * s) and torch.equal(out, 4 * s)      # behind the compression
    assert torch.equal(net.eval()._features(torch.zeros(2, 800)), 2 * s) and len(seen) == 3
    net.compression = net.augmentation = None
    assert net.train()._features(torch.zeros(2, 800)) is s
    import dmel_amd
    net.augmentation = dmel_amd.SpecMask(seed=3)
    assert list(net.state_dict().keys()) == keys + ["augmentation.rng_state"]
    assert net.eval()._features(torch.zeros(2, 800)) is s
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.train()._features(torch.zeros(2, 800))


# ---- the C entry points on the host -----------------------------------------------------------------------------------------------------
def test_symbols_listed_exported_and_named():
    from dmel_amd import capi
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert L.dmel_abi_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NAMES)


def _draw(L, **kw):
    a = dict(images=4, channels=1, n_mels=8, T=10, lengths=None, time_param=4, time_permille=1000, n_time=1, freq_param=2, n_freq=1,
             rng_state=C.c_void_p(64), advance=1, stripes=C.c_void_p(64), stream=None)
    a.update(kw)
    return L.dmel_specmask_draw(*a.values())


def _apply(L, **kw):
    a = dict(s=C.c_void_p(64), rows=16, n_mels=8, rows_per_clip=8, T=10, lengths=None, stripes=C.c_void_p(64), n_time=1, n_freq=1, elem_bf16=0,
             fill=C.c_float(0.0), y=C.c_void_p(64), stream=None)
    a.update(kw)
    return L.dmel_specmask_apply(*a.values())


def test_argument_checks_need_no_device_and_name_the_argument():
    """(the pointers are never dereferenced: every refusal comes before the first launch, and this machine has no device)"""
    from dmel_amd import capi
    L = capi.load()
    INVALID = 1
    for kw, word in ((dict(rng_state=None), "rng_state"), (dict(rng_state=C.c_void_p(68)), "rng_state"), (dict(stripes=None), "stripes"),
                     (dict(n_time=5, n_freq=4), "n_time + n_freq <= 8"), (dict(n_time=-1), "n_time"), (dict(time_param=-1), "time_param"),
                     (dict(freq_param=-3), "freq_param"), (dict(time_permille=1001), "time_permille"), (dict(time_permille=-1), "time_permille"),
                     (dict(channels=3), "channels"), (dict(channels=0), "channels"), (dict(images=-1), "images"), (dict(n_mels=0), "n_mels"),
                     (dict(advance=2), "advance")):
        assert _draw(L, **kw) == INVALID, kw
        assert word.encode() in L.dmel_last_error(), (kw, L.dmel_last_error())
    for kw, word in ((dict(s=None), "s must"), (dict(y=None), "y must"), (dict(y=C.c_void_p(72)), "y must be a 16-byte aligned"),
                     (dict(s=C.c_void_p(66)), "s must"), (dict(stripes=None), "stripes"), (dict(n_time=8, n_freq=1), "n_time + n_freq <= 8"),
                     (dict(rows=12), "rows must be a multiple of rows_per_clip"), (dict(rows_per_clip=12, rows=24), "rows_per_clip must be a positive multiple of n_mels"),
                     (dict(elem_bf16=2), "elem_bf16"), (dict(T=-1), "T out of range")):
        assert _apply(L, **kw) == INVALID, kw
        assert word.encode() in L.dmel_last_error(), (kw, L.dmel_last_error())
    assert _apply(L, s=C.c_void_p(66), elem_bf16=1, rows=0) == 0                  # a bf16 input at a 2-byte offset is fine; nothing to do
    # nothing to do is a success and launches nothing (so it needs no device either)
    assert _draw(L, images=0) == 0 and _draw(L, T=0) == 0 and _draw(L, n_time=0, n_freq=0, stripes=None) == 0
    assert _apply(L, rows=0) == 0 and _apply(L, T=0) == 0
    if not torch.cuda.is_available():                                             # loud without a device (never run with one: the pointers are not memory)
        assert _draw(L) == capi.DMEL_ERR_NO_DEVICE and b"dmel_specmask_draw" in L.dmel_last_error()
        assert _apply(L) == capi.DMEL_ERR_NO_DEVICE and b"dmel_specmask_apply" in L.dmel_last_error()
