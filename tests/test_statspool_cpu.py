"""StatsPool without a GPU: the case list of tests/statspool_cases.py is the one the GPU tests need and cannot pass vacuously; the fp32 torch
restatement stays within the bounds the GPU tests hold the kernels to, and the restatement over all T frames (the defect the stage removes)
does not; the order of the maximum on hand-written rows; dmel_amd.StatsPool constructs, orders its statistics and refuses on the CPU; the
two C entry points are exported, check their arguments on the host and are loud without a device."""
import ctypes as C
import os

import pytest
import torch

import statspool_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_statspool_forward", "dmel_statspool_backward")
IDS = [P.case_id(c) for c in P.CASES]
SHORT = [c for c in P.CASES if P.pad_fraction(c) >= 0.1]          # a clip with at least a tenth of its frames padding


def test_case_list_is_what_the_issue_asks_for():
    assert P.SHAPES == [(1, 1, 1, 1), (3, 1, 5, 2), (2, 1, 2, 3), (2, 1, 2, 5), (2, 1, 7, 31), (4, 1, 4, 32), (2, 1, 3, 33), (2, 1, 3, 63),
                        (1, 1, 6, 64), (2, 1, 3, 65), (1, 1, 2, 130), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5), (4, 1, 128, 32)]
    assert len(P.CASES) == len(IDS) == len(set(IDS)) == 2 * 15 + 4 * 4
    for si, shape in enumerate(P.SHAPES):
        mine = [c for c in P.CASES if c["shape"] == shape]
        assert {c["Tc"] is None for c in mine if c["which"] == 7} == {True, False}, shape
        assert sorted(c["which"] for c in mine if c["which"] != 7) == ([1, 2, 4, 5] if si % 4 == 0 else []), shape
    assert {c["kind"] for c in P.CASES} == {"log", "linear"} and abs(sum(c["kind"] == "log" for c in P.CASES) * 2 - len(P.CASES)) <= 1
    for c in P.CASES:
        T, p = c["shape"][3], P.pool(c["shape"][3])
        assert p == [T, 1, 2, 63, 64, 65, T - 1, T // 2] and len(p) == P.POOL_SIZE
        if c["Tc"] is not None:
            assert c["Tc"] == [min(max(p[(c["index"] + b) % 8], 1), T) for b in range(c["shape"][0])]


def test_the_cases_cannot_pass_vacuously():
    """the count of cases with a short clip (found here, fixed here); every case carries a constant row, every case with three rows a tie
    row and a row whose valid maximum is negative, and the short cases hold +0.0 and 5.0 behind that row's valid frames"""
    print(f"{len(SHORT)} of {len(P.CASES)} cases have a clip with at least a tenth of its frames padding")
    assert len(SHORT) == 18 and len(SHORT) >= 10
    for c in P.CASES:
        s, g, ref, _ = P.case_reference(c["index"])
        B, Cc, M, T = c["shape"]
        rows, Tc, r = s.reshape(-1, T), P.lengths_of(c), c["rows"]
        am = ref["am"].reshape(-1)
        tc = Tc[r["const"] // (Cc * M)]
        assert bool((rows[r["const"], :tc] == rows[r["const"], 0]).all()) and int(am[r["const"]]) == 0
        assert (r["neg"] is not None and r["tie"] is not None) == (B * Cc * M >= 2)
        if r["neg"] is not None:
            tc = Tc[r["neg"] // (Cc * M)]
            assert float(rows[r["neg"], :tc].max()) < 0
            if tc < T:
                assert float(rows[r["neg"], tc]) == 0.0 and (T - tc < 2 or float(rows[r["neg"], tc + 1]) == 5.0)
        if r["tie"] is not None and Tc[r["tie"] // (Cc * M)] >= 2:
            tc = Tc[r["tie"] // (Cc * M)]
            v = rows[r["tie"], :tc]
            assert int((v == v.max()).sum()) >= 2 and int(am[r["tie"]]) == int((v == v.max()).nonzero()[0])
    assert all(c["rows"]["neg"] is not None and P.lengths_of(c)[c["rows"]["neg"] // (c["shape"][1] * c["shape"][2])] < c["shape"][3] for c in SHORT)


def test_restatement_on_hand_made_rows():
    """Tc = 3 of T = 5, s = 1 2 6 (| 100 100): mean 3, biased variance 14 / 3, max 6 at frame 2; over all T frames the mean is 41.8"""
    s = torch.tensor([1.0, 2.0, 6.0, 100.0, 100.0], dtype=torch.float64).reshape(1, 1, 1, 5).requires_grad_(True)
    y, am = P.forward(s, [3], 7, eps=0.25)
    assert y.shape == (1, 3, 1) and am.tolist() == [[[2]]]
    assert y.reshape(-1).tolist() == pytest.approx([3.0, (14.0 / 3.0 + 0.25) ** 0.5, 6.0], abs=1e-15)
    sd = float(y[0, 1, 0].detach())
    (ds,) = torch.autograd.grad(y, [s], torch.tensor([3.0, 2.0, 5.0], dtype=torch.float64).reshape(1, 3, 1))
    want = [1.0 + 2.0 * (v - 3.0) / (3.0 * sd) + (5.0 if t == 2 else 0.0) for t, v in enumerate([1.0, 2.0, 6.0])] + [0.0, 0.0]
    assert ds.reshape(-1).tolist() == pytest.approx(want, abs=1e-14)
    wrong, _ = P.forward(s.detach(), [3], 7, eps=0.25, over_all_T=True)
    assert float(wrong[0, 0, 0]) == pytest.approx(41.8) and float(wrong[0, 2, 0]) == 100.0
    assert P.forward(s.detach(), None, 5)[0].shape == (1, 2, 1) and P.forward(s.detach(), [2], 2)[0].shape == (1, 1, 1)
    ref = P.reference(s.detach().float(), torch.tensor([3.0, -2.0, 5.0]).reshape(1, 3, 1), [3], 7, eps=0.25)
    assert ref["scale"]["mean"].reshape(-1).tolist() == pytest.approx([3.0]) and ref["scale"]["std"].reshape(-1).tolist() == pytest.approx([sd])
    assert ref["ds_scale"].reshape(-1).tolist() == pytest.approx([1.0 + 2.0 * abs(v - 3.0) / (3.0 * sd) + (5.0 if v == 6.0 else 0.0) for v in (1.0, 2.0, 6.0)] + [0.0, 0.0])


def test_the_order_of_the_maximum_on_hand_written_rows():
    nan, inf = float("nan"), float("inf")
    rows = [([1.0, 3.0, 3.0, 2.0], 1),            # a tie: the lower t
            ([-2.0, -1.0, -1.0], 1),              # among negatives too
            ([-0.0, 0.0, -1.0], 0), ([0.0, -0.0, -1.0], 0),   # -0.0 and +0.0 tie: the lower t, whichever sign it carries
            ([1.0, nan, 5.0, nan], 1),            # a NaN beats a non-NaN; two NaNs: the lower t
            ([inf, nan], 1), ([nan, inf], 0), ([-inf, -inf], 0), ([-inf, 4.0, inf, inf], 2), ([7.0], 0)]
    for values, want in rows:
        x = torch.tensor(values)
        assert int(P.argmax_by_the_order(x)) == want, values
        y, am = P.forward(x.reshape(1, 1, 1, -1), None, 4)
        assert int(am) == want and y.view(torch.int32).item() == x.view(torch.int32)[want].item(), values      # moved as a word
    # the order is associative and commutative: every split of a row into two halves, reduced separately, gives the row's winner
    x = torch.tensor([2.0, nan, 2.0, -0.0, 0.0, nan, 2.0])
    for cut in range(1, 7):
        a, b = int(P.argmax_by_the_order(x[:cut])), cut + int(P.argmax_by_the_order(x[cut:]))
        assert [a, b][int(P.argmax_by_the_order(x[[a, b]]))] == int(P.argmax_by_the_order(x)) == 1, cut


WORST = {}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_fp32_restatement_stays_within_the_bounds(c):
    """every element of mean, std and ds of the fp32 torch restatement against the fp64 one, in units of its scale: within 1e-4, the cap
    of the bounds the GPU tests take from these very errors"""
    s, g, ref, r32 = P.case_reference(c["index"])
    b, w = P.bounds(r32, ref, c)
    for k, v in w.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= b[k] <= 1e-4, (k, v, b)
    C_ = c["shape"][1]
    if c["which"] & 4:                                            # the maximum and its index do not depend on the precision
        assert torch.equal(P.split(r32["y"], c["which"], C_)["max"].double(), P.split(ref["y"], c["which"], C_)["max"])
    assert not bool(ref["ds"][~P.valid_mask(c["shape"], c["Tc"]).expand(c["shape"])].any())


def test_worst_fp32_ratios_are_printed():
    print("worst error of the fp32 restatement in units of the scales over the cases:", {k: f"{v:.3e}" for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", SHORT, ids=[P.case_id(c) for c in SHORT])
def test_statistics_over_all_T_fail_the_bounds_where_a_clip_is_short(c):
    s, g, ref, r32 = P.case_reference(c["index"])
    b, _ = P.bounds(r32, ref, c)
    wrong, _ = P.forward(s.double(), c["Tc"], c["which"], over_all_T=True)
    w = P.errors(wrong, None, ref, c, exact_zeros=False)
    for k in ("mean", "std"):
        if k in w:
            assert w[k] > b[k], (k, w[k], b[k])
    if c["which"] & 4:                                            # the +0.0 and the 5.0 behind the row whose valid maximum is negative
        C_ = c["shape"][1]
        assert not torch.equal(P.split(wrong, c["which"], C_)["max"], P.split(ref["y"], c["which"], C_)["max"])


# ---- the module on the CPU ------------------------------------------------------------------------------------------------------------
def test_constructor_canonical_order_and_refusals():
    import dmel_amd
    assert "StatsPool" in dmel_amd.__all__ and "statspool" in dmel_amd.__all__ and dmel_amd.statspool.StatsPool is dmel_amd.StatsPool
    m = dmel_amd.StatsPool()
    assert (m.stats, m.eps, m.which, m.groups) == (("mean", "std", "max"), 1e-5, 7, 3)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    for given, want, which in ((("max", "mean"), ("mean", "max"), 5), (["std"], ("std",), 2), (("max", "std", "mean"), ("mean", "std", "max"), 7),
                               ("max", ("max",), 4), (("std", "mean"), ("mean", "std"), 3)):
        m = dmel_amd.StatsPool(given)
        assert (m.stats, m.which, m.groups) == (want, which, len(want)), given
    assert "stats=('mean', 'max')" in repr(dmel_amd.StatsPool(("max", "mean"), eps=1e-3)) and "eps=0.001" in repr(dmel_amd.StatsPool(eps=1e-3))
    for kw in (dict(stats=()), dict(stats=("mean", "mean")), dict(stats=("mean", "median")), dict(stats=("Mean",)), dict(stats=(1,)), dict(stats=None),
               dict(stats=7), dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps="1e-5"), dict(eps=True)):
        with pytest.raises(ValueError, match="StatsPool"):
            dmel_amd.StatsPool(**kw)


def test_cpu_tensors_dtypes_shapes_and_the_empty_tensor():
    import dmel_amd
    m = dmel_amd.StatsPool()
    s = torch.rand(2, 1, 4, 6)
    for mod in (m.train(), m.eval()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(s[:, 0], torch.tensor([6, 3]))
    for dt in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match=str(dt).replace(".", r"\.")):
            m(s.to(dt))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m(torch.rand(4, 6))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m([1.0])
    with pytest.raises(TypeError, match="1-D integer tensor"):
        m(s, [6, 3])
    with pytest.raises(TypeError, match="int32 or int64"):
        m(s, torch.tensor([6.0, 3.0]))
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        m(s, torch.tensor([6, 3, 1]))
    with pytest.raises(ValueError, match="no frames"):
        m(torch.empty(2, 3, 4, 0))
    # a tensor without rows comes back with the output's shape and launches nothing (so it needs no device)
    assert m(torch.empty(0, 4, 6)).shape == (0, 3, 4) and dmel_amd.StatsPool(("max",))(torch.empty(2, 2, 0, 5)).shape == (2, 2, 0)
    assert dmel_amd.StatsPool(("mean", "max"))(torch.empty(0, 2, 4, 5), torch.empty(0, dtype=torch.int64)).shape == (0, 4, 4)


def test_mel_pool_net_constructs_on_the_cpu():
    from dmel_amd import nets
    import dmel_amd
    net = nets.MelPoolNet(5, 128.0, "cpu", 40, 16000, 4000, hop_length=64)
    assert isinstance(net.pool, dmel_amd.StatsPool) and net.pool.stats == ("mean", "std", "max")
    assert (net.fc.in_features, net.fc.out_features) == (120, 5) and net.normalization is None and net.augmentation is None
    assert net.spectrogram_layer.log and net.spectrogram_layer.optimized
    assert [n for n, _ in net.named_parameters()] == ["spectrogram_layer.lambd", "fc.weight", "fc.bias"]
    small = nets.MelPoolNet(3, 128.0, "cpu", 40, 16000, 4000, hop_length=64, energy_normalize=False, stats=("max", "mean"))
    assert small.fc.in_features == 80 and not small.spectrogram_layer.log and small.pool.stats == ("mean", "max")
    assert len(nets.make_optimizer(net, 1e-3, 1.0).param_groups) == 3


# ---- the C entry points on the host -----------------------------------------------------------------------------------------------------
def test_symbols_listed_exported_and_named():
    from dmel_amd import capi
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert L.dmel_abi_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NAMES)
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    assert all(f"dmel_status {name}(" in header for name in NAMES)


def _forward(L, **kw):
    a = dict(s=C.c_void_p(64), rows=16, rows_per_clip=8, T=10, lengths=None, which=7, eps=1e-5, y=C.c_void_p(64), stats=C.c_void_p(64),
             argmax=C.c_void_p(64), stream=None)
    a.update(kw)
    return L.dmel_statspool_forward(*a.values())


def _backward(L, **kw):
    a = dict(g=C.c_void_p(64), s=C.c_void_p(64), stats=C.c_void_p(64), argmax=C.c_void_p(64), rows=16, rows_per_clip=8, T=10, lengths=None,
             which=7, ds=C.c_void_p(64), stream=None)
    a.update(kw)
    return L.dmel_statspool_backward(*a.values())


def test_argument_checks_need_no_device_and_name_the_argument():
    """(the pointers are never dereferenced: every refusal comes before the first launch, and this machine has no device)"""
    from dmel_amd import capi
    L = capi.load()
    INVALID = 1
    nan = float("nan")
    shared = ((dict(rows=12), "rows_per_clip must be positive and divide rows"), (dict(rows_per_clip=0), "rows_per_clip"), (dict(which=0), "which must lie in 1 ... 7"),
              (dict(which=8), "which"), (dict(which=-1), "which"), (dict(rows=-8), "rows"), (dict(T=-1), "n_time"),
              (dict(lengths=C.c_void_p(66)), "frame_lengths"), (dict(stats=C.c_void_p(72)), "stats must be a 16-byte aligned"))
    fwd = shared + ((dict(s=None), "s must"), (dict(s=C.c_void_p(66)), "s must"), (dict(y=None), "y must"), (dict(eps=0.0), "eps must be finite and > 0"),
                    (dict(eps=-1.0), "eps"), (dict(eps=nan), "eps"), (dict(eps=nan, which=3), "eps"), (dict(eps=0.0, which=2), "eps"))
    bwd = shared + ((dict(g=None), "g must"), (dict(g=C.c_void_p(66)), "g must"), (dict(ds=None), "ds must"), (dict(s=None), "std is selected"),
                    (dict(stats=None), "std is selected"), (dict(s=None, which=2), "std is selected"), (dict(argmax=None), "max is selected"),
                    (dict(argmax=None, which=4), "max is selected"))
    for call, name, table in ((_forward, NAMES[0], fwd), (_backward, NAMES[1], bwd)):
        for kw, word in table:
            assert call(L, **kw) == INVALID, (name, kw)
            msg = L.dmel_last_error()
            assert word.encode() in msg and name.encode() in msg, (kw, msg)
        assert call(L, rows=0) == 0 and call(L, T=0) == 0                     # nothing to do is a success and launches nothing
    # what a statistic that is not selected would need is not asked for
    assert _forward(L, rows=0, eps=0.0, which=5, stats=None, argmax=None) == 0 and _forward(L, rows=0, eps=nan, which=4) == 0
    assert _backward(L, rows=0, s=None, stats=None, which=5) == 0 and _backward(L, rows=0, argmax=None, which=3) == 0
    assert _backward(L, rows=0, s=None, stats=None, argmax=None, which=1) == 0
    # s and g need their element's alignment only
    assert _forward(L, rows=0, s=C.c_void_p(68), y=C.c_void_p(68)) == 0 and _backward(L, rows=0, g=C.c_void_p(68), s=C.c_void_p(68)) == 0
    if not torch.cuda.is_available():                                       # loud without a device (never run with one: the pointers are not memory)
        for call, name in ((_forward, NAMES[0]), (_backward, NAMES[1])):
            assert call(L) == capi.DMEL_ERR_NO_DEVICE and name.encode() in L.dmel_last_error()
