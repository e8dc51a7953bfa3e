"""AttentivePool without a GPU: the case list of tests/attnpool_cases.py is the one the GPU tests need and cannot pass vacuously; the fp32
torch restatement stays within the bounds the GPU tests hold the kernels to, and the restatement with the softmax over all T frames (the
defect the stage removes) does not; hand-made rows worked by hand; zero logits give StatsPool's mean and std; dmel_amd.AttentivePool and
nets.MelAttnPoolNet construct and refuse on the CPU; the two C entry points are exported, check their arguments on the host and are loud
without a device."""
import ctypes as C
import math
import os

import pytest
import torch

import attnpool_cases as P
import statspool_cases as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_attnpool_forward", "dmel_attnpool_backward")
IDS = [P.case_id(c) for c in P.CASES]
SHORT = [c for c in P.CASES if P.pad_fraction(c) >= 0.1]          # a clip with at least a tenth of its frames padding


def test_case_list_is_what_the_issue_asks_for():
    assert P.SHAPES is SP.SHAPES and P.pool is SP.pool
    assert len(P.CASES) == len(IDS) == len(set(IDS)) == 2 * 15 + 4 * 4 + 1 == 47
    for si, shape in enumerate(P.SHAPES):
        R = shape[1] * shape[2]
        mine = [(c["which"], c["form"], c["A"], c["Tc"] is None) for c in P.CASES if c["shape"] == shape]
        want = [(3, "shared", 1, True), (3, "shared", 1, False)]
        if si % 4 == 0:                                            # (at (1, 1, 1, 1) one attention per band is A = 1 again: the case is kept)
            want += [(1, "shared", 1, False), (2, "shared", 1, False), (3, "band", R, False), (3, "band", R, True)]
        if shape == (2, 3, 5, 40):
            want += [(3, "channel", 3, False)]
        assert mine == want, (shape, mine)
    assert {c["kind"] for c in P.CASES} == {"log", "linear"} and abs(sum(c["kind"] == "log" for c in P.CASES) * 2 - len(P.CASES)) <= 1
    for c in P.CASES:
        T, p = c["shape"][3], P.pool(c["shape"][3])
        assert (c["shape"][1] * c["shape"][2]) % c["A"] == 0
        if c["Tc"] is not None:
            assert c["Tc"] == [min(max(p[(c["index"] + b) % 8], 1), T) for b in range(c["shape"][0])]


def test_the_cases_cannot_pass_vacuously():
    """the count of cases with a short clip (found here, fixed here); every case carries a constant row, and every case with two valid
    frames somewhere one -inf logit on a valid frame next to finite ones, with weight exactly 0 and zero gradients there"""
    print(f"{len(SHORT)} of {len(P.CASES)} cases have a clip with at least a tenth of its frames padding")
    assert len(SHORT) == 17 and len(SHORT) >= 10
    planted = 0
    for c in P.CASES:
        s, a, g, ref, _ = P.case_reference(c["index"])
        B, Cc, M, T = c["shape"]
        rows, Tc, k = s.reshape(-1, T), P.lengths_of(c), c["const"]
        tc = Tc[k // (Cc * M)]
        assert bool((rows[k, :tc] == rows[k, 0]).all()) and float(rows[k, 0] * 64.0) == round(float(rows[k, 0] * 64.0))
        assert ref["stats"][k].tolist() == [float(rows[k, 0]), 0.0]                  # exact in the reference: mu == c, var == 0
        assert (c["ninf"] is not None) == any(t >= 2 for t in Tc)
        assert bool(torch.isfinite(a).sum() == a.numel() - (c["ninf"] is not None))
        if c["ninf"] is not None:
            b, r, t = c["ninf"]
            planted += 1
            assert t < Tc[b] and float(a[b, r, t]) == float("-inf") and float(ref["w"][b, r, t]) == 0.0
            assert float(ref["da"][b, r, t]) == 0.0 and float(ref["da_scale"][b, r, t]) == 0.0
            group = Cc * M // c["A"]
            assert not bool(ref["ds"].reshape(B, c["A"], group, T)[b, r, :, t].any())
        assert bool(torch.isfinite(ref["y"]).all()) and bool(torch.isfinite(ref["ds"]).all()) and bool(torch.isfinite(ref["da"]).all())
        valid = P.valid_mask(c["shape"], c["Tc"])
        assert not bool(ref["ds"][~valid.expand(c["shape"])].any()) and not bool(ref["da"][~valid[:, 0].expand(B, c["A"], T)].any())
    assert planted == 39                                           # all but the six cases of (1, 1, 1, 1) and two single clips of length 1


def test_restatement_on_hand_made_rows():
    """Tc = 3 of T = 5, s = 1 2 6 (| 100 100), logits 0 0 ln 2 (| 9 9): weights 1/4 1/4 1/2, mean 3.75, variance 5.1875
    (= 1/4 + 1 + 18 - 3.75^2); with eps = 1.0625 sd = 2.5, and for g = (3, 2), d = -2.75 -1.75 2.25:
    ds = w (3 + 0.8 d) = 0.2 0.4 2.4,  da = w (3 d + 0.4 (d^2 - 5.1875)) = -1.825 -1.525 3.35 (they add up to 0)"""
    s = torch.tensor([1.0, 2.0, 6.0, 100.0, 100.0], dtype=torch.float64).reshape(1, 1, 1, 5).requires_grad_(True)
    a = torch.tensor([0.0, 0.0, math.log(2.0), 9.0, 9.0], dtype=torch.float64).reshape(1, 1, 5).requires_grad_(True)
    y, mu, var = P.forward(s, a, [3], 3, eps=1.0625)
    assert y.shape == (1, 2, 1)
    assert y.reshape(-1).tolist() == pytest.approx([3.75, 2.5], abs=1e-14) and float(var.detach()) == pytest.approx(5.1875, abs=1e-14)
    w, m, Z = P.weights(a.detach(), [3])
    assert w.reshape(-1).tolist() == pytest.approx([0.25, 0.25, 0.5, 0.0, 0.0], abs=1e-15) and float(m) == math.log(2.0) and float(Z) == pytest.approx(2.0)
    g = torch.tensor([3.0, 2.0], dtype=torch.float64).reshape(1, 2, 1)
    ds, da = torch.autograd.grad(y, [s, a], g)
    assert ds.reshape(-1).tolist() == pytest.approx([0.2, 0.4, 2.4, 0.0, 0.0], abs=1e-14)
    assert da.reshape(-1).tolist() == pytest.approx([-1.825, -1.525, 3.35, 0.0, 0.0], abs=1e-14)
    wrong, _, _ = P.forward(s.detach(), a.detach(), [3], 3, eps=1.0625, over_all_T=True)
    assert float(wrong[0, 0, 0]) > 99.0                            # e^9 against 1, 1, 2: the pad frames take the weight
    assert P.forward(s.detach(), a.detach(), None, 1)[0].shape == (1, 1, 1) and P.forward(s.detach(), a.detach(), [2], 2)[0].shape == (1, 1, 1)
    ref = P.reference(s.detach().float(), a.detach().float(), torch.tensor([3.0, -2.0]).reshape(1, 2, 1), [3], 3, eps=1.0625)
    assert ref["scale"]["mean"].reshape(-1).tolist() == pytest.approx([3.75]) and ref["scale"]["std"].reshape(-1).tolist() == pytest.approx([2.5])
    d = (-2.75, -1.75, 2.25)
    assert ref["ds_scale"].reshape(-1).tolist() == pytest.approx([wt * (3.0 + 0.8 * abs(v)) for wt, v in zip((0.25, 0.25, 0.5), d)] + [0.0, 0.0], rel=1e-6)
    assert ref["da_scale"].reshape(-1).tolist() == pytest.approx([wt * (3.0 * abs(v) + 0.4 * (v * v + 5.1875)) for wt, v in zip((0.25, 0.25, 0.5), d)] + [0.0, 0.0], rel=1e-6)
    assert ref["stats"].reshape(-1).tolist() == pytest.approx([3.75, 5.1875], rel=1e-6) and ref["norm"].reshape(-1).tolist() == pytest.approx([math.log(2.0), 2.0], rel=1e-6)


@pytest.mark.parametrize("c", [c for c in SP.CASES if c["which"] == 7][::3], ids=[SP.case_id(c) for c in SP.CASES if c["which"] == 7][::3])
def test_zero_logits_give_the_statistics_of_statspool(c):
    """uniform weights: the mean and the std of tests/statspool_cases.py's restatement, to 1e-15 (relative) in fp64, for A = 1 and A = C M"""
    s, _, _, _ = SP.case_reference(c["index"])
    B, Cc, M, T = c["shape"]
    want, _ = SP.forward(s.double(), c["Tc"], 3)
    for A in sorted({1, Cc * M}):
        got, _, _ = P.forward(s.double(), torch.zeros(B, A, T, dtype=torch.float64), c["Tc"], 3)
        assert float(((got - want).abs() / want.abs().clamp_min(1.0)).max()) <= 1e-15


WORST = {}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_fp32_restatement_stays_within_the_bounds(c):
    """every element of mean, std, ds and da of the fp32 torch restatement against the fp64 one, in units of its scale: within 1e-4, the cap
    of the bounds the GPU tests take from these very errors"""
    s, a, g, ref, r32 = P.case_reference(c["index"])
    b, w = P.bounds(r32, ref, c)
    assert set(w) == {k for k in P.selected(c["which"])} | {"ds", "da"}
    for k, v in w.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= b[k] <= 1e-4, (k, v, b)


def test_worst_fp32_ratios_are_printed():
    print("worst error of the fp32 restatement in units of the scales over the cases:", {k: f"{v:.3e}" for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("c", SHORT, ids=[P.case_id(c) for c in SHORT])
def test_softmax_over_all_T_fails_the_mean_bound_where_a_clip_is_short(c):
    s, a, g, ref, r32 = P.case_reference(c["index"])
    b, _ = P.bounds(r32, ref, c)
    wrong, _, _ = P.forward(s.double(), a.double(), c["Tc"], c["which"], over_all_T=True)
    w = P.errors(wrong, None, None, ref, c, exact_zeros=False)
    k = "mean" if c["which"] & 1 else "std"                       # (the one case that selects the std alone is held to the std's bound)
    assert w[k] > b[k], (k, w[k], b[k])


# ---- the module on the CPU ------------------------------------------------------------------------------------------------------------
def test_constructor_canonical_order_and_refusals():
    import dmel_amd
    assert "AttentivePool" in dmel_amd.__all__ and "attnpool" in dmel_amd.__all__ and dmel_amd.attnpool.AttentivePool is dmel_amd.AttentivePool
    m = dmel_amd.AttentivePool()
    assert (m.stats, m.eps, m.which, m.groups) == (("mean", "std"), 1e-5, 3, 2)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    for given, want, which in ((("std", "mean"), ("mean", "std"), 3), (["std"], ("std",), 2), ("mean", ("mean",), 1)):
        m = dmel_amd.AttentivePool(given)
        assert (m.stats, m.which, m.groups) == (want, which, len(want)), given
    assert "stats=('mean', 'std')" in repr(dmel_amd.AttentivePool(("std", "mean"), eps=1e-3)) and "eps=0.001" in repr(dmel_amd.AttentivePool(eps=1e-3))
    for kw in (dict(stats=()), dict(stats=("mean", "mean")), dict(stats=("mean", "max")), dict(stats=("Mean",)), dict(stats=(1,)), dict(stats=None),
               dict(stats=3), dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps="1e-5"), dict(eps=True)):
        with pytest.raises(ValueError, match="AttentivePool"):
            dmel_amd.AttentivePool(**kw)
    from dmel_amd import capi
    assert (capi.ATTNPOOL_MEAN, capi.ATTNPOOL_STD) == (1, 2)


def test_cpu_tensors_dtypes_shapes_and_the_empty_tensor():
    import dmel_amd
    m = dmel_amd.AttentivePool()
    s, a = torch.rand(2, 1, 4, 6), torch.rand(2, 6)
    for mod in (m.train(), m.eval()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(s, a)
    for logits in (torch.rand(2, 2, 6), torch.rand(2, 4, 6), torch.rand(2, 1, 4, 6)):
        with pytest.raises(RuntimeError, match="AttentivePool.*no CPU fallback"):
            m(s, logits)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(s[:, 0], a, torch.tensor([6, 3]))
    for dt in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match="AttentivePool.*" + str(dt).replace(".", r"\.")):
            m(s.to(dt), a)
        with pytest.raises(RuntimeError, match="AttentivePool.*logits.*" + str(dt).replace(".", r"\.")):
            m(s, a.to(dt))
    with pytest.raises(ValueError, match=r"AttentivePool.*\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m(torch.rand(4, 6), a)
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m([1.0], a)
    for logits in (torch.rand(2, 5), torch.rand(3, 6), torch.rand(2, 3, 6), torch.rand(2, 0, 6), torch.rand(2, 8, 6), torch.rand(2, 4, 1, 6), torch.rand(6), [0.0]):
        with pytest.raises(ValueError, match=r"AttentivePool: logits must .*\(2, 6\), \(2, A, 6\) with A dividing C n_mels = 4, or \(2, 1, 4, 6\)"):
            m(s, logits)
    with pytest.raises(TypeError, match="1-D integer tensor"):
        m(s, a, [6, 3])
    with pytest.raises(TypeError, match="int32 or int64"):
        m(s, a, torch.tensor([6.0, 3.0]))
    with pytest.raises(ValueError, match=r"AttentivePool.*shape \(2,\)"):
        m(s, a, torch.tensor([6, 3, 1]))
    with pytest.raises(ValueError, match="AttentivePool.*no frames"):
        m(torch.empty(2, 3, 4, 0), torch.empty(2, 0))
    # a tensor without rows comes back with the output's shape and launches nothing (so it needs no device)
    assert m(torch.empty(0, 4, 6), torch.empty(0, 6)).shape == (0, 2, 4)
    assert dmel_amd.AttentivePool(("std",))(torch.empty(2, 2, 0, 5), torch.empty(2, 1, 5)).shape == (2, 2, 0)
    assert m(torch.empty(0, 2, 4, 5), torch.empty(0, 2, 4, 5), torch.empty(0, dtype=torch.int64)).shape == (0, 4, 4)


def test_mel_attn_pool_net_constructs_on_the_cpu():
    from dmel_amd import nets
    import dmel_amd
    net = nets.MelAttnPoolNet(5, 128.0, "cpu", 40, 16000, 4000, hop_length=64)
    assert isinstance(net.pool, dmel_amd.AttentivePool) and net.pool.stats == ("mean", "std") and net.attention == "shared"
    assert (net.fc.in_features, net.fc.out_features) == (80, 5) and net.normalization is None and net.augmentation is None
    assert net.spectrogram_layer.log and net.spectrogram_layer.optimized
    assert [n for n, _ in net.named_parameters()] == ["spectrogram_layer.lambd", "attention_fc1.weight", "attention_fc1.bias", "attention_fc2.weight",
                                                      "attention_fc2.bias", "fc.weight", "fc.bias"]
    assert tuple(net.attention_fc1.weight.shape) == (32, 40, 1) and tuple(net.attention_fc2.weight.shape) == (1, 32, 1)
    band = nets.MelAttnPoolNet(3, 128.0, "cpu", 40, 16000, 4000, hop_length=64, energy_normalize=False, stats=("std",), attention="band", attention_hidden=8)
    assert band.fc.in_features == 40 and not band.spectrogram_layer.log and band.pool.stats == ("std",)
    assert tuple(band.attention_fc1.weight.shape) == (8, 40, 1) and tuple(band.attention_fc2.weight.shape) == (40, 8, 1)
    assert len(nets.make_optimizer(net, 1e-3, 1.0).param_groups) == 7
    for bad in ("channel", "", None, 1):
        with pytest.raises(ValueError, match="MelAttnPoolNet: attention"):
            nets.MelAttnPoolNet(5, 128.0, "cpu", 40, 16000, 4000, hop_length=64, attention=bad)


# ---- the C entry points on the host -----------------------------------------------------------------------------------------------------
def test_symbols_listed_exported_and_named():
    from dmel_amd import capi
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert callable(capi.attnpool_forward) and callable(capi.attnpool_backward)
    assert L.dmel_abi_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NAMES)
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    assert all(f"dmel_status {name}(" in header for name in NAMES)


def _forward(L, **kw):
    args = dict(s=C.c_void_p(64), a=C.c_void_p(64), rows=16, rows_per_clip=8, logit_rows=2, T=10, lengths=None, which=3, eps=1e-5, y=C.c_void_p(64),
                stats=C.c_void_p(64), norm=C.c_void_p(64), stream=None)
    args.update(kw)
    return L.dmel_attnpool_forward(*args.values())


def _backward(L, **kw):
    args = dict(g=C.c_void_p(64), s=C.c_void_p(64), a=C.c_void_p(64), stats=C.c_void_p(64), norm=C.c_void_p(64), rows=16, rows_per_clip=8, logit_rows=2,
                T=10, lengths=None, which=3, eps=1e-5, ds=C.c_void_p(64), da=C.c_void_p(64), stream=None)
    args.update(kw)
    return L.dmel_attnpool_backward(*args.values())


def test_argument_checks_need_no_device_and_name_the_argument():
    """(the pointers are never dereferenced: every refusal comes before the first launch, and this machine has no device)"""
    from dmel_amd import capi
    L = capi.load()
    INVALID = 1
    nan = float("nan")
    shared = ((dict(rows=12), "rows_per_clip must be positive and divide rows"), (dict(rows_per_clip=0), "rows_per_clip"),
              (dict(logit_rows=3), "logit_rows_per_clip must be positive and divide rows_per_clip"), (dict(logit_rows=0), "logit_rows_per_clip"),
              (dict(logit_rows=16), "logit_rows_per_clip"), (dict(which=0), "which must lie in 1 ... 3"), (dict(which=4), "which"), (dict(which=-1), "which"),
              (dict(rows=-8), "rows"), (dict(T=-1), "n_time"), (dict(lengths=C.c_void_p(66)), "frame_lengths"),
              (dict(eps=0.0), "eps must be finite and > 0"), (dict(eps=-1.0), "eps"), (dict(eps=nan), "eps"), (dict(eps=float("inf"), which=2), "eps"),
              (dict(s=None), "s must"), (dict(s=C.c_void_p(66)), "s must"), (dict(a=None), "a must"), (dict(a=C.c_void_p(66)), "a must"),
              (dict(stats=C.c_void_p(72)), "stats must be a 16-byte aligned"), (dict(norm=C.c_void_p(72)), "norm must be a 16-byte aligned"),
              (dict(stats=None), "stats and norm must both"), (dict(norm=None), "stats and norm must both"))
    fwd = shared + ((dict(y=None), "y must"), (dict(y=C.c_void_p(66)), "y must"))
    bwd = shared + ((dict(g=None), "g must"), (dict(g=C.c_void_p(66)), "g must"), (dict(ds=None), "ds must"), (dict(ds=C.c_void_p(65)), "ds must"),
                    (dict(da=None), "da must"), (dict(da=C.c_void_p(67)), "da must"), (dict(stats=None, norm=None), "stats and norm the forward wrote"))
    for call, name, table in ((_forward, NAMES[0], fwd), (_backward, NAMES[1], bwd)):
        for kw, word in table:
            assert call(L, **kw) == INVALID, (name, kw)
            msg = L.dmel_last_error()
            assert word.encode() in msg and name.encode() in msg, (kw, msg)
        assert call(L, rows=0) == 0 and call(L, T=0) == 0                     # nothing to do is a success and launches nothing
        assert call(L, rows=0, eps=0.0, which=1) == 0 and call(L, rows=0, eps=nan, which=1) == 0      # eps is asked for with std only
        assert call(L, rows=0, s=C.c_void_p(68), a=C.c_void_p(68)) == 0       # s and a need their element's alignment only
        assert call(L, rows=0, logit_rows=1) == 0 and call(L, rows=0, logit_rows=8) == 0
    assert _forward(L, rows=0, stats=None, norm=None) == 0 and _forward(L, rows=0, y=C.c_void_p(68)) == 0
    assert _backward(L, rows=0, g=C.c_void_p(68), ds=C.c_void_p(68), da=C.c_void_p(68)) == 0
    if not torch.cuda.is_available():                                       # loud without a device (never run with one: the pointers are not memory)
        for call, name in ((_forward, NAMES[0]), (_backward, NAMES[1])):
            assert call(L) == capi.DMEL_ERR_NO_DEVICE and name.encode() in L.dmel_last_error()
