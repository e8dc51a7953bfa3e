"""Deltas without a GPU: the case list of tests/deltas_cases.py is the one the GPU tests need and cannot pass vacuously; the restatement gives
hand-worked values; the fp32 numpy evaluation of the specified arithmetic and the fp32 run of the restatement stay within the bounds the GPU
tests hold the kernels to, and the restatement with its edge at T - 1 (the defect the stage removes) does not; dmel_amd.Deltas constructs,
refuses and handles an empty tensor on the CPU; the two C entry points are exported, check their arguments on the host and are loud without
a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import deltas_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_deltas_forward", "dmel_deltas_backward")
IDS = [D.case_id(c) for c in D.CASES]
SHORT = [c for c in D.CASES if c["Tc"] is not None and any(t < c["shape"][3] for t in c["Tc"])]


def test_case_list_is_what_the_issue_asks_for():
    assert D.SHAPES == [(1, 1, 1, 1), (3, 1, 5, 2), (2, 1, 3, 3), (2, 1, 2, 4), (2, 1, 2, 5), (2, 1, 3, 9), (2, 1, 7, 31), (4, 1, 4, 32), (2, 1, 3, 33),
                        (2, 1, 3, 47), (2, 1, 2, 48), (2, 1, 2, 49), (2, 1, 3, 56), (2, 1, 3, 57), (2, 1, 3, 60), (2, 1, 3, 61), (2, 1, 3, 63),
                        (1, 1, 6, 64), (2, 1, 3, 65), (1, 1, 2, 113), (1, 1, 2, 130), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5), (4, 1, 128, 32)]
    assert len(D.CASES) == len(IDS) == len(set(IDS))
    for si, shape in enumerate(D.SHAPES):
        mine = [c for c in D.CASES if c["shape"] == shape]
        for win in (3, 5, 9):
            assert {c["Tc"] is None for c in mine if c["win_length"] == win and c["order"] == 2 and c["include_static"]} == {True, False}, (shape, win)
        assert any(c["order"] == 1 for c in mine) == any(not c["include_static"] for c in mine) == (si % 4 == 0), shape
    assert {c["kind"] for c in D.CASES} == {"log", "linear"} and abs(sum(c["kind"] == "log" for c in D.CASES) * 2 - len(D.CASES)) <= 1
    for c in D.CASES:
        if c["Tc"] is not None:
            T, p = c["shape"][3], D.pool(c["shape"][3], D.half(c["win_length"]))
            assert len(p) == D.POOL_SIZE
            assert c["Tc"] == [min(max(p[(c["index"] + b) % 11], 1), T) for b in range(c["shape"][0])]
    # the kernel's chunk steps (64 - 4 n: 60, 56, 48 for win_length 3, 5, 9) are among the sizes 48, 56, 60, 64 the shapes straddle
    assert {64 - 4 * D.half(w) for w in D.WIN_LENGTHS} <= {48, 56, 60, 64}


def test_the_cases_cannot_pass_vacuously():
    """every pool entry occurs strictly below T for each win_length; at least a third of the clips with lengths given are shorter than T"""
    for win in D.WIN_LENGTHS:
        seen = set()
        for c in D.CASES:
            if c["win_length"] == win and c["Tc"] is not None:
                T, p = c["shape"][3], D.pool(c["shape"][3], D.half(win))
                seen |= {e for e, t in zip(c["entries"], c["Tc"]) if e != 0 and 1 <= p[e] < T and t == p[e]}
        assert seen == set(range(1, D.POOL_SIZE)), (win, sorted(seen))
        assert any(c["win_length"] == win and c["Tc"] is not None and c["entries"][0] == 0 for c in D.CASES)       # and the full length, given
    clips = [(t, c["shape"][3]) for c in D.CASES if c["Tc"] is not None for t in c["Tc"]]
    short = sum(t < T for t, T in clips)
    print(f"{short} of {len(clips)} clips with lengths given are shorter than T; {len(SHORT)} cases have one")
    assert 3 * short >= len(clips)
    assert len(SHORT) >= 40


def test_restatement_on_a_hand_made_row():
    """win_length 5 (n = 2, denom 10), Tc = 3 of T = 6, x = 1 4 9 (| 100 100 100 behind the clip's end):
         d[0]  = (1 (4 - 1) + 2 (9 - 1)) / 10 = 1.9      d[1] = (1 (9 - 1) + 2 (9 - 1)) / 10 = 2.4      d[2] = (1 (9 - 4) + 2 (9 - 1)) / 10 = 2.1
         dd[0] = (1 (2.4 - 1.9) + 2 (2.1 - 1.9)) / 10 = 0.09     dd[1] = (1 (2.1 - 1.9) + 2 (2.1 - 1.9)) / 10 = 0.06
         dd[2] = (1 (2.1 - 2.4) + 2 (2.1 - 1.9)) / 10 = 0.01
       with the edge at T - 1 = 5 instead, d[2] = (1 (100 - 4) + 2 (100 - 1)) / 10 = 29.4: the defect"""
    s = torch.tensor([1.0, 4.0, 9.0, 100.0, 100.0, 100.0], dtype=torch.float64).reshape(1, 1, 1, 6)
    y = D.forward(s, [3], 5, 2, True)
    assert y.shape == (1, 3, 1, 6) and torch.equal(y[0, 0, 0], s[0, 0, 0])
    assert torch.allclose(y[0, 1, 0], torch.tensor([1.9, 2.4, 2.1, 0.0, 0.0, 0.0], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(y[0, 2, 0], torch.tensor([0.09, 0.06, 0.01, 0.0, 0.0, 0.0], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.equal(y[0, 1:, 0, 3:], torch.zeros(2, 3, dtype=torch.float64))
    d, dd = D.spec_forward(s.numpy().astype(np.float32), [3], 5)
    # (fp32: 7 u and 14 u of the scales, which are at most (1 (9 + 4) + 2 (9 + 1)) / 10 = 3.3 and (1 (3.3 + 3.0) + 2 (3.3 + 2.5)) / 10 = 1.79 here)
    assert np.allclose(d[0, 0, 0], [1.9, 2.4, 2.1, 0, 0, 0], rtol=0, atol=7 * D.U * 3.3)
    assert np.allclose(dd[0, 0, 0], [0.09, 0.06, 0.01, 0, 0, 0], rtol=0, atol=14 * D.U * 1.79)
    wrong = D.forward(s, [3], 5, 2, True, edge_at_T=True)
    assert abs(float(wrong[0, 1, 0, 2]) - 29.4) < 1e-12 and torch.equal(wrong[0, 1:, 0, 3:], torch.zeros(2, 3, dtype=torch.float64))
    assert D.forward(s, [3], 5, 1, False).shape == (1, 1, 1, 6) and D.forward(s, None, 3, 2, False).shape == (1, 2, 1, 6)
    # the scales: |j| on |s|
    assert abs(float(D.forward(s.abs(), [3], 5, 1, False, absolute=True)[0, 0, 0, 0]) - (1 * (4 + 1) + 2 * (9 + 1)) / 10) < 1e-15


WORST = {}


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_fp32_evaluations_stay_within_the_bounds(c):
    """the fp32 numpy evaluation of the specified arithmetic and the fp32 run of the restatement, every element, in units of its scale;
    the backward of the fp32 restatement likewise"""
    s, g, ref = D.case_reference(c["index"])
    b = D.bounds(c["win_length"])
    _, d64, dd64 = D.split(ref["y"], c)
    _, dsc, ddsc = D.split(ref["y_scale"], c)
    d, dd = D.spec_forward(s.numpy(), c["Tc"], c["win_length"], c["order"])
    x = s.clone().requires_grad_(True)
    y32 = D.forward(x, c["Tc"], c["win_length"], c["order"], c["include_static"])
    (ds32,) = torch.autograd.grad(y32, [x], g)
    _, d32, dd32 = D.split(y32.detach(), c)
    ratios = dict(d_spec=D.worst(d, d64, dsc) / D.U, d_torch=D.worst(d32, d64, dsc) / D.U, ds_torch=D.worst(ds32, ref["ds"], ref["ds_scale"]) / D.U)
    if c["order"] == 2:
        ratios.update(dd_spec=D.worst(dd, dd64, ddsc) / D.U, dd_torch=D.worst(dd32, dd64, ddsc) / D.U)
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v * D.U <= b[k.split("_")[0]], (k, v, b)
    pad = ~D.valid_mask(c["shape"], c["Tc"]).expand(c["shape"]).numpy()
    assert not d.view(np.uint32)[pad].any() and not dd.view(np.uint32)[pad].any()


def test_worst_fp32_ratios_are_printed():
    print("worst error in units of u = 2^-24 over the cases:", {k: round(v, 2) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("win", [3, 5, 7, 9])
def test_specified_arithmetic_gives_exact_zeros(win):
    """a constant row (under the log: silence, -23.03), Tc = 1 and a row of zeros give +0.0 bit for bit in both channels"""
    s = np.full((3, 1, 2, 12), np.float32(np.log(1e-10)), dtype=np.float32)
    s[1] = np.random.default_rng(0).standard_normal((1, 2, 12)).astype(np.float32)
    s[2] = 0.0
    d, dd = D.spec_forward(s, [12, 1, 7], win)
    assert not d.view(np.uint32).any() and not dd.view(np.uint32).any()


@pytest.mark.parametrize("c", SHORT, ids=[D.case_id(c) for c in SHORT])
def test_the_edge_at_T_fails_the_bounds_where_a_clip_is_short(c):
    s, g, ref = D.case_reference(c["index"])
    b = D.bounds(c["win_length"])
    wrong = D.forward(s.double(), c["Tc"], c["win_length"], c["order"], c["include_static"], edge_at_T=True)
    _, d64, _ = D.split(ref["y"], c)
    _, dsc, _ = D.split(ref["y_scale"], c)
    _, dw, _ = D.split(wrong, c)
    err = (dw - d64).abs()
    bad = err > b["d"] * dsc
    assert bool(bad.any()), "the shifted edge went unnoticed"
    for bi, tc in enumerate(c["Tc"]):                              # and exactly behind the short clips' ends
        assert bool(bad[bi].any()) == (tc < c["shape"][3]), (bi, tc)


# ---- the module on the CPU ------------------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    import dmel_amd
    assert "Deltas" in dmel_amd.__all__
    m = dmel_amd.Deltas()
    assert (m.win_length, m.order, m.include_static, m.groups) == (5, 2, True, 3)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    assert dmel_amd.Deltas(9, 1, False).groups == 1 and "win_length=9" in repr(dmel_amd.Deltas(9))
    for kw in (dict(win_length=4), dict(win_length=11), dict(win_length=1), dict(win_length=5.5), dict(order=0), dict(order=3), dict(order=1.5),
               dict(include_static=1), dict(win_length=True)):
        with pytest.raises(ValueError, match="Deltas"):
            dmel_amd.Deltas(**kw)


def test_cpu_tensors_dtypes_shapes_and_the_empty_tensor():
    import dmel_amd
    m = dmel_amd.Deltas()
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
    # an empty tensor comes back with the output's shape and launches nothing (so it needs no device)
    assert m(torch.empty(0, 4, 6)).shape == (0, 3, 4, 6) and m(torch.empty(2, 3, 4, 0)).shape == (2, 9, 4, 0)
    assert dmel_amd.Deltas(3, 1, False)(torch.empty(2, 2, 0, 5)).shape == (2, 2, 0, 5)
    assert dmel_amd.Deltas(3, 1)(torch.empty(0, 2, 4, 5), torch.empty(0, dtype=torch.int64)).shape == (0, 4, 4, 5)


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


def _call(L, name, **kw):
    a = dict(s=C.c_void_p(64), rows=16, rows_per_clip=8, T=10, lengths=None, win_length=5, order=2, include_static=1, y=C.c_void_p(64), stream=None)
    a.update(kw)
    return getattr(L, name)(*a.values())


@pytest.mark.parametrize("name,src,dst", [("dmel_deltas_forward", "s", "y"), ("dmel_deltas_backward", "g", "ds")])
def test_argument_checks_need_no_device_and_name_the_argument(name, src, dst):
    """(the pointers are never dereferenced: every refusal comes before the first launch, and this machine has no device)"""
    from dmel_amd import capi
    L = capi.load()
    INVALID = 1
    for kw, word in ((dict(s=None), f"{src} must"), (dict(s=C.c_void_p(66)), f"{src} must"), (dict(y=None), f"{dst} must be a 16-byte aligned"),
                     (dict(y=C.c_void_p(72)), f"{dst} must be a 16-byte aligned"), (dict(rows=12), "rows_per_clip must be positive and divide rows"),
                     (dict(rows_per_clip=0), "rows_per_clip"), (dict(win_length=4), "win_length must be 3, 5, 7 or 9"), (dict(win_length=11), "win_length"),
                     (dict(win_length=1), "win_length"), (dict(order=0), "order must be 1 or 2"), (dict(order=3), "order"),
                     (dict(include_static=2), "include_static"), (dict(rows=-8), "rows"), (dict(T=-1), "n_time"),
                     (dict(lengths=C.c_void_p(66)), "frame_lengths")):
        assert _call(L, name, **kw) == INVALID, kw
        msg = L.dmel_last_error()
        assert word.encode() in msg and name.encode() in msg, (kw, msg)
    assert _call(L, name, rows=0) == 0 and _call(L, name, T=0) == 0          # nothing to do is a success and launches nothing
    if not torch.cuda.is_available():                                       # loud without a device (never run with one: the pointers are not memory)
        assert _call(L, name) == capi.DMEL_ERR_NO_DEVICE and name.encode() in L.dmel_last_error()
