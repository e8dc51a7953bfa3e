"""Every kernel path that writes a tangent d out / d lambd, element by element through the C ABI against the oracle's tangent, in the
metric of tests/tangent_cases.py (|got - ref| over the cancellation-free magnitude of the element, 1e-4 on every element; exact zeros
where nothing can contribute).  Until here most paths saw their tangent only through one dot product with one seeded cotangent, where a
few wrong elements -- an edge frame, the tail tile, a Nyquist row, the last mel tile of a group -- disappear.  Each case asserts from
dmel_plan_get_info that it runs the path it is named for; the outputs are compared too.  tests/test_tangent_restatement_cpu.py holds
the references to a quarter of the bar on these very inputs.

Not here, because an existing test asserts their tangent is the scalar host path's bit for bit: the band-split forwards
(test_hip_band_split.py::test_tangent_rows_through_the_c_abi), the device-lambd forwards (test_hip_device_lambd.py: torch.equal(tan0,
tan1); test_hip_lengths_parity.py::test_c_abi_tangent_at_partial_lengths for the lengths pair).  The multi-window forward had no such
test (its channels were compared through lambd.grad to 1e-6): test_multi_window_tangent_is_the_scalar_paths below."""
import numpy as np
import pytest
import torch

import tangent_cases as TC
from tangent_cases import assert_tangent
from test_hip_parity import TOL, _rel_err, assert_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-10
SENTINEL = 7.0


def _forward(case, log, extra_flags=0, out_dtype=torch.float32):
    """(out, tangent, plan info) of one training forward of `case` through the C ABI; both in the layout of TC.out_shape"""
    from dmel_amd import capi
    x = torch.from_numpy(np.array(TC.make_input(case))).to(DEV)
    B, L, hop = case["B"], case["L"], case["hop"]
    n = TC.n_fft_of(case)
    shape = TC.out_shape(case)
    out = torch.full(shape, SENTINEL, dtype=out_dtype, device=DEV)
    tan = torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if case["spectrogram"]:
        plan = capi.Plan(L, hop, 1, 2, 0.0, 1.0, case["normalize_window"])                       # as SpectrogramLayer builds it
        plan.spectrogram_ex(x.data_ptr(), B, case["lambd"], n, out.data_ptr(), tan.data_ptr(), st, remove_dc=True, half_window=case["half_window"])
    else:
        plan = capi.Plan(L, hop, case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
        if case["dense"]:
            plan.set_filterbank(n, TC.dense_bank(case["name"]))
        flags = case["flags"] | extra_flags | (0 if case["optimized"] else capi.DMEL_FLAG_FULL_WINDOW)
        plan.forward(x.data_ptr(), B, case["lambd"], out.data_ptr(), tan.data_ptr(), log, EPS, st, extra_flags=flags)
    torch.cuda.synchronize()
    info = plan.info()
    plan.close()
    return out, tan, info


LDS_CHIRP = {"full_L77": True, "full_L601": True, "full_L5000": True, "full_L8193": False}      # chirp-z in LDS (L 5000: as two half transforms) / the sequence in global memory


def _assert_path(case, info):
    """the case runs the path it is named for"""
    T = case["L"] // case["hop"] + 1
    assert info["n_fft"] == TC.n_fft_of(case) and info["n_time"] == T, (case["name"], info)
    assert info["kernel_path"] == case["path"], (case["name"], info)
    if case["contraction"] is not None:
        assert info["contraction"] == case["contraction"], (case["name"], info)
    if case["name"] in LDS_CHIRP:
        assert (info["lds_bytes"] > 0) == LDS_CHIRP[case["name"]], (case["name"], info)
    if case["path"] == 0 and not case["spectrogram"]:
        fpt = info["frames_per_tile"]
        tiles = -(-T // fpt)
        if case["one_tile"]:
            assert tiles == 1, (case["name"], T, info)
        else:
            assert tiles >= 2 and T % fpt != 0, (case["name"], "at least two tiles per clip and a partial last one", T, info)
        if case["tpw"] is not None:                              # tiles per workgroup, from the grid
            assert info["grid_fwd"] == case["B"] * -(-tiles // case["tpw"]), (case["name"], tiles, info)
            assert case["tpw"] == 1 or info["grid_fwd"] < case["B"] * tiles
        if case["t_mod4"] is not None:                           # the staged epilogue of the wave-local contraction needs T % 4 == 0
            assert (T % 4 == 0) == case["t_mod4"]


def _assert_outputs(tag, case, log, o, o_ref):
    if case["spectrogram"]:
        assert _rel_err(o, o_ref, floor=TC.SPEC_FLOOR) <= TOL, tag          # single bins: as test_spectrogram_stage
    elif log:
        assert_parity(tag + "/exp_logmel", np.exp(o.astype(np.float64)), np.exp(np.asarray(o_ref, dtype=np.float64)))
    else:
        assert_parity(tag + "/mel", o, o_ref)


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_tangent_matches_oracle_elementwise(case):
    for log in ((False,) if case["spectrogram"] else (False, True)):
        tag = f"tangent/{case['name']}/{'log' if log else 'lin'}"
        out, tan, info = _forward(case, log)
        _assert_path(case, info)
        o, t = out.cpu().numpy(), tan.cpu().numpy()
        assert np.isfinite(o).all() and np.isfinite(t).all() and not (t == SENTINEL).any() and not (o == SENTINEL).any(), tag
        o_ref, t_ref = TC.reference(case, log)
        _, _, scale = TC.fp64(case, log)
        st = TC.tangent_stats(t, t_ref, scale, TC.floor_of(case))
        print(f"{tag}: max err {st['max_err']:.3g} at {np.unravel_index(st['worst_index'], t.shape)}, floored {st['floored_max_err']:.3g}, "
              f"{100 * st['frac_below_floor']:.2f} % below the floor, old measure {st['global_max_measure']:.3g}, info {info}")
        _assert_outputs(tag, case, log, o, o_ref)
        assert_tangent(tag, t, t_ref, scale, floor=TC.floor_of(case), shape=t.shape)


@pytest.mark.parametrize("name", ["dense_n1024", "dense_n1024_bf16x3", "fused_n256"])
def test_bf16_output_leaves_the_tangent_bits_alone(name):
    """DMEL_FLAG_OUT_BF16 rounds the output once more and nothing else: the tangent has the bits of the fp32-output run"""
    from dmel_amd import capi
    case = TC.BY_NAME[name]
    for log in (False, True):
        out32, tan32, info32 = _forward(case, log)
        out16, tan16, info16 = _forward(case, log, extra_flags=capi.DMEL_FLAG_OUT_BF16, out_dtype=torch.bfloat16)
        assert info16["contraction"] == info32["contraction"] and info16["kernel_path"] == info32["kernel_path"]
        assert torch.equal(tan16.view(torch.int32), tan32.view(torch.int32)), (name, log)
        assert torch.equal(out16.view(torch.int16), out32.to(torch.bfloat16).view(torch.int16)), (name, log)


@pytest.mark.parametrize("log", [False, True])
def test_multi_window_tangent_is_the_scalar_paths(log):
    """dmel_forward_multi against dmel_forward per channel: out AND tangent bit for bit (n_fft 64, 1024 twice, 4096: one launch serves
    two channels); the scalar path's tangent is held to the oracle above"""
    from dmel_amd import capi
    case = TC.BY_NAME["fused_n1024"]
    B, L, hop, M, sr = case["B"], case["L"], case["hop"], case["n_mels"], case["sr"]
    T = L // hop + 1
    lams = [9.0, 150.0, 500.0, -128.0]
    x = torch.from_numpy(np.array(TC.make_input(case))).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    plan = capi.Plan(L, hop, M, sr)
    out = torch.full((B, len(lams), M, T), SENTINEL, device=DEV)
    tan = torch.full((B, len(lams), M, T), SENTINEL, device=DEV)
    scratch = torch.zeros((plan.scratch_bytes_multi(B, len(lams)),), dtype=torch.uint8, device=DEV)
    plan.forward_multi(x.data_ptr(), B, lams, out.data_ptr(), tan.data_ptr(), log, EPS, st, scratch.data_ptr())
    ref_plan = capi.Plan(L, hop, M, sr)
    for k, lam in enumerate(lams):
        o_k, t_k = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
        ref_plan.forward(x.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), log, EPS, st)
        torch.cuda.synchronize()
        assert torch.equal(out[:, k:k + 1].contiguous().view(torch.int32), o_k.view(torch.int32)), (k, lam)
        assert torch.equal(tan[:, k:k + 1].contiguous().view(torch.int32), t_k.view(torch.int32)), (k, lam)
