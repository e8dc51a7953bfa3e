"""The references of the filterbank gradient, element by element, against an independent fp64 evaluation (oracle/torch_restatement.py:
fbgrad_fp64), in the metric of tests/fbgrad_cases.py: |got - ref| over the cancellation-free magnitude sum spec |gm| of the element, on
every element, no floor.  The condition that makes the bar of tests/test_hip_fbgrad.py fair: on every shared case the C oracle AND the
reference's own fp32 arithmetic stay within REF_BAR = TOL / 4 of the fp64 evaluation, and so do the committed reference fixtures
(g8_fbgrad_*: torch autograd through the reference with mel_fb made a leaf).  Then the metric checks itself: errors planted where a kernel
would make them pass the measure the suite used (test_hip_parity._gfb_err) and fail this one.  No GPU."""
import os

import numpy as np
import pytest

import cases as C
import fbgrad_cases as FC
import tangent_cases as TC
from dmel_amd import synth
from fbgrad_cases import EPS, REF_BAR, TOL, assert_fbgrad, fbgrad_stats
from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from test_hip_parity import _gfb_err          # the measure the suite used: the planted faults below must pass it


def _check_scale(ref, sc):
    assert np.isfinite(ref).all() and np.isfinite(sc).all() and (sc >= 0).all()
    assert (np.abs(ref) <= sc * (1 + 1e-9) + 1e-300).all(), "scale bounds the gradient"
    assert (ref[sc == 0] == 0).all(), "scale == 0 only where the reference is exactly 0"


@pytest.mark.parametrize("case", FC.CASES, ids=[c["name"] for c in FC.CASES])
def test_oracle_and_fp32_reference_sit_inside_the_bar(case):
    """both references within TOL / 4 of fbgrad_fp64 on every element, linear and log"""
    x, g = FC.make_input(case), FC.make_cotangent(case)
    args = (x, case["lambd"], case["hop"], case["n_mels"], case["sr"], g)
    for log in (False, True):
        tag = f"fbgrad_ref/{case['name']}/{'log' if log else 'lin'}"
        out = FC.cpu_log_out(case) if log else None                 # the oracle's log output, as a kernel is given its own
        kw = dict(FC._kw(case), eps=EPS if (log and out is None) else None)
        ref, sc = FC.fp64_lin(case) if not log else R.fbgrad_fp64(*args, out, **kw)
        assert ref.shape == FC.grad_shape(case) == sc.shape
        _check_scale(ref, sc)
        g32, _ = R.fbgrad_fp32(*args, out, **kw)
        st32 = assert_fbgrad(tag + "/fp32_restatement", g32, ref, sc, tol=REF_BAR, shape=ref.shape)
        line = f"{tag}: fp32 restatement {st32['max_err']:.3g}"
        orc = FC.oracle(case, log, out)
        if orc is not None:
            st = assert_fbgrad(tag + "/oracle", orc, ref, sc, tol=REF_BAR, shape=ref.shape)
            line += f", oracle {st['max_err']:.3g} at {st['worst_index']}"
        print(line + f"; {100 * st32['frac_below_tol_of_largest']:.1f} % of the elements below 1e-4 of the largest")


def _bf16x3(a, b):
    """DMEL_FLAG_MFMA_BF16X3 restated: both fp32 operands split into two bf16 halves (hi = bf16(v), lo = bf16(v - hi), round to nearest even),
    three of the four products kept -- hi hi + lo hi + hi lo -- and added here without further rounding (the kernel adds them in fp32)"""
    import torch
    def split(v):
        hi = v.to(torch.bfloat16).to(torch.float32)
        return hi.double(), (v - hi).to(torch.bfloat16).double()
    (ah, al), (bh, bl) = split(a), split(b)
    c = lambda u, v: torch.einsum("bft,bmt->fm", u, v)
    return (c(al, bh) + c(ah, bl) + c(ah, bh)).numpy()


@pytest.mark.parametrize("case", FC.CASES, ids=[c["name"] for c in FC.CASES])
def test_three_term_bf16_split_sits_inside_the_bar(case):
    """the arithmetic DMEL_FLAG_MFMA_BF16X3 is built on, applied to the fp32 restatement's operands: within TOL / 4 of fbgrad_fp64, so the
    flag's runs are held to the same TOL as the exact ones.  (Dropping one of the three products costs 2e-3 in this metric: asserted too.)"""
    import torch
    x, g = FC.make_input(case), FC.make_cotangent(case)
    args = (x, case["lambd"], case["hop"], case["n_mels"], case["sr"], g)
    for log in (False, True):
        out = FC.cpu_log_out(case) if log else None
        kw = dict(FC._kw(case), eps=EPS if (log and out is None) else None)
        ref, sc = FC.fp64_lin(case) if not log else R.fbgrad_fp64(*args, out, **kw)
        p, gm = R.fbgrad_operands(torch.float32, *args, out, **kw)
        st = assert_fbgrad(f"fbgrad_ref/{case['name']}/{'log' if log else 'lin'}/bf16x3_emulation", _bf16x3(p, gm), ref, sc, tol=REF_BAR, shape=ref.shape)
        print(f"{case['name']} {'log' if log else 'lin'}: three-term bf16 split {st['max_err']:.3g}")
    if case["name"] == "rows_F513":
        hi = lambda v: v.to(torch.bfloat16).double()
        two = torch.einsum("bft,bmt->fm", hi(p), hi(gm)) + torch.einsum("bft,bmt->fm", (p - hi(p).float()).to(torch.bfloat16).double(), hi(gm))
        assert fbgrad_stats(two.numpy(), ref, sc)["max_err"] > 10 * TOL


def test_every_instantiation_of_the_kernel_is_reached():
    """LOG x TINY x BF16X3 x LEN of dmel_fbgrad_lds_kernel from the case list: both output kinds and the flag run on every case, so T < 4 and
    `lengths` must each occur with and without the other; every C ABI entry point and the layer have a case"""
    seen = {(FC.n_time(c) < 4, c["lengths"] is not None) for c in FC.CASES if c["entry"] != "layer"}
    assert seen == {(False, False), (True, False), (False, True), (True, True)}
    assert {c["entry"] for c in FC.CASES} == {"host", "dev", "saved", "saved_dl", "lengths", "layer"}


def _golden_case_references(tag, case):
    """fp32 restatement and oracle against fbgrad_fp64 on the inputs of a case of tests/golden/cases.py (or one derived from it, as the GPU
    tests derive theirs), linear and log; returns {log: (ref, scale)} with the log output computed by the reference itself"""
    x, g = C.make_input(case).astype(np.float32), C.make_cotangent(case)
    args = (x, case["lambd"], case["hop"], case["n_mels"], case["sr"], g)
    kw = dict(f_min=case["f_min"], f_max=case["f_max"], normalize_window=case["normalize_window"], optimized=case.get("optimized", True))
    res = {}
    for log in (False, True):
        t = f"fbgrad_ref/{tag}/{'log' if log else 'lin'}"
        ref, sc = R.fbgrad_fp64(*args, None, eps=EPS if log else None, **kw)
        _check_scale(ref, sc)
        g32, _ = R.fbgrad_fp32(*args, None, eps=EPS if log else None, **kw)
        st32 = assert_fbgrad(t + "/fp32_restatement", g32, ref, sc, tol=REF_BAR, shape=ref.shape)
        line = f"{t}: fp32 restatement {st32['max_err']:.3g}"
        if kw["optimized"]:
            # the oracle with its own log output, against the fp64 evaluation given that same output: what the GPU tests do with the kernel's
            out = O.forward(x, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"],
                            apply_log=True, eps=EPS, want_tangent=False)[0] if log else None
            r2, s2 = R.fbgrad_fp64(*args, out, **kw) if log else (ref, sc)
            st = assert_fbgrad(t + "/oracle", O.backward_fb(x, case["lambd"], case["hop"], g, out, case["normalize_window"]), r2, s2, tol=REF_BAR,
                               shape=ref.shape)
            line += f", oracle {st['max_err']:.3g} at {st['worst_index']}"
        print(line + f"; {100 * st32['frac_below_tol_of_largest']:.1f} % of the elements below 1e-4 of the largest")
        res[log] = (ref, sc)
    return res


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g5_n128", "g6_n256_ragged", "g7_mel_nonopt_256", "g7_mel_nonopt_601"])
def test_committed_reference_fixtures_sit_inside_the_bar(name):
    """g8_fbgrad_*.npz (the reference's fp32 autograd with mel_fb a leaf): within TOL / 4 of fbgrad_fp64, and so are the oracle and the fp32
    restatement on these inputs; the two g7 cases through optimized=False"""
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g8_fbgrad_{name}.npz"))
    refs = _golden_case_references(name, C.BY_NAME[name])
    for log, key in ((False, "gfb_lin"), (True, "gfb_log")):
        ref, sc = refs[log]
        st = assert_fbgrad(f"fbgrad_ref/{name}/{'log' if log else 'lin'}/fixture", gold[key], ref, sc, tol=REF_BAR, shape=ref.shape)
        print(f"{name} {key}: fixture {st['max_err']:.3g} at {st['worst_index']}, old measure {st['global_max_measure']:.3g}")


# the inputs of the GPU tests that carry the element-wise assertion beside the old one (tests/test_hip_parity.py:
# test_filterbank_gradient_with_short_and_ragged_rows, test_optional_gradients_on_edge_configurations)
RAGGED = [dict(C.BY_NAME["g1_c1"], name=f"fb_T{T}", B=3, L=700, lambd=40.0, hop=hop, n_mels=24) for hop, T in [(1000, 1), (300, 3), (100, 8), (47, 15), (41, 18)]]
EDGE = [C.BY_NAME[n] for n in ["g6_normwin", "g6_neglambd", "g6_fminmax", "g6_n2048_short", "g5_n4096"]]


@pytest.mark.parametrize("case", RAGGED + EDGE, ids=[c["name"] for c in RAGGED + EDGE])
def test_inputs_of_the_existing_gpu_sites_sit_inside_the_bar(case):
    _golden_case_references(case["name"], case)


@pytest.mark.parametrize("lam", [80.0, 128.0], ids=["nfft512", "nfft1024"])
def test_inputs_of_the_lengths_oracle_comparison_sit_inside_the_bar(lam):
    """tests/test_hip_fb_lengths.py::test_every_clip_matches_the_oracle_on_that_clip_alone: ten clips of Tc = 1 ... T frames in one launch,
    a dense positive bank; the per-clip oracle sum and the fp32 restatement against fbgrad_fp64 with lengths"""
    import torch
    L, hop, M, sr, lens = 4000, 100, 40, 16000, [1, 150, 250, 399, 400, 1499, 1500, 1650, 3999, 4000]
    B, T = len(lens), L // hop + 1
    x, g = synth.waveforms(B, L, seed=5), synth.cotangent((B, 1, M, T), seed=6)
    fb = O.mel_fbanks(O.n_fft(lam) // 2 + 1, 0.0, sr // 2, M, sr) + (0.02 * torch.rand((O.n_fft(lam) // 2 + 1, M), generator=torch.Generator().manual_seed(1234))).numpy()
    for log in (False, True):
        kw = dict(lengths=lens, fb=fb, eps=EPS if log else None)
        ref, sc = R.fbgrad_fp64(x, lam, hop, M, sr, g, None, **kw)
        _check_scale(ref, sc)
        g32, _ = R.fbgrad_fp32(x, lam, hop, M, sr, g, None, **kw)
        st32 = assert_fbgrad(f"fbgrad_ref/fb_lengths_{int(lam)}/{'log' if log else 'lin'}/fp32_restatement", g32, ref, sc, tol=REF_BAR, shape=ref.shape)
        # the oracle clip by clip, the log output from the fp64 mel of that bank
        orc = np.zeros_like(ref)
        for b, Lb in enumerate(lens):
            Tc = Lb // hop + 1
            out = None
            if log:
                spec = O.spectrogram(x[b:b + 1, :Lb], lam, hop, False, True).astype(np.float64)
                out = np.log(np.einsum("ft,fm->mt", spec[0], fb.astype(np.float64)) + EPS)[None, None].astype(np.float32)
            orc += O.backward_fb(x[b:b + 1, :Lb], lam, hop, g[b:b + 1, :, :, :Tc], out)
        if log:
            full = np.zeros((B, 1, M, T), np.float32)
            for b, Lb in enumerate(lens):
                spec = O.spectrogram(x[b:b + 1, :Lb], lam, hop, False, True).astype(np.float64)
                full[b, 0, :, :Lb // hop + 1] = np.log(np.einsum("ft,fm->mt", spec[0], fb.astype(np.float64)) + EPS)
            ref, sc = R.fbgrad_fp64(x, lam, hop, M, sr, g, full, lengths=lens)
        st = assert_fbgrad(f"fbgrad_ref/fb_lengths_{int(lam)}/{'log' if log else 'lin'}/oracle", orc, ref, sc, tol=REF_BAR, shape=ref.shape)
        print(f"lengths {lam} {'log' if log else 'lin'}: fp32 restatement {st32['max_err']:.3g}, oracle {st['max_err']:.3g}")


# ---- the metric checks itself: what a wrong kernel edge would leave, under both measures ----------------------------------------------------
# Inputs: g5_n128 with the log output (95 % of the tensor below 1e-4 of the largest element: three mel bands hold no bin, out = log(eps), and
# their columns are 1e10 louder than the other 61) and the loud gated tone of tangent_cases, linear (94 %: a few rows carry the tone) and log
# (98.6 %: the columns of the quiet bands are the loud ones).  Measured here, old measure / element by element:
#                            zeroed Nyquist row     1 % on the quietest column     last frame of the last clip dropped
#   loud_tone_n1024 lin      1.1e-5 / 0.47          2.1e-3 / 4.2e-3 (*)            1.4e-6 / 0.098
#   loud_tone_n1024 log      1.5e-5 / 0.60          3.4e-8 / 6.6e-3                7.7e-6 / 0.59
#   g5_n128 log              0.54 (**) / 0.83       7.4e-12 / 3.7e-3               0.11 (**) / 0.74
# (*) with the linear output every column has the same row profile (the bank does not enter its own gradient): there is no quiet column, and
#     1 % of any column is 2e-3 of the largest element -- the old measure sees it, so that plant is not made there.
# (**) a whole row, or a whole frame, also reaches the three loud columns, where the old measure does see it.  What it cannot see is the same
#     fault on the other 61 columns (as a wrong second column tile, or a fault in one wave's columns, would leave it): planted there.
SELFCHECK = ["g5_n128_log", "loud_tone_n1024_lin", "loud_tone_n1024_log"]


def _selfcheck_inputs(which):
    """(x, lambd, hop, M, sr, cotangent, log)"""
    log = which.endswith("_log")
    if which.startswith("g5_n128"):
        c = C.BY_NAME["g5_n128"]
        return C.make_input(c).astype(np.float32), c["lambd"], c["hop"], c["n_mels"], c["sr"], C.make_cotangent(c), log
    c = TC.BY_NAME["loud_tone_n1024"]
    return np.array(TC.make_input(c)), c["lambd"], c["hop"], c["n_mels"], c["sr"], synth.cotangent(TC.out_shape(c), seed=c["seed"] + 11), log


def _selfcheck_reference(which, g=None):
    x, lam, hop, M, sr, g0, log = _selfcheck_inputs(which)
    return R.fbgrad_fp64(x, lam, hop, M, sr, g0 if g is None else g, None, eps=EPS if log else None)


def _quiet_columns(which, ref):
    """the columns a whole-row or whole-frame fault is planted on: all of them, on g5_n128 log those below 1e-4 of the largest element (**)"""
    top = np.abs(ref).max(axis=0)
    quiet = top < TOL * top.max() if which == "g5_n128_log" else np.ones(ref.shape[1], dtype=bool)
    assert quiet.sum() >= 0.9 * ref.shape[1]
    return quiet


def _both_measures(tag, bad, ref, sc):
    st = fbgrad_stats(bad, ref, sc)
    print(f"{tag}: old measure {st['global_max_measure']:.3g}, element by element {st['max_err']:.3g}; "
          f"{100 * st['frac_below_tol_of_largest']:.1f} % of the elements below 1e-4 of the largest")
    assert _gfb_err(bad, ref) <= TOL, (tag, "the old measure was meant to pass", st)
    assert st["max_err"] > 10 * TOL, (tag, st)
    with pytest.raises(AssertionError):
        assert_fbgrad("fbgrad_selfcheck/" + tag, bad, ref, sc, shape=ref.shape)


@pytest.mark.parametrize("which", SELFCHECK)
def test_metric_catches_a_zeroed_nyquist_row(which):
    """the folded 65th row of the last row tile never stored"""
    ref, sc = _selfcheck_reference(which)
    bad = ref.copy()
    bad[-1, _quiet_columns(which, ref)] = 0.0
    _both_measures(which + "/nyquist_row", bad, ref, sc)


@pytest.mark.parametrize("which", ["g5_n128_log", "loud_tone_n1024_log"])
def test_metric_catches_one_percent_on_a_quiet_column(which):
    """(not with the linear output: no column is quiet there (*))"""
    ref, sc = _selfcheck_reference(which)
    cols = sc.max(axis=0)
    m = int(np.where(cols > 0, cols, np.inf).argmin())
    bad = ref.copy()
    bad[:, m] *= 1.01
    _both_measures(which + "/quiet_column", bad, ref, sc)


@pytest.mark.parametrize("which", SELFCHECK)
def test_metric_catches_a_dropped_last_frame_of_one_clip(which):
    """a slice that loses the K-block piece at a clip's end: the gradient without the last frame of the last clip"""
    ref, sc = _selfcheck_reference(which)
    g = np.array(_selfcheck_inputs(which)[5])
    g[-1, :, :, -1] = 0.0
    dropped, _ = _selfcheck_reference(which, g)
    quiet = _quiet_columns(which, ref)
    bad = ref.copy()
    bad[:, quiet] = dropped[:, quiet]
    _both_measures(which + "/dropped_frame", bad, ref, sc)


def test_metric_demands_exact_zeros_where_nothing_can_contribute():
    ref = np.array([[1.0, 0.0], [2.0, 0.0]])
    sc = np.array([[1.5, 0.0], [2.5, 0.0]])
    assert_fbgrad("fbgrad_selfcheck/zeros_ok", ref, ref, sc)
    bad = ref.copy()
    bad[1, 1] = 1e-30
    with pytest.raises(AssertionError):
        assert_fbgrad("fbgrad_selfcheck/zeros", bad, ref, sc)
    bad = ref.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError):
        assert_fbgrad("fbgrad_selfcheck/nan", bad, ref, sc)
