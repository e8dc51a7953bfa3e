"""The tangent d out / d lambd element by element: the shared case list, the inputs, the references and the metric of
tests/test_tangent_restatement_cpu.py (oracle and fp32 restatement against an independent fp64 evaluation, no GPU) and
tests/test_hip_tangent.py (every kernel path that writes a tangent, against the oracle).

The metric.  A tangent element is a signed sum -- over the bins of a mel band -- of 2 Re(conj(S) D), S the frame's spectrum and D the
spectrum of the frame under d window / d lambd: it can cancel to anything.  What an fp32 evaluation can be held to is the
cancellation-free magnitude of the same sum, scale = sum fb 2 |S| |D| (over mel + eps for the log output), which
oracle/torch_restatement.py: tangent_fp64 returns next to the tangent.  err = |got - ref| / scale on every element with scale > 0; where
scale == 0 (a mel band of no bins, a silent frame) `got` must be exactly 0.  The bar is the project's TOL = 1e-4 on every element.  A
floored fallback exists exactly as in test_hip_parity.assert_parity(allow_floor=True): denominator max(scale, FLOOR max scale), plain on
everything at or above the floor, and no more than 2 % of the tensor below it; single-bin spectrogram tangents (no mel averaging) may
use the floor 1e-5, as test_spectrogram_stage does.

The measure this replaces divided by the LARGEST tangent element of the whole tensor: 32 ... 81 % of the elements of a noise-plus-tone
clip are below 1e-4 of it, and for those it accepted any value.

The inputs.  The bar is fair only where the reference sits well inside it: the CPU test asserts, for every case below, that the oracle's
tangent and the reference's own fp32 arithmetic (the restatement's stft path in fp32) are within TOL / 4 of the fp64 evaluation.  Clips
are noise plus a 440 Hz tone with the clip mean removed: with an offset, the last ulp of the fp32 clip mean moves the tangent of the
lowest bands by up to 9e-5 in this metric (test_hip_parity.explain_by_clip_mean knows the effect from the outputs).
"""
from __future__ import annotations

import functools

import numpy as np

from dmel_amd import synth
from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from test_hip_parity import FLOOR, TOL, record_parity

SPEC_FLOOR = 1e-5          # single FFT bins: test_hip_parity.test_spectrogram_stage
REF_BAR = TOL / 4          # the room the references must leave (module docstring)


def _case(name, group, B, L, lambd, hop, n_mels, sr=16000, f_min=0.0, f_max=None, normalize_window=False, optimized=True, seed=0,
          spectrogram=False, half_window=False, dense=False, flags=0, path=0, contraction=None, one_tile=False, tpw=None, t_mod4=None, tone=0.05, noise=0.1, gated=False):
    return dict(name=name, group=group, B=B, L=L, lambd=lambd, hop=hop, n_mels=n_mels, sr=sr, f_min=f_min, f_max=f_max,
                normalize_window=normalize_window, optimized=optimized, seed=seed, spectrogram=spectrogram, half_window=half_window,
                dense=dense, flags=flags, path=path, contraction=contraction, one_tile=one_tile, tpw=tpw, t_mod4=t_mod4, tone=tone, noise=noise, gated=gated)


def _fused():
    """the fused kernel with the HTK bank at every radix plan: (n_fft, lambd, sr, n_mels, hop, T) with T = L // hop + 1 two or three
    tiles and a partial last one (frames per tile 32, 32, 16, 16, 8, 8, 2 for training)"""
    out = []
    for i, (n, lam, sr, M, hop, T) in enumerate([(32, 5.0, 8000, 10, 16, 45), (64, 9.0, 8000, 20, 40, 41), (256, 30.0, 22050, 48, 97, 21),
                                                 (1024, 150.0, 16000, 64, 100, 37), (2048, 260.0, 16000, 80, 333, 13),
                                                 (4096, 500.0, 16000, 64, 1001, 11), (16384, 1700.0, 16000, 64, 4999, 5)]):
        L = hop * (T - 1) + max(1, hop // 3)
        s = 100 + 10 * i
        out.append(_case(f"fused_n{n}", "fused", 3, L, lam, hop, M, sr, seed=s, tpw=1 if n == 256 else None))
        # every frame mostly padding: fewer than n_fft / 2 samples (n_fft 32 and 64: such a clip has at most 16 / 32 frames -- one tile)
        Ls = n // 2 - 3
        hs = max(1, Ls // (T - 1))
        out.append(_case(f"fused_n{n}_short", "fused", 2, Ls, lam, hs, M, sr, seed=s + 1, one_tile=n <= 64))
        out.append(_case(f"fused_n{n}_neg", "fused", 2, L + 1, -0.93 * lam, hop, M, sr, seed=s + 2))
        out.append(_case(f"fused_n{n}_norm", "fused", 2, L + 2, 0.97 * lam, hop, M, sr, seed=s + 3, normalize_window=True))
        out.append(_case(f"fused_n{n}_band", "fused", 2, L + 3, lam, hop, M, sr, seed=s + 4, f_min=125.0, f_max=0.4375 * sr))
    return out


CASES = _fused() + [
    # n_fft 1024, wave-local contraction: the staged epilogue needs T % 4 == 0; 1, 7 bands, more than one group of tiles, empty quads.
    # The host gives a bank to the wave-local kernel only where its schedule is short (dmel_api.cpp: wl_compact, 320 steps): ONE band, or
    # seven, over the whole spectrum are hundreds of bins wide and run the banded 16 x 16 x 4 tiles (banded_*), so the one- and seven-band
    # cases of the wave-local kernel sit on a narrow frequency range.  (The wave-local kernels are built one tile per workgroup; two
    # tiles per workgroup: tpw2_n256 below.)
    _case("wlc_m1_T37", "wlc", 3, 3650, 170.0, 100, 1, seed=200, contraction=1, t_mod4=False, tpw=1, f_min=1000.0, f_max=1300.0),
    _case("wlc_m7_T36", "wlc", 3, 3599, 128.0, 100, 7, seed=201, contraction=1, t_mod4=True, tpw=1, f_min=500.0, f_max=2500.0),
    _case("banded_m1_T37", "wlc", 3, 3650, 170.0, 100, 1, seed=206, contraction=0, t_mod4=False),
    _case("banded_m7_T36", "wlc", 3, 3599, 128.0, 100, 7, seed=207, contraction=0, t_mod4=True),
    _case("wlc_m130_T37", "wlc", 2, 3650, 170.0, 100, 130, seed=202, contraction=1, t_mod4=False),
    _case("wlc_m130_T36", "wlc", 2, 3599, 100.0, 100, 130, seed=203, contraction=1, t_mod4=True),
    # (512 bands on 513 bins are single bins: see "single bins" below; these two clips are noise alone)
    _case("wlc_m512_T36", "wlc", 2, 3599, 128.0, 100, 512, seed=1404, contraction=1, t_mod4=True, tone=0.0),
    _case("wlc_m512_T37", "wlc", 2, 3650, 100.0, 100, 512, seed=605, contraction=1, t_mod4=False, tone=0.0),
    # two tiles per workgroup (forward_tiles_per_wg: more workgroups than the device holds at once, n_fft 256 ... 1024 without the
    # wave-local contraction) and, same transform, one: fused_n256
    _case("tpw2_n256", "tpw", 3, 27367, 30.0, 5, 24, 22050, seed=210, tpw=2),
    # n_fft 1024 through a caller-supplied dense bank: exact fp32 MFMA, and the bf16x3 matrix pipe
    _case("dense_n1024", "dense", 2, 3650, 150.0, 100, 40, seed=220, dense=True, contraction=0),
    _case("dense_n1024_bf16x3", "dense", 2, 3650, 150.0, 100, 40, seed=220, dense=True, flags=8, contraction=2),
    # direct DFT (n_fft 1, 4, 16)
    _case("dft_n1", "dft", 2, 500, 0.2, 16, 10, 8000, seed=230, path=1),
    _case("dft_n4", "dft", 2, 501, 0.7, 16, 10, 8000, seed=231, path=1),
    _case("dft_n16", "dft", 2, 502, 2.0, 16, 10, 8000, seed=232, path=1),
    # the long transforms of dmel_big.hip: n_fft 32768
    _case("big_n32768", "big", 2, 40003, 2800.0, 8111, 64, 8000, seed=240, path=3),
    # optimized=False: window = whole clip, n_fft = 2 L, hop about L / 5 (six frames: one tile)
    _case("full_L64", "full", 3, 64, 6.0, 13, 12, 8000, seed=250, optimized=False, one_tile=True),
    _case("full_L1024", "full", 2, 1024, 70.0, 205, 64, seed=251, optimized=False, normalize_window=True, one_tile=True),
    _case("full_L77", "full", 2, 77, 9.0, 15, 12, 8000, seed=252, optimized=False, path=3),
    _case("full_L601", "full", 2, 601, 50.0, 120, 24, 8000, seed=253, optimized=False, normalize_window=True, path=3),
    _case("full_L5000", "full", 2, 5000, -400.0, 1000, 64, 8000, seed=254, optimized=False, path=3),
    _case("full_L8193", "full", 2, 8193, 700.0, 1639, 64, 8000, seed=255, optimized=False, path=3),
    # dmel_spectrogram_ex: the DSPEC layer (n_fft = 2 L, half window), the optimized branch at g5_n128's shape.
    # Single bins: no mel band averages over them, and |S[k]| of a noise frame is Rayleigh distributed -- among 13 000 ... 33 000 elements a
    # few sit 1 / 100 of the frame's rms or lower, where the rounding of ANY fp32 transform (relative to the frame, not to the bin) is 3e-5
    # ... 5e-4 of the bin's own scale: the reference's fp32 stft and the oracle's fp32 windowed frame included.  Whether a clip holds such a
    # near-null is a property of the clip, and the condition of the CPU test finds it: of the seeds s, s + 400, s + 800, ... these are ones
    # at which both references stay within TOL / 4 (one seed in four does at L 128 and L 100, one in ten at 8000 samples).
    _case("dspec_L128", "spec", 2, 128, 6.38, 1, 1, 2, seed=3860, optimized=False, spectrogram=True, half_window=True),
    _case("dspec_L77", "spec", 2, 77, 9.0, 5, 1, 2, seed=5461, optimized=False, spectrogram=True, half_window=True, normalize_window=True, path=3),
    _case("dspec_L100", "spec", 2, 100, 6.38, 1, 1, 2, seed=262, optimized=False, spectrogram=True, half_window=True, path=3),
    _case("dspec_L256_half", "spec", 2, 256, -20.0, 8, 1, 2, seed=2263, optimized=False, spectrogram=True, half_window=True),
    _case("spec_n128", "spec", 2, 8000, 8000 * 0.01 / 6, 80, 1, 2, seed=8664, spectrogram=True),
    # tiny clips on the default path (n_fft 64): shorter than one 16-byte load, and its neighbours
    # a loud tone in the middle half of the clip over weak noise: most tangent elements, and every one of the edge frames, are far below the
    # largest one (the self-check of the metric plants its errors here)
    _case("loud_tone_n1024", "fused", 2, 4000, 170.0, 100, 64, seed=280, tone=0.5, noise=0.01, gated=True),
] + [_case(f"tiny_L{L}", "tiny", 3, L, 9.0, 3, 20, 8000, seed=270 + L, one_tile=True) for L in (2, 7, 15, 16, 17)] + [
    # ... and at the transforms where test_hip_lengths_parity.py met its d lambd discrepancy: a clip of a few samples inside a long window.
    # There conj(S) D is almost purely imaginary in every low bin (the clip's samples sum to zero and the window barely changes across
    # them), so each tangent element is 1e2 ... 1e5 below its scale 2 |S| |D|
    _case("tiny_L2_n1024", "tiny", 3, 2, 128.0, 1, 64, seed=290, one_tile=True),
    _case("tiny_L7_n1024", "tiny", 3, 7, -150.0, 2, 64, seed=1891, one_tile=True, normalize_window=True),
    _case("tiny_L13_n256", "tiny", 3, 13, 30.0, 4, 48, 22050, seed=292, one_tile=True),
    _case("tiny_L15_n8192", "tiny", 2, 15, 700.0, 5, 40, seed=293, one_tile=True),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def n_fft_of(case) -> int:
    return O.n_fft(case["lambd"]) if case["optimized"] else 2 * case["L"]


def out_shape(case):
    rows = n_fft_of(case) // 2 + 1 if case["spectrogram"] else case["n_mels"]
    return (case["B"], 1, rows, case["L"] // case["hop"] + 1)


def synth_clips(B, L, seed, sr, tone=0.05, noise=0.1, gated=False):
    """(B, L) fp32: noise + a 440 Hz tone (``gated``: in the middle half of the clip only), the clip mean removed (module docstring)"""
    x = synth.normal((B, L), seed=seed, scale=noise, dtype=np.float64)
    ph = 6.283 * synth.uniform01(B, seed=seed + 7)
    gate = ((np.arange(L) >= L // 4) & (np.arange(L) < 3 * L // 4)) if gated else np.ones(L)
    x += tone * gate[None, :] * np.sin(2.0 * np.pi * 440.0 * np.arange(L)[None, :] / float(max(sr, 8000)) + ph[:, None])
    x -= x.mean(axis=1, keepdims=True)                       # zero offset (module docstring)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _input(name):
    c = BY_NAME[name]
    x = synth_clips(c["B"], c["L"], c["seed"], c["sr"], c["tone"], c["noise"], c["gated"])
    x.setflags(write=False)
    return x


def make_input(case) -> np.ndarray:
    """(B, L) fp32, read-only and shared: noise + a 440 Hz tone, the clip mean removed"""
    return _input(case["name"])


@functools.lru_cache(maxsize=None)
def dense_bank(name):
    """a caller-supplied bank with no zero entry (every MFMA block), positive so that the log output exists"""
    c = BY_NAME[name]
    fb = (0.05 + 0.95 * synth.uniform01((n_fft_of(c) // 2 + 1) * c["n_mels"], seed=c["seed"] + 3)).astype(np.float32)
    return fb.reshape(n_fft_of(c) // 2 + 1, c["n_mels"])


def _kw(case, log):
    return dict(f_min=case["f_min"], f_max=case["f_max"], normalize_window=case["normalize_window"], log=log, optimized=case["optimized"],
                fb=dense_bank(case["name"]) if case["dense"] else None, spectrogram=case["spectrogram"])


@functools.lru_cache(maxsize=None)
def _fp64(name, log):
    c = BY_NAME[name]
    res = R.tangent_fp64(make_input(c), c["lambd"], c["hop"], c["n_mels"], c["sr"], **_kw(c, log))
    for a in res:
        a.setflags(write=False)
    return res


def fp64(case, log):
    """(out, tangent, scale) of tangent_fp64, computed once per session and read-only"""
    return _fp64(case["name"], bool(log))


def fp32(case, log):
    """the same construction in the reference's own fp32 arithmetic"""
    return R.tangent_fp32(make_input(case), case["lambd"], case["hop"], case["n_mels"], case["sr"], **_kw(case, log))


@functools.lru_cache(maxsize=None)
def _oracle(name, log):
    c = BY_NAME[name]
    x = make_input(c)
    if c["dense"] or (c["spectrogram"] and c["optimized"]):
        return None                                          # the oracle has no such entry point: tangent_fp64 is the reference
    if c["spectrogram"]:
        if log:
            return None
        res = O.dspec(x, c["lambd"], c["hop"], c["normalize_window"])
    else:
        res = O.forward(x, c["lambd"], c["hop"], c["n_mels"], c["sr"], c["f_min"], c["f_max"], c["normalize_window"], apply_log=log,
                        optimized=c["optimized"])
    for a in res:
        a.setflags(write=False)
    return res


def oracle(case, log):
    """(out, tangent) of the C oracle in the layout of out_shape, or None where it has no entry point (dense bank, the optimized
    spectrogram stage); computed once per session and read-only"""
    return _oracle(case["name"], bool(log))


def reference(case, log):
    """(out, tangent) the kernels are compared with: the oracle's, tangent_fp64's where the oracle has none"""
    o = oracle(case, log)
    if o is not None:
        return o
    out, tan, _ = fp64(case, log)
    return out, tan


def floor_of(case) -> float:
    return SPEC_FLOOR if case["spectrogram"] else FLOOR


def tangent_stats(got, ref, scale, floor=FLOOR):
    """the comparison of the tangent `got` with `ref` against the cancellation-free magnitude `scale`, with nothing hidden"""
    g, r, s = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, scale))
    assert g.shape == r.shape == s.shape, (g.shape, r.shape, s.shape)
    err = np.abs(g - r)
    pos = s > 0
    top = float(s.max()) if s.size else 0.0
    above = s >= floor * top
    rel = np.zeros_like(err)
    rel[pos] = err[pos] / s[pos]
    worst = int(rel.argmax()) if rel.size else 0
    old_scale = float(np.abs(r).max()) + 1e-30 if r.size else 1.0
    return {"n": int(s.size), "max_err": float(rel.max()) if rel.size else 0.0, "worst_index": worst,
            "frac_below_floor": float(1.0 - above.mean()) if s.size else 0.0,
            "max_err_above_floor": float(rel[above & pos].max()) if (above & pos).any() else 0.0,
            "floored_max_err": float((err / np.maximum(s, floor * top + 1e-300)).max()) if s.size and top > 0 else 0.0,
            "max_abs_where_scale_is_zero": float(np.abs(g[~pos]).max()) if (~pos).any() else 0.0,
            "global_max_measure": float(err.max()) / old_scale if err.size else 0.0,
            "frac_below_tol_of_largest": float((np.abs(r) < TOL * old_scale).mean()) if r.size else 0.0}


def assert_tangent(name, got, ref, scale, tol=TOL, floor=FLOOR, max_frac_below=0.02, allow_floor=True, shape=None):
    """|got - ref| / scale <= tol on every element with scale > 0 and got == 0 exactly elsewhere; recorded under ``name`` in the parity
    report.  The plain form is tried first; the floored one (module docstring) only if it fails, and the record says which was needed."""
    st = tangent_stats(got, ref, scale, floor)
    st["floor_needed"] = bool(st["max_err"] > tol)
    if shape is not None:
        st["worst_index"] = [int(v) for v in np.unravel_index(st["worst_index"], shape)]
    record_parity(name, st)
    assert st["max_abs_where_scale_is_zero"] == 0.0, (name, "an element that cannot be anything but zero is not zero", st)
    if not st["floor_needed"]:
        return st
    assert allow_floor, (name, "tangent error above the bar", st)
    assert st["max_err_above_floor"] <= tol, (name, st)
    assert st["floored_max_err"] <= tol, (name, st)
    assert st["frac_below_floor"] <= max_frac_below, (name, st)
    return st
