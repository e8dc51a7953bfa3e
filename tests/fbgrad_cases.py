"""The filterbank gradient d loss / d mel_fb element by element: the shared case list, the inputs, the references and the metric of
tests/test_fbgrad_restatement_cpu.py (oracle, fp32 restatement and the committed fixtures against an independent fp64 evaluation, no GPU)
and tests/test_hip_fbgrad.py (every instantiation of dmel_fbgrad_lds_kernel and the reduce kernel, through every entry point).

The metric.  grad_fb[f, m] = sum_{b,t} spec[b, f, t] gm[b, m, t], gm = grad_out (linear output) or grad_out exp(-out) (log output, `out`
the saved log output the kernel itself is given).  spec >= 0, so the sum cancels only through the sign of the cotangent and
scale[f, m] = sum_{b,t} spec[b, f, t] |gm[b, m, t]| is free of cancellation: oracle/torch_restatement.py: fbgrad_fp64 returns it next to
the gradient.  err = |got - ref| / scale on EVERY element with scale > 0, got == 0 exactly where scale == 0; the bar is the project's
TOL = 1e-4, plain: no floor, no share of the tensor left out.  With per-clip lengths both sums run over each clip's own frames.

The measure this stands beside (test_hip_parity._gfb_err) divides the largest error by the LARGEST element of the whole (F, M) tensor.
With the log output a mel band of no bins has out = log(eps): its column is 1e10 louder than the others, and up to 98 % of the tensor is
below 1e-4 of the largest element -- for those the old measure accepts any value.  fbgrad_stats reports both, and that share.

The inputs.  The bar is fair only where the references sit well inside it: the CPU test asserts for every case below that the C oracle and
the reference's own fp32 arithmetic are within REF_BAR = TOL / 4 of the fp64 evaluation.  Clips follow tangent_cases.synth_clips (noise plus
a 440 Hz tone, the clip mean removed), the cotangent is a seeded signed normal one.  A clip of a handful of samples inside a long window is
not admissible: its scale is tiny against the frame and the last ulp of the clip mean shows (7 samples in a 1024-point window: fp32
restatement 3e-4, oracle 1.8e-4 in this metric); no case here is of that kind, and short clips of a lengths batch ride in a launch whose
other clips carry the scale.  Seed rule: a case whose references miss REF_BAR takes seed + 400, + 800, ... until they hold; none needed it.

Case -> edge of dmel_aux.hip (tile 64 rows x 128 columns, K-blocks of 16 frames, 16-byte pieces of 4 frames, ring depth 3, 8 reduce
waves).  Every case runs linear and log, exact and DMEL_FLAG_MFMA_BF16X3; T < 4 takes the TINY build, `lengths` the LEN build:

  rows_F17, rows_F33            one partial row tile, no folded row (n_fft 32, 64); F * M no multiple of 64
  rows_F65                      the folded 65th row inside the only tile (n_fft 128)
  rows_F129 / F513 / F1025      the fold in the last of 2 / 8 / 16 row tiles (n_fft 256, 1024, 2048)
  rows_F8193                    128 row tiles (n_fft 16384, T = 5)
  rows_F1, rows_F2              n_fft 1 and 2: the direct-DFT forward, a bank of empty bands
  full_L63 / L77 / L127         DMEL_FLAG_FULL_WINDOW, F = L + 1 not 64 k + 1: one exactly full tile (64), 78, two full tiles (128)
  full_L601, full_L1024         ... F = 602 (chirp-z spectrogram pass), F = 1025 (folds)
  cols_M1 ... cols_M130         one column; 127, 128, 129 (the second column tile holds one live row, the rest clamped), 130
  cols_M512                     four column tiles (on 513 bins: bands of no bins, the loud log columns)
  ends_T1, T2, T3               TINY: element-wise requests
  ends_T4 ... T7                one piece; T % 4 = 1, 2, 3 (in_place shifts by 3, 2, 1)
  ends_T16, T17, T32            an exactly full block; one frame into the second block; two full blocks
  ends_T29, ends_T33            T % 16 = 13 and 1: whole pieces behind the row end in the last block
  slices_b3_t200                more K-blocks than slices, slices cut across clip boundaries
  slices_b7_t250, _b3_t1000     slices of more than DEPTH = 3 blocks (the ring wraps), at least one across a clip boundary
  reduce_s1, s3, s7, s9         1, 3, 7, 9 slices (B * ceil(T / 16)): reduce waves with empty ranges, counts no multiple of 8
  set_neg, set_norm, set_band   negative lambd, normalised window, a band-limited bank (empty bands: loud log columns)
  entry_dev                     dmel_backward_fb_dev
  entry_saved                   dmel_backward_fb_saved on the spectrogram dmel_forward_dev_fixed_spec wrote
  entry_saved_dl_m64            dmel_backward_fb_saved_dl, d lambd in the same launch (M <= 128); d lambd against the fp64 dot
  entry_saved_dl_m130           ... two column tiles: d lambd from the stand-alone kernel
  entry_layer                   MelSpectrogramLayer(learnable_fb=True) after one optimiser step on the bank
  lengths_mixed                 dmel_backward_fb_dev_lengths and _saved_lengths: one launch with full length, one sample, Tc = 2, 3, 5, 6, 7,
                                16, 17 and clips whose last blocks are all pad, slices across such clips
  lengths_tiny                  the LEN build with T = 3
(every other case goes through dmel_backward_fb: host lambd, spectrogram recomputed)
"""
from __future__ import annotations

import functools

import numpy as np

from dmel_amd import synth
from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from tangent_cases import REF_BAR, synth_clips
from test_hip_parity import TOL, record_parity

EPS = 1e-10
BF, BM, KB, DEPTH, RED_WAVES = 64, 128, 16, 3, 8          # dmel_aux.hip: kFbgBF, kFbgBM, frames per K-block, ring depth, kFbgRedWaves


def _case(name, B, L, lambd, hop, n_mels, sr=16000, f_min=0.0, f_max=None, normalize_window=False, optimized=True, seed=0, entry="host",
          lengths=None, slices=None, splits=None, tone=0.05, noise=0.1):
    return dict(name=name, B=B, L=L, lambd=lambd, hop=hop, n_mels=n_mels, sr=sr, f_min=f_min, f_max=f_max, normalize_window=normalize_window,
                optimized=optimized, seed=seed, entry=entry, lengths=lengths, slices=slices, splits=splits, tone=tone, noise=noise)


def _hop_for(L, T):
    """the largest hop with L // hop + 1 == T"""
    for hop in range(L + 1, 0, -1):
        if L // hop + 1 == T:
            return hop
    raise ValueError((L, T))


def _len_T(hop, T):
    return hop * (T - 1) + max(1, hop // 3)


def _rows():
    out = []
    for i, (n, lam, sr, M, hop, T, B) in enumerate([(32, 5.0, 8000, 10, 16, 45, 3), (64, 9.0, 8000, 20, 40, 41, 3), (128, 20.0, 8000, 24, 50, 18, 3),
                                                    (256, 30.0, 22050, 48, 97, 23, 3), (1024, 150.0, 16000, 64, 100, 37, 3),
                                                    (2048, 260.0, 16000, 80, 333, 13, 3), (16384, 1700.0, 16000, 64, 4999, 5, 2)]):
        out.append(_case(f"rows_F{n // 2 + 1}", B, _len_T(hop, T), lam, hop, M, sr, seed=3000 + 10 * i))
    out.append(_case("rows_F1", 2, 500, 0.2, 16, 10, 8000, seed=3100))
    out.append(_case("rows_F2", 2, 501, 0.34, 16, 10, 8000, seed=3101))
    for j, (L, lam, M, norm) in enumerate([(63, 6.0, 12, False), (77, 9.0, 12, False), (127, 12.0, 16, True), (601, 50.0, 24, True), (1024, 70.0, 64, False)]):
        out.append(_case(f"full_L{L}", 2, L, lam, max(1, L // 5), M, 8000 if L < 1024 else 16000, normalize_window=norm, optimized=False, seed=3200 + j))
    return out


def _cols():
    out = [_case(f"cols_M{M}", 2, _len_T(50, 19), 20.0, 50, M, 8000, seed=3300 + M) for M in (1, 127, 128, 129, 130)]
    out.append(_case("cols_M512", 2, 3599, 128.0, 100, 512, seed=3390, tone=0.0))
    return out


def _ends():
    L = {33: 704}                                             # (no hop gives 33 frames on 700 samples)
    return [_case(f"ends_T{T}", 3, L.get(T, 700), 20.0, _hop_for(L.get(T, 700), T), 24, 8000, seed=3400 + T)
            for T in (1, 2, 3, 4, 5, 6, 7, 16, 17, 29, 32, 33)]


CASES = _rows() + _cols() + _ends() + [
    _case("slices_b3_t200", 3, _len_T(16, 200), 150.0, 16, 130, seed=3500, slices="more"),
    _case("slices_b7_t250", 7, _len_T(16, 250), 150.0, 16, 130, seed=3501, slices="deep"),
    _case("slices_b3_t1000", 3, _len_T(8, 1000), 150.0, 8, 130, seed=3502, slices="deep"),
    _case("reduce_s1", 1, _len_T(16, 16), 5.0, 16, 10, 8000, seed=3510, splits=1),
    _case("reduce_s3", 3, _len_T(16, 13), 5.0, 16, 10, 8000, seed=3511, splits=3),
    _case("reduce_s7", 7, _len_T(16, 9), 5.0, 16, 10, 8000, seed=3512, splits=7),
    _case("reduce_s9", 3, _len_T(16, 40), 5.0, 16, 10, 8000, seed=3513, splits=9),
    _case("set_neg", 2, _len_T(97, 21) + 1, -0.93 * 30.0, 97, 48, 22050, seed=3520),
    _case("set_norm", 2, _len_T(97, 21) + 2, 0.97 * 30.0, 97, 48, 22050, seed=3521, normalize_window=True),
    _case("set_band", 2, _len_T(97, 21) + 3, 30.0, 97, 48, 22050, seed=3522, f_min=125.0, f_max=0.4375 * 22050),
    _case("entry_dev", 3, _len_T(100, 37), 150.0, 100, 64, seed=3530, entry="dev"),
    _case("entry_saved", 3, _len_T(100, 38), 150.0, 100, 64, seed=3531, entry="saved"),
    _case("entry_saved_dl_m64", 3, _len_T(16, 200), 150.0, 16, 64, seed=3532, entry="saved_dl"),
    _case("entry_saved_dl_m130", 2, _len_T(100, 37), 150.0, 100, 130, seed=3533, entry="saved_dl"),
    _case("entry_layer", 3, _len_T(100, 39), 150.0, 100, 40, seed=3534, entry="layer"),
    # n_fft 2048 x 130 bands: 32 tiles, so that 12 clips of 3 K-blocks are more blocks than slices on 256 CUs (test_hip_fbgrad.py asserts
    # it on the device at hand).  hop 32, T = 41: Tc = 41 (full), 1 (one sample), 2, 3, 5, 6, 7, 16, 17, 33, then a full clip and Tc = 20.
    # A clip with Tc <= 16 / <= 32 has its last two / last K-block all pad: skipped inside the slices that span it.
    _case("lengths_mixed", 12, _len_T(32, 41), 260.0, 32, 130, seed=3540, entry="lengths",
          lengths=[_len_T(32, 41), 1, 40, 70, 130, 175, 200, 490, 515, 1030, _len_T(32, 41), 610]),
    _case("lengths_tiny", 4, _len_T(300, 3), 30.0, 300, 24, 22050, seed=3541, entry="lengths", lengths=[_len_T(300, 3), 1, 310, 599]),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def n_fft_of(case) -> int:
    return O.n_fft(case["lambd"]) if case["optimized"] else 2 * case["L"]


def n_time(case) -> int:
    return case["L"] // case["hop"] + 1


def grad_shape(case):
    return (n_fft_of(case) // 2 + 1, case["n_mels"])


def out_shape(case):
    return (case["B"], 1, case["n_mels"], n_time(case))


def frames_of(case):
    """frames per clip: T, or lengths[b] // hop + 1"""
    T = n_time(case)
    return [T] * case["B"] if case["lengths"] is None else [n // case["hop"] + 1 for n in case["lengths"]]


def expected_splits(case, cus: int) -> int:
    """dmel_aux.hip: fbgrad_splits restated -- min(2 CUs / tiles, B ceil(T / 16)), at least 1"""
    F, M = grad_shape(case)
    folds = F > BF and F % BF == 1
    tiles = (F // BF if folds else -(-F // BF)) * -(-M // BM)
    return max(1, min(2 * cus // tiles, case["B"] * -(-n_time(case) // KB)))


def slice_layout(case, splits: int):
    """(K-blocks of the largest slice, number of slices that hold blocks of two clips) for the static cuts of launch_fbgrad"""
    ntc = -(-n_time(case) // KB)
    total = case["B"] * ntc
    base, rem = divmod(total, splits)
    spans, lo = 0, 0
    for s in range(splits):
        n = base + (1 if s < rem else 0)
        if n > 0 and lo // ntc != (lo + n - 1) // ntc:
            spans += 1
        lo += n
    return base + (1 if rem else 0), spans


@functools.lru_cache(maxsize=None)
def _input(name):
    c = BY_NAME[name]
    x = synth_clips(c["B"], c["L"], c["seed"], c["sr"], c["tone"], c["noise"])
    if c["lengths"] is not None:
        # the mean of the clip's OWN samples removed (what the kernel subtracts is then tiny, as for the other cases); samples past the clip stay
        for b, n in enumerate(c["lengths"]):
            x[b, :n] -= np.float32(x[b, :n].astype(np.float64).mean())
    x.setflags(write=False)
    return x


def make_input(case) -> np.ndarray:
    """(B, L) fp32, read-only and shared"""
    return _input(case["name"])


@functools.lru_cache(maxsize=None)
def _cotangent(name):
    c = BY_NAME[name]
    g = synth.cotangent(out_shape(c), seed=c["seed"] + 11)
    g.setflags(write=False)
    return g


def make_cotangent(case) -> np.ndarray:
    """(B, 1, n_mels, T) fp32 signed normal, read-only and shared"""
    return _cotangent(case["name"])


def _kw(case):
    return dict(f_min=case["f_min"], f_max=case["f_max"], normalize_window=case["normalize_window"], optimized=case["optimized"],
                lengths=case["lengths"])


def fp64_with_out(case, out):
    """fbgrad_fp64 on the case's inputs with the saved log output `out` (None: the linear output)"""
    return R.fbgrad_fp64(make_input(case), case["lambd"], case["hop"], case["n_mels"], case["sr"], make_cotangent(case), out, **_kw(case))


@functools.lru_cache(maxsize=None)
def _fp64_lin(name):
    res = fp64_with_out(BY_NAME[name], None)
    for a in res:
        a.setflags(write=False)
    return res


def fp64_lin(case):
    """(grad_fb, scale) of the linear output, computed once per session and read-only"""
    return _fp64_lin(case["name"])


@functools.lru_cache(maxsize=None)
def _oracle_out(name):
    """the C oracle's log output (HTK bank) in the layout of out_shape, pad frames 0; None where it has no entry point (full window)"""
    c = BY_NAME[name]
    if not c["optimized"]:
        return None
    x = make_input(c)
    if c["lengths"] is None:
        out, _ = O.forward(x, c["lambd"], c["hop"], c["n_mels"], c["sr"], c["f_min"], c["f_max"], c["normalize_window"], apply_log=True,
                           eps=EPS, want_tangent=False)
    else:
        out = np.zeros(out_shape(c), np.float32)
        for b, n in enumerate(c["lengths"]):
            Tc = n // c["hop"] + 1
            if n == 1:
                out[b, :, :, :Tc] = np.float32(np.log(EPS))              # x - mean(x) = 0 exactly
                continue
            o, _ = O.forward(x[b:b + 1, :n], c["lambd"], c["hop"], c["n_mels"], c["sr"], c["f_min"], c["f_max"], c["normalize_window"],
                             apply_log=True, eps=EPS, want_tangent=False)
            out[b, :, :, :Tc] = o[0]
    out.setflags(write=False)
    return out


def cpu_log_out(case):
    """a saved log output for the pure CPU references: the oracle's, or None (the references then compute their own)"""
    return _oracle_out(case["name"])


def oracle(case, log, out=None):
    """O.backward_fb on the case's inputs (clip by clip with per-clip lengths), or None where the oracle has no entry point (full window)"""
    if not case["optimized"]:
        return None
    x, g = make_input(case), make_cotangent(case)
    if case["lengths"] is None:
        return O.backward_fb(x, case["lambd"], case["hop"], g, out if log else None, case["normalize_window"])
    ref = np.zeros(grad_shape(case), np.float64)
    for b, n in enumerate(case["lengths"]):
        Tc = n // case["hop"] + 1
        if n == 1:
            continue                                                      # a silent clip: spec == 0
        ref += O.backward_fb(x[b:b + 1, :n], case["lambd"], case["hop"], g[b:b + 1, :, :, :Tc], out[b:b + 1, :, :, :Tc] if log else None,
                             case["normalize_window"])
    return ref


def fbgrad_stats(got, ref, scale):
    """the comparison of the filterbank gradient `got` with `ref` against the cancellation-free magnitude `scale`, with nothing hidden;
    next to it the measure the suite used (one maximum over the largest element) and the share of the tensor that measure cannot see"""
    g, r, s = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, scale))
    assert g.shape == r.shape == s.shape, (g.shape, r.shape, s.shape)
    err = np.abs(g - r)
    pos = s > 0
    rel = np.zeros_like(err)
    rel[pos] = err[pos] / s[pos]
    rel[~np.isfinite(g)] = np.inf
    worst = int(rel.argmax()) if rel.size else 0
    top = float(np.abs(r).max()) + 1e-30 if r.size else 1.0
    return {"n": int(s.size), "max_err": float(rel.max()) if rel.size else 0.0, "worst_index": worst,
            "max_abs_where_scale_is_zero": float(np.abs(g[~pos]).max()) if (~pos).any() else 0.0,
            "global_max_measure": float(err.max()) / top if err.size else 0.0,
            "frac_below_tol_of_largest": float((np.abs(r) < TOL * top).mean()) if r.size else 0.0}


def assert_fbgrad(name, got, ref, scale, tol=TOL, shape=None):
    """|got - ref| / scale <= tol on every element with scale > 0 and got == 0 exactly elsewhere: no floor.  Recorded under ``name`` in the
    parity report."""
    st = fbgrad_stats(got, ref, scale)
    if shape is not None:
        st["worst_index"] = [int(v) for v in np.unravel_index(st["worst_index"], shape)]
    record_parity(name, st)
    assert st["max_abs_where_scale_is_zero"] == 0.0, (name, "an element that cannot be anything but zero is not zero", st)
    assert st["max_err"] <= tol, (name, "filterbank gradient error above the bar", st)
    return st
