"""The fp32 clip mean of models.py:38 as the kernels add it up, modelled in numpy -- both sides of the address dispatch.

The fused forward (csrc/dmel_fwd_body.inc, "short clips") and dmel_prep_kernel (csrc/dmel_fwd.hip) pick their loads by the clip's
address: a 16-byte aligned clip is read as float4 into FOUR accumulators per thread, any other clip as dwords into ONE (the fused
kernel) or into four strided ones (the prep kernel).  The order of the fp32 additions differs between the sides by design, so their
means may differ in the last ulp -- and on the DC-dominated fixtures (tests/golden/cases.py: DC_CASES) one ulp of the mean moves the
lowest mel bands by up to 3e-2.  tests/test_hip_addresses.py therefore asserts the g13 fixtures at misaligned addresses through
explain_by_clip_mean(max_ulps=2); that cap is a CONDITION on the summation order, checked here without a GPU: for every fp32 g13 clip,
every workgroup size the fused kernel is built with and both sides, the modelled mean lies within 2 ulp of the correctly rounded one
(dmel_kernels.h, "the clip mean": measured 0 or +-1 on the aligned side).

Orders restated (THREADS = 64 x waves, KB = 8 loads per thread and batch):
  aligned    thread tid adds float4 number q = tid, tid + THREADS, ... into (a0, a1, a2, a3) component-wise, the last L % 4 samples
             (tid + THREADS j past 4 (L / 4)) into a0; per thread (a0 + a1) + (a2 + a3)
  unaligned  thread tid adds samples tid, tid + THREADS, ... ascending into a0 alone
  then       wave_sum (dmel_wavefft.h): xor 1, xor 2, half-mirror, mirror inside each row of 16 lanes, (r0 + r1) + (r2 + r3) over the rows;
             the waves' sums pairwise (t[i] += t[i + st], st = 1, 2, 4, ...); mean_quotient: q = s * fl(1/L), one Newton step in fma.
  prep       (clips > 32768 samples) per chunk of `chunk` samples, 256 threads: aligned as above with float4 number tid + 256 u;
             unaligned acc_u += x[i + 256 u] for i = lo + tid, lo + tid + 1024, ..., the rest into acc0; the four accumulators, the
             64 lanes (xor butterfly) and the four waves in fp64, one rounding to fp32 per chunk; the forward adds the <= 64 chunk sums
             with wave_sum and divides with mean_quotient."""
from fractions import Fraction

import numpy as np
import pytest

import cases as C

F32 = np.float32
FP32_DC = [c for c in C.DC_CASES if c["dtype"] == "float32"]


def _wave_sum(v):
    """dmel_wavefft.h: wave_sum over (..., 64) fp32 lanes -> (...,)"""
    lane = np.arange(64)
    v = v.astype(F32)
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    v = v + v[..., (lane & ~7) | (7 - (lane & 7))]           # row_half_mirror
    v = v + v[..., (lane & ~15) | (15 - (lane & 15))]        # row_mirror
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _round_f32(fr):
    """a rational rounded to the nearest fp32 (no double rounding)"""
    c = F32(float(fr))
    best = c
    for cand in (np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))):
        if abs(Fraction(float(cand)) - fr) < abs(Fraction(float(best)) - fr):
            best = cand
    return F32(best)


def _fma(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _mean_quotient(s, L):
    """dmel_kernels.h: mean_quotient(sum, L, fl32(1 / L))"""
    inv, fl = F32(1.0) / F32(L), F32(L)
    q = F32(s) * inv
    return _fma(_fma(-q, fl, s), inv, q)


def _strided_chain(x, threads):
    """per thread: x[tid], x[tid + threads], ... added ascending into one fp32 accumulator -> (threads,)"""
    n = -(-len(x) // threads)
    pad = np.zeros(n * threads, F32)
    pad[:len(x)] = x
    acc = np.zeros(threads, F32)
    for row in pad.reshape(n, threads):
        acc = acc + row                                      # (a + 0.f is a)
    return acc


def _tree_over_waves(ws):
    t = list(ws)
    st = 1
    while st < len(t):
        for i in range(0, len(t), 2 * st):
            t[i] = F32(t[i] + t[i + st])
        st *= 2
    return t[0]


def fused_mean(x, threads, aligned):
    """the fused forward's own clip mean for one clip, at a 16-byte aligned address or at any other"""
    x = x.astype(F32)
    L = len(x)
    if aligned:
        n4 = L // 4
        a = [_strided_chain(x[c:4 * n4:4], threads) for c in range(4)]
        a[0] = a[0] + _strided_chain(x[4 * n4:], threads)
        per_thread = (a[0] + a[1]) + (a[2] + a[3])
    else:
        per_thread = _strided_chain(x, threads)              # (a0 + 0) + (0 + 0)
    ws = _wave_sum(per_thread.reshape(threads // 64, 64))
    return _mean_quotient(_tree_over_waves(ws), L)


def prep_chunk_sum(x, aligned):
    """dmel_prep_kernel: one chunk's sum, 256 threads, fp64 from the accumulators on"""
    x = x.astype(F32)
    n = len(x)
    if aligned:
        n4 = n // 4
        acc = [_strided_chain(x[c:4 * n4:4], 256) for c in range(4)]
        acc[0] = acc[0] + _strided_chain(x[4 * n4:], 256)
    else:
        acc = [np.zeros(256, F32) for _ in range(4)]
        full = (np.maximum(n - 768 - np.arange(256), 0) + 1023) // 1024        # rounds of four loads per thread: i + 768 < n
        rounds = int(full.max())
        tid = np.arange(256)
        for r in range(rounds):
            ok = r < full
            for u in range(4):
                idx = np.minimum(tid + 1024 * r + 256 * u, n - 1)
                acc[u] = acc[u] + np.where(ok, x[idx], F32(0))
        i = tid + 1024 * full
        while (i < n).any():
            acc[0] = acc[0] + np.where(i < n, x[np.minimum(i, n - 1)], F32(0))
            i = i + 256
    s = (acc[0].astype(np.float64) + acc[1].astype(np.float64)) + (acc[2].astype(np.float64) + acc[3].astype(np.float64))
    s = s.reshape(4, 64)
    lane = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        s = s + s[:, lane ^ m]
    return F32((s[0, 0] + s[1, 0]) + (s[2, 0] + s[3, 0]))


def prep_mean(x, aligned):
    """clips longer than 32768 samples: chunk sums from the prep kernel (dmel_plan_create's chunking), added by the forward's wave_sum"""
    L = len(x)
    nch = max(1, min((L + 4095) // 4096, 64))
    chunk = ((L + nch - 1) // nch + 3) // 4 * 4
    ps = np.zeros(64, F32)
    for c in range(nch):
        ps[c] = prep_chunk_sum(x[c * chunk:min((c + 1) * chunk, L)], aligned)
    return _mean_quotient(_wave_sum(ps), L)


def _ulps_off(mean, x):
    cr = F32(x.astype(np.float64).mean())
    return float((np.float64(mean) - np.float64(cr)) / np.spacing(np.abs(cr)))


def test_model_pieces():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(64).astype(F32)
    assert abs(float(_wave_sum(v)) - float(v.astype(np.float64).sum())) <= 1e-5
    assert _mean_quotient(F32(48000.0), 16000) == F32(3.0)
    assert _fma(F32(3.0), F32(5.0), F32(-15.0)) == F32(0.0)
    # exact data: every order gives the same, exact, mean
    x = (rng.integers(-8, 9, size=9001) * 0.125).astype(F32)
    exact = F32(x.astype(np.float64).mean())
    for threads in (256, 512, 1024):
        assert fused_mean(x, threads, True) == exact and fused_mean(x, threads, False) == exact
    x = (rng.integers(-8, 9, size=40000) * 0.125).astype(F32)
    assert prep_mean(x, True) == F32(x.astype(np.float64).mean()) == prep_mean(x, False)
    # the unaligned prep chains cover every sample exactly once, at lengths around the four-load rounds
    for n in (1, 255, 256, 769, 1024, 1025, 3999, 4000):
        y = np.ones(n, F32)
        assert prep_chunk_sum(y, False) == F32(n) == prep_chunk_sum(y, True)


@pytest.mark.parametrize("case", FP32_DC, ids=[c["name"] for c in FP32_DC])
def test_dc_dominated_means_stay_within_two_ulp_on_both_sides_of_the_address_dispatch(case):
    x = C.make_input(case).astype(F32)
    for b in range(case["B"]):
        for aligned in (True, False):
            if case["L"] > 32768:
                got = {"prep": prep_mean(x[b], aligned)}
            else:
                got = {threads: fused_mean(x[b], threads, aligned) for threads in (256, 512, 1024)}
            for how, m in got.items():
                off = _ulps_off(m, x[b])
                print(f"{case['name']} clip {b} {'aligned' if aligned else 'unaligned'} {how}: {off:+.0f} ulp from the correctly rounded mean")
                assert abs(off) <= 2.0, (case["name"], b, aligned, how, off)
