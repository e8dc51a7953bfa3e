"""Every kernel path that is chosen by the ADDRESS of a tensor, taken by tensors that are not 16-byte aligned.

The allocator hands out 512-byte aligned blocks, so every other GPU test gives the kernels aligned tensors; the kernels, however,
dispatch on `pointer & 15` (bf16 gradients: `& 7`) in eight places ("Address dispatch"): the clip mean of the
fused forward (scalar, multi-window, lengths and band-split builds), of dmel_prep_kernel and of the wave x-gradient kernel, the four
d lambd dot products, the x-gradient's combine, and the filterbank gradient's 16-byte loads that are declared 4-byte aligned.  Normal
use reaches the unaligned sides -- a contiguous view with a storage offset (a crop of a long recording), a slice of torch.cat's
gradient, a SlotInput cell, a C caller -- and here every one of them is run against the fp64 oracle.

`_placed(t, k)` is the tool: a contiguous copy of `t` that starts 4 + k elements into a NaN-filled buffer.  The NaN on both sides are
guards: a kernel that reads one element outside the tensor poisons a sum, and every test asserts finite results.  Comparisons use the
helpers and tolerances of test_hip_parity.py / test_hip_random_shapes.py unchanged; the one extra figure, 1e-6 |d| + 1e-12 between
the aligned and the unaligned run of a d lambd reduction, is the one tests/test_hip_band_split.py uses for two fp64 reductions that
partition the same sum differently.  Outputs at different k are NOT expected to be bit-equal (the clip mean adds in another order by
design, tests/test_clip_mean_orders_cpu.py); asserted instead: the same view twice gives the same bits, and a clip gives the same
bits wherever only the alignment class of its first sample is the same.

The C ABI's side of it (include/dmel.h, "Alignment"): what the library stores through must be 16-byte aligned, checked on the host;
the refusals and their messages are tested at the end.  No test launches a kernel with a misaligned output."""
import os

import numpy as np
import pytest
import torch

import cases as C
from oracle import dmel_oracle as O
from test_hip_parity import TOL, _gfb_err, _gx_err, _log_err, _rel_err, assert_parity, explain_by_clip_mean, record_parity
from test_hip_random_shapes import _assert_dlam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


def _placed(t, k):
    """`t` copied to element 4 + k of a NaN-filled flat buffer of t.numel() + 16 elements; returns the contiguous view"""
    t = t.detach()
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[4 + k:4 + k + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous()
    assert view.data_ptr() % 16 == (4 + k) * t.element_size() % 16
    return view


def _mk(case, log, sync=False, out_dtype=torch.float32, **kw):
    from dmel_amd import MelSpectrogramLayer
    return MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                               f_min=case["f_min"], f_max=case["f_max"], hop_length=case["hop"], device=DEV, optimized=case["optimized"],
                               normalize_window=case["normalize_window"], log=log, out_dtype=out_dtype, lambd_sync=sync, **kw).to(DEV)


def _oracle(case, x_np, log):
    return O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"],
                     apply_log=log, optimized=case["optimized"])


def _check_output(name, o, o_ref, log, plain):
    """every element against the oracle: the floored bars of test_hip_parity always, and -- where test_hip_random_shapes asserts it too
    (optimized=True, n_fft up to 16384) -- the plain relative error of every element without any floor"""
    assert np.isfinite(o).all(), name
    assert (_log_err(o, o_ref) if log else _rel_err(o, o_ref)) <= TOL, name
    if plain:
        if log:
            assert_parity("addresses/" + name + "/exp_logmel", np.exp(o.astype(np.float64)), np.exp(o_ref.astype(np.float64)), allow_floor=False)
        else:
            assert_parity("addresses/" + name + "/mel", o, o_ref, allow_floor=False)


def _cotangent(shape, seed):
    """The cotangent of every d lambd comparison here: synth.cotangent + 1.  d lambd = sum g t; with a zero-mean g it is a random-sign
    sum whose value can be 5e5 times below sum |g t| (oracle alone, n_fft 64, log output: |d| / sum |g t| = 1.9e-6), where the
    rounding of the fp32 tangent itself (3e-6 relative per element is enough) exceeds _dlam_tol on the ALIGNED control.  A cotangent
    with mean 1 -- what a loss such as y.sum() hands back -- keeps every sum here well conditioned (|d| / sum |g t| >= 3e-2 on the
    oracle), so that _dlam below can require the plain relative 1e-4 without the cancellation exemption."""
    from dmel_amd import synth
    return (synth.cotangent(tuple(shape), seed=seed) + np.float32(1.0)).astype(np.float32)


def _dlam(got_d, exp_d, g_np, t_ref, name):
    """_assert_dlam on a sum that is asserted (on the oracle alone) not to be cancellation-dominated: the plain 1e-4 is always in force"""
    cancel = float(np.abs(g_np.astype(np.float64) * t_ref.astype(np.float64)).sum())
    assert abs(exp_d) > 1e-3 * cancel, ("the cancellation exemption would be taken", name, exp_d, cancel)
    _assert_dlam(got_d, exp_d, g_np, t_ref, name)


def _bf16_np(a):
    """fp32 numpy values rounded to bf16 (as torch rounds), back in fp32"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF16).float().numpy()


# ---- a. forward with x at k = 0 (control), 1, 2, 3 ----------------------------------------------------------------------------------
# one configuration per route; clip lengths with L % 4 == 0 and != 0 so that the rows of a batch land in every alignment class;
# B T n_fft <= 6e6 each (the oracle stays in seconds)
FWD_CASES = [
    C._case("direct_dft_n16", 3, 1001, 8000, 2.0, 50, 10, seed=101),
    C._case("fused_n64", 3, 2001, 8000, 10.0, 32, 20, seed=102),
    C._case("fused_n512", 3, 4002, 16000, 80.0, 128, 64, seed=103, normalize_window=True),
    dict(C.BY_NAME["g2_c2"], name="fused_n1024_config2_b8"),
    C._case("fused_n2048", 2, 8003, 16000, 300.0, 256, 128, seed=104),
    C._case("fused_n4096", 2, 12001, 16000, 600.0, 600, 64, seed=105),
    C._case("fused_n16384", 2, 20002, 16000, -2500.0, 1000, 64, seed=106, normalize_window=True),
    C._case("prep_long_clip_L40001", 3, 40001, 16000, 128.0, 2000, 64, seed=107),      # rows at 0, 4, 8 bytes mod 16 when the base is aligned
    C._case("prep_long_clip_L40000", 2, 40000, 16000, 300.0, 2000, 40, seed=108),      # every chunk of every row in the base's class
    C._case("global_n32768", 2, 16001, 8000, 5000.0, 800, 64, seed=109),
    C._case("full_window_pow2_L1024", 3, 1024, 16000, 70.0, 128, 64, seed=110, optimized=False),
    C._case("full_window_chirpz_lds_L601", 3, 601, 8000, 50.0, 60, 24, seed=111, optimized=False, normalize_window=True),
    C._case("full_window_chirpz_split_L5001", 2, 5001, 8000, 700.0, 500, 40, seed=112, optimized=False),
    C._case("full_window_chirpz_global_L8193", 2, 8193, 16000, 1500.0, 800, 64, seed=113, optimized=False),
]
WITH_BF16 = {"fused_n512", "fused_n1024_config2_b8", "prep_long_clip_L40001"}


def _plain_bar(case):
    return case["optimized"] and O.n_fft(case["lambd"]) <= 16384


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c["name"] for c in FWD_CASES])
def test_forward_with_x_at_every_alignment(case, log):
    """training mode, no_grad, lambd_sync both ways, at k = 0 ... 3: output on every element and d lambd against the fp64 oracle; the
    same view twice gives the same bits; bf16 output (three routes) is the rounded fp32 output of the same view"""
    assert case["B"] * (case["L"] // case["hop"] + 1) * (O.n_fft(case["lambd"]) if case["optimized"] else 2 * case["L"]) <= 6_000_000
    x_np = C.make_input(case).astype(np.float32)
    g_np = _cotangent(C.out_shape(case), 1000 + case["seed"])
    o_ref, t_ref = _oracle(case, x_np, log)
    exp_d = O.backward(g_np, t_ref)
    x0 = torch.from_numpy(x_np).to(DEV)
    g = torch.from_numpy(g_np).to(DEV)
    layers = {sync: _mk(case, log, sync) for sync in (False, True)}
    bf = {sync: _mk(case, log, sync, out_dtype=BF16) for sync in (False, True)} if case["name"] in WITH_BF16 else {}
    g_bf = g.to(BF16)
    exp_d_bf = O.backward(_bf16_np(g_np), t_ref)
    for k in range(4):
        xk = _placed(x0, k)
        for sync, lay in layers.items():
            name = f"{case['name']}/k{k}/{'sync' if sync else 'dev'}"
            lay.lambd.grad = None
            y = lay(xk)
            (y * g).sum().backward()
            d = float(lay.lambd.grad)
            assert np.isfinite(d), name
            _check_output(name + "/train", y.detach().cpu().numpy(), o_ref, log, _plain_bar(case))
            _dlam(d, exp_d, g_np, t_ref, name)
            with torch.no_grad():
                yi = lay(xk)
            assert not yi.requires_grad
            _check_output(name + "/no_grad", yi.cpu().numpy(), o_ref, log, _plain_bar(case))
            # determinism: the same view again, the same bits
            lay.lambd.grad = None
            y2 = lay(xk)
            (y2 * g).sum().backward()
            assert torch.equal(y2, y) and float(lay.lambd.grad) == d, name
            with torch.no_grad():
                assert torch.equal(lay(xk), yi), name
            if bf:
                lb = bf[sync]
                lb.lambd.grad = None
                yb = lb(xk)
                assert yb.dtype == BF16 and torch.equal(yb.view(torch.int16), y.detach().to(BF16).view(torch.int16)), name
                yb.backward(g_bf)
                db = float(lb.lambd.grad)
                assert np.isfinite(db)
                _dlam(db, exp_d_bf, _bf16_np(g_np), t_ref, name + "/bf16")
                with torch.no_grad():
                    assert torch.equal(lb(xk).view(torch.int16), yi.to(BF16).view(torch.int16)), name
            assert lay.lambd_status()["error"] == 0


@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
def test_forward_lengths_with_x_at_every_alignment(log):
    """forward(x, lengths) at partial lengths (dmel_fwd_len_kernel: every sum stops at the clip's own length), clip by clip against the
    oracle at that length; the pad frames keep their value; NaN behind a clip's end and around the batch reach nothing"""
    case = C._case("lengths_n1024", 4, 8001, 16000, 128.0, 256, 64, seed=120)
    B, L, hop, M, T = case["B"], case["L"], case["hop"], case["n_mels"], case["L"] // case["hop"] + 1
    lens = [8001, 5002, 3333, 1]
    x_np = C.make_input(case).astype(np.float32)
    g_np = _cotangent(C.out_shape(case), 1000 + case["seed"])
    pad = np.float32(np.log(np.float32(1e-10))) if log else np.float32(0.0)
    o_ref = np.full((B, 1, M, T), pad, np.float32)
    t_ref = np.zeros((B, 1, M, T), np.float32)
    for b, lc in enumerate(lens):
        ob, tb = O.forward(x_np[b:b + 1, :lc], case["lambd"], hop, M, case["sr"], apply_log=log)
        o_ref[b, :, :, :lc // hop + 1], t_ref[b, :, :, :lc // hop + 1] = ob[0], tb[0]
    exp_d = O.backward(g_np, t_ref)
    xm = x_np.copy()
    for b, lc in enumerate(lens):
        xm[b, lc:] = np.nan                                     # what lies behind a clip is never read
    x0 = torch.from_numpy(xm).to(DEV)
    g = torch.from_numpy(g_np).to(DEV)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for sync in (False, True):
        lay = _mk(case, log, sync)
        # a pad frame is a frame of a silent clip through the same kernels (tests/test_hip_lengths.py), in the kernel's own log
        full = torch.full((B,), L, dtype=torch.int32, device=DEV)
        silent = lay(torch.zeros((B, L), device=DEV), full).detach().cpu().numpy()
        with torch.no_grad():
            silent_inf = lay(torch.zeros((B, L), device=DEV), full).cpu().numpy()
        assert np.abs(silent - o_ref[3, 0, 0, -1]).max() <= TOL and np.abs(silent_inf - o_ref[3, 0, 0, -1]).max() <= TOL
        for k in range(4):
            xk = _placed(x0, k)
            name = f"lengths/k{k}/{'sync' if sync else 'dev'}"
            lay.lambd.grad = None
            y = lay(xk, lengths)
            (y * g).sum().backward()
            d = float(lay.lambd.grad)
            o = y.detach().cpu().numpy()
            assert np.isfinite(o).all() and np.isfinite(d), name
            for b, lc in enumerate(lens):
                tc = lc // hop + 1
                _check_output(f"{name}/clip{b}", o[b:b + 1, :, :, :tc], o_ref[b:b + 1, :, :, :tc], log, True)
                assert np.array_equal(o[b, :, :, tc:], silent[b, :, :, tc:]), (name, b)
            _dlam(d, exp_d, g_np, t_ref, name)
            with torch.no_grad():
                yi = lay(xk, lengths)
            oi = yi.cpu().numpy()
            assert np.isfinite(oi).all()
            for b, lc in enumerate(lens):
                tc = lc // hop + 1
                _check_output(f"{name}/no_grad/clip{b}", oi[b:b + 1, :, :, :tc], o_ref[b:b + 1, :, :, :tc], log, True)
                assert np.array_equal(oi[b, :, :, tc:], silent_inf[b, :, :, tc:]), (name, b)
            lay.lambd.grad = None
            y2 = lay(xk, lengths)
            (y2 * g).sum().backward()
            assert torch.equal(y2, y) and float(lay.lambd.grad) == d


MULTI_LAMS = [300.0, 128.0, 40.0]          # n_fft 2048, 1024, 256: three launches


@pytest.mark.parametrize("which", ["multi_window", "band_split"])
@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
def test_multi_window_and_band_split_with_x_at_every_alignment(which, log):
    from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram
    B, L, sr, hop, M = 3, 8002, 16000, 200, 48
    T = L // hop + 1
    edges = [0, 5, 30, 48]
    case = C._case(which, B, L, sr, 0.0, hop, M, seed=130)
    x_np = C.make_input(case).astype(np.float32)
    K = len(MULTI_LAMS)
    refs = [O.forward(x_np, lam, hop, M, sr, apply_log=log) for lam in MULTI_LAMS]
    x0 = torch.from_numpy(x_np).to(DEV)
    band = which == "band_split"
    from dmel_amd import synth
    g_np = _cotangent((B, 1 if band else K, M, T), 131)
    g = torch.from_numpy(g_np).to(DEV)
    for sync in (False, True):
        if band:
            lay = BandSplitMelSpectrogram(MULTI_LAMS, M, L, sr, hop_length=hop, band_edges=edges, log=log, lambd_sync=sync).to(DEV)
        else:
            lay = MultiWindowMelSpectrogram(MULTI_LAMS, M, L, sr, hop_length=hop, log=log, lambd_sync=sync).to(DEV)
        for k in range(4):
            xk = _placed(x0, k)
            name = f"{which}/k{k}/{'sync' if sync else 'dev'}"
            lay.lambd.grad = None
            y = lay(xk)
            (y * g).sum().backward()
            with torch.no_grad():
                yi = lay(xk)
            o, oi, dl = y.detach().cpu().numpy(), yi.cpu().numpy(), lay.lambd.grad.cpu().numpy()
            assert np.isfinite(o).all() and np.isfinite(oi).all() and np.isfinite(dl).all(), name
            for c, (o_ref, t_ref) in enumerate(refs):
                if band:
                    lo, hi = edges[c], edges[c + 1]
                    got, goti, ref = o[:, :, lo:hi], oi[:, :, lo:hi], o_ref[:, :, lo:hi]
                    gk = np.zeros_like(g_np)
                    gk[:, :, lo:hi] = g_np[:, :, lo:hi]
                else:
                    got, goti, ref = o[:, c:c + 1], oi[:, c:c + 1], o_ref
                    gk = np.ascontiguousarray(g_np[:, c:c + 1])
                _check_output(f"{name}/c{c}/train", got, ref, log, True)
                _check_output(f"{name}/c{c}/no_grad", goti, ref, log, True)
                _dlam(float(dl[c]), O.backward(gk, t_ref), gk, t_ref, f"{name}/c{c}")
            lay.lambd.grad = None
            y2 = lay(xk)
            (y2 * g).sum().backward()
            assert torch.equal(y2, y) and torch.equal(lay.lambd.grad.cpu(), torch.from_numpy(dl)), name
            for c in range(K):
                assert lay.lambd_status(channel=c)["error"] == 0


def test_dspec_layer_with_x_at_every_alignment():
    """SpectrogramLayer(optimized=False): n_fft = 2 L with the half-length window, a power-of-two length (fused kernel, spectrogram
    mode) and one that is not (chirp-z); bars as test_dspec_layer_matches_reference_and_oracle"""
    from dmel_amd import SpectrogramLayer, synth
    for L, hop, lam, norm, floor in ((1024, 64, 90.0, True, 1e-6), (77, 5, 9.0, True, 1e-5)):
        x_np = synth.waveforms(3, L, seed=L, scale=1.0)
        rs, rt = O.dspec(x_np, lam, hop=hop, normalize_window=norm)
        g_np = _cotangent(rs.shape, L + 1)
        ref_d = O.backward(g_np, rt)
        g = torch.from_numpy(g_np).to(DEV)
        x0 = torch.from_numpy(x_np).to(DEV)
        for sync in (False, True):
            lay = SpectrogramLayer(torch.tensor(lam), optimized=False, hop_length=hop, normalize_window=norm, lambd_sync=sync).to(DEV)
            for k in range(4):
                xk = _placed(x0, k)
                lay.lambd.grad = None
                s = lay(xk)
                (s * g).sum().backward()
                o, d = s.detach().cpu().numpy(), float(lay.lambd.grad)
                assert o.shape == rs.shape and np.isfinite(o).all() and np.isfinite(d)
                assert _rel_err(o, rs, floor=floor) <= TOL, (L, k, sync)
                _dlam(d, ref_d, g_np, rt, f"dspec/L{L}/k{k}")
                with torch.no_grad():
                    si = lay(xk)
                assert _rel_err(si.cpu().numpy(), rs, floor=floor) <= TOL
                lay.lambd.grad = None
                s2 = lay(xk)
                (s2 * g).sum().backward()
                assert torch.equal(s2, s) and float(lay.lambd.grad) == d


@pytest.mark.parametrize("L,lam,hop", [(4001, 80.0, 128), (40001, 128.0, 2000)], ids=["in_kernel_mean", "prep_kernel_partial_sums"])
def test_class_equality_of_a_clip_at_equal_alignment(L, lam, hop):
    """Where only the alignment CLASS of a clip's first sample matters, the bits are equal: clip data D alone at k = 1, and D as row 1 of
    an ALIGNED batch with L % 4 == 1 (4 bytes past a 16-byte boundary either way).  Row 1 of an aligned batch is what the existing
    oracle tests already cover (ragged lengths), so this ties the misaligned base address to tested ground.  D carries an offset 500 x
    its signal: the last ulp of its mean shows in the lowest bands, a different summation order would too.  (The prep route: every
    chunk is a multiple of 4 samples long, dmel_plan_create.)"""
    from dmel_amd import synth
    assert L % 4 == 1
    sr, M = 16000, 64
    case = C._case("class_eq", 2, L, sr, lam, hop, M, seed=140)
    d_np = (0.5 + 1e-3 * synth.waveforms(1, L, seed=141, scale=1.0)).astype(np.float32)
    z_np = synth.waveforms(1, L, seed=142)
    alone = _placed(torch.from_numpy(d_np).to(DEV), 1)
    batch = torch.from_numpy(np.concatenate([z_np, d_np])).to(DEV)
    swapped = _placed(torch.from_numpy(np.concatenate([d_np, z_np])).to(DEV), 1)       # the same batch size: D in class 1 as row 0
    assert batch.data_ptr() % 16 == 0 and (batch.data_ptr() + 4 * L) % 16 == 4 == alone.data_ptr() % 16 == swapped.data_ptr() % 16
    for log in (False, True):
        for sync in (False, True):
            lay = _mk(case, log, sync)
            ya, yb, ys = lay(alone), lay(batch), lay(swapped)
            assert torch.isfinite(ya).all() and torch.isfinite(yb).all()
            assert torch.equal(ys[0], yb[1]), ("train, same batch size", log, sync)
            assert torch.equal(ya[0], yb[1]), ("train", log, sync)
            with torch.no_grad():
                assert torch.equal(lay(swapped)[0], lay(batch)[1]), ("no_grad, same batch size", log, sync)
                assert torch.equal(lay(alone)[0], lay(batch)[1]), ("no_grad", log, sync)


# ---- d. DC-dominated clips ----------------------------------------------------------------------------------------------------------
FP32_DC = [c for c in C.DC_CASES if c["dtype"] == "float32"]


@pytest.mark.parametrize("case", FP32_DC, ids=[c["name"] for c in FP32_DC])
def test_dc_dominated_fixtures_with_x_at_every_alignment(case):
    """the fp32 g13_dc_* fixtures at k = 1, 2, 3 through explain_by_clip_mean, unchanged, at max_ulps = 2: per clip and on every
    element the kernel is the reference's path at a mean within two ulp of the correctly rounded one.  That the unaligned summation
    order stays inside that cap is shown without a GPU by tests/test_clip_mean_orders_cpu.py."""
    from test_oracle_golden import dc_reference_input
    from test_hip_parity import _dlam_tol
    gold = C.load(case)
    x_np = C.make_input(case)
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to(DEV)
    exp = gold["mel"].astype(np.float64)
    xin, mean_ref = dc_reference_input(case, gold)
    mean_cr = np.float32(x_np.astype(np.float64).mean(1))
    x0 = torch.from_numpy(x_np).to(DEV)
    for k in (1, 2, 3):
        xk = _placed(x0, k)
        for log in (False, True):
            e = 1e-10 if log else 0.0
            layer = _mk(case, log)
            assert layer.n_fft() == int(gold["n_fft"])
            out = layer(xk)
            (out * g).sum().backward()
            got = out.detach().cpu().numpy().astype(np.float64)
            got_d = float(layer.lambd.grad)
            assert np.isfinite(got).all() and np.isfinite(got_d)
            lin = np.exp(got) if log else got
            used, mean_used, rel_fix = explain_by_clip_mean(case, gold, lin, e, xin, mean_ref, mean_cr, max_ulps=2)
            record_parity(f"addresses/golden/{case['name']}/k{k}" + ("/exp_logmel" if log else "/mel"),
                          {"n": int(exp.size), "plain_max_rel_vs_fixture": float(rel_fix.max()),
                           "kernel_mean_ulps_from_correctly_rounded": [int(v) for v in used]})
            _, t_ref = O.forward(xin, case["lambd"], case["hop"], case["n_mels"], case["sr"], apply_log=log, mean=mean_used)
            same = bool((mean_used == mean_ref).all())
            exp_d = float(gold["dlam_log" if log else "dlam_lin"]) if same else O.backward(g_np, t_ref)
            assert abs(got_d - exp_d) <= _dlam_tol(exp_d, g_np, t_ref), (case["name"], k, log, got_d, exp_d)


# ---- b. grad_out at k = 1, 2, 3 (fp32) and 1 ... 4 (bf16) -----------------------------------------------------------------------------
def _close_to_aligned(d, d0):
    """two fp64 reductions that partition the same sum differently (tests/test_hip_band_split.py)"""
    return abs(d - d0) <= 1e-6 * abs(d0) + 1e-12


def _ks(dtype):
    return (1, 2, 3) if dtype == torch.float32 else (1, 2, 3, 4)


def _backward_with(y, gk, seen):
    h = y.register_hook(lambda gr: seen.append((gr.data_ptr() % 16, gr.is_contiguous(), gr.data_ptr())))
    y.backward(gk)
    h.remove()


# T % 4 == 0 (the address alone selects the scalar side), and one T % 4 != 0
DOT_SHAPES = [(3, 3900, 100, 48), (3, 4000, 100, 48)]


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,hop,M", DOT_SHAPES, ids=["T40", "T41"])
def test_scalar_dot_with_grad_out_at_every_alignment(B, L, hop, M, dtype):
    """dmel_dot_kernel<GBF16, false> by torch.ops.dmel (the layer's C++ autograd node) and by Plan.backward with accumulate; also the
    TANGENT placed (the kernel dispatches on both addresses; a C caller may have moved it)"""
    from dmel_amd import capi
    sr, lam = 16000, 128.0
    case = C._case("dot", B, L, sr, lam, hop, M, seed=150)
    T = L // hop + 1
    x_np = C.make_input(case).astype(np.float32)
    g_np = _cotangent(C.out_shape(case), 1000 + case["seed"])
    if dtype == BF16:
        g_np = _bf16_np(g_np)
    x = torch.from_numpy(x_np).to(DEV)
    g = torch.from_numpy(g_np).to(DEV).to(dtype)
    for log in (False, True):
        _, t_ref = _oracle(case, x_np, log)
        exp_d = O.backward(g_np, t_ref)
        lay = _mk(case, log, out_dtype=dtype)
        y = lay(x)
        y.backward(g)
        d0 = float(lay.lambd.grad)
        _dlam(d0, exp_d, g_np, t_ref, "aligned")
        for k in _ks(dtype):
            gk = _placed(g, k)
            seen = []
            lay.lambd.grad = None
            _backward_with(lay(x), gk, seen)
            d = float(lay.lambd.grad)
            assert seen == [(gk.data_ptr() % 16, True, gk.data_ptr())], "the gradient did not reach the node as the placed view"
            assert np.isfinite(d)
            _dlam(d, exp_d, g_np, t_ref, f"dot/{dtype}/k{k}")
            assert _close_to_aligned(d, d0), (k, d, d0)
        # the C ABI: dmel_backward(_ex) on the plan's own scratch, then a second call that accumulates onto the first
        plan = capi.Plan(L, hop, M, sr)
        st = torch.cuda.current_stream().cuda_stream
        out, tan = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
        plan.forward(x.data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), log, 1e-10, st)
        for k in _ks(dtype):
            for gk, tk in ((_placed(g, k), tan), (g, _placed(tan, min(k, 3))), (_placed(g, k), _placed(tan, 4 - min(k, 3)))):
                dl = torch.full((1,), float("nan"), device=DEV)
                plan.backward(gk.data_ptr(), tk.data_ptr(), g.numel(), dl.data_ptr(), st, grad_bf16=dtype == BF16)
                once = dl.clone()
                plan.backward(gk.data_ptr(), tk.data_ptr(), g.numel(), dl.data_ptr(), st, accumulate=True, grad_bf16=dtype == BF16)
                torch.cuda.synchronize()
                d = float(once)
                assert np.isfinite(d)
                _dlam(d, exp_d, g_np, t_ref, f"dot/capi/{dtype}/k{k}")
                assert _close_to_aligned(d, d0), (k, d, d0)
                assert torch.allclose(dl, 2 * once, rtol=2.0 ** -22, atol=0.0), (dl, once)     # (fp64 total added to the fp32 value, rounded once)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,hop,M", DOT_SHAPES, ids=["T40", "T41"])
@pytest.mark.parametrize("which", ["multi_window", "band_split"])
def test_multi_and_band_dot_with_grad_out_at_every_alignment(which, B, L, hop, M, dtype):
    """dmel_dot_multi_kernel (per_row = M T) and dmel_dot_band_kernel (uneven edges), fp32 and bf16 gradients"""
    from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram, synth
    sr = 16000
    T = L // hop + 1
    edges = [0, 5, 30, 48]
    K = len(MULTI_LAMS)
    band = which == "band_split"
    x_np = synth.waveforms(B, L, seed=160)
    g_np = _cotangent((B, 1 if band else K, M, T), 161)
    if dtype == BF16:
        g_np = _bf16_np(g_np)
    x = torch.from_numpy(x_np).to(DEV)
    g = torch.from_numpy(g_np).to(DEV).to(dtype)
    refs = [O.forward(x_np, lam, hop, M, sr, apply_log=True)[1] for lam in MULTI_LAMS]
    if band:
        lay = BandSplitMelSpectrogram(MULTI_LAMS, M, L, sr, hop_length=hop, band_edges=edges, log=True, out_dtype=dtype).to(DEV)
    else:
        lay = MultiWindowMelSpectrogram(MULTI_LAMS, M, L, sr, hop_length=hop, log=True, out_dtype=dtype).to(DEV)
    lay(x).backward(g)
    d0 = lay.lambd.grad.cpu().numpy().astype(np.float64)
    for k in _ks(dtype):
        gk = _placed(g, k)
        seen = []
        lay.lambd.grad = None
        _backward_with(lay(x), gk, seen)
        assert seen == [(gk.data_ptr() % 16, True, gk.data_ptr())]
        dl = lay.lambd.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(dl).all()
        for c, t_ref in enumerate(refs):
            if band:
                gc = np.zeros_like(g_np)
                gc[:, :, edges[c]:edges[c + 1]] = g_np[:, :, edges[c]:edges[c + 1]]
            else:
                gc = np.ascontiguousarray(g_np[:, c:c + 1])
            _dlam(float(dl[c]), O.backward(gc, t_ref), gc, t_ref, f"{which}/{dtype}/k{k}/c{c}")
            assert _close_to_aligned(float(dl[c]), float(d0[c])), (k, c, dl[c], d0[c])


@pytest.mark.parametrize("B,L,hop,M", DOT_SHAPES, ids=["T40", "T41"])
def test_trainable_filterbank_step_with_grad_out_at_every_alignment(B, L, hop, M):
    """lambd AND the filterbank trained: d lambd rides in the filterbank gradient's launch (fbgrad_dot_body, dmel_backward_fb_saved_dl),
    and that launch reads grad_out with 16-byte loads declared 4-byte aligned (f4u)"""
    sr, lam = 16000, 128.0
    case = C._case("fbstep", B, L, sr, lam, hop, M, seed=170)
    x_np = C.make_input(case).astype(np.float32)
    g_np = _cotangent(C.out_shape(case), 1000 + case["seed"])
    x = torch.from_numpy(x_np).to(DEV)
    g = torch.from_numpy(g_np).to(DEV)
    for log in (False, True):
        _, t_ref = _oracle(case, x_np, log)
        exp_d = O.backward(g_np, t_ref)
        lay = _mk(case, log, learnable_fb=True)
        y = lay(x)
        y.backward(g)
        d0, fb0 = float(lay.lambd.grad), lay.mel_fb.grad.clone()
        ref_fb = O.backward_fb(x_np, lam, hop, g_np, y.detach().cpu().numpy() if log else None)
        assert _gfb_err(fb0.cpu().numpy(), ref_fb) <= TOL
        for k in (1, 2, 3):
            for xk in (x, _placed(x, k)):
                gk = _placed(g, k)
                seen = []
                lay.lambd.grad = None
                lay.mel_fb.grad = None
                _backward_with(lay(xk), gk, seen)
                assert seen == [(gk.data_ptr() % 16, True, gk.data_ptr())]
                d, gfb = float(lay.lambd.grad), lay.mel_fb.grad.cpu().numpy()
                assert np.isfinite(d) and np.isfinite(gfb).all()
                _dlam(d, exp_d, g_np, t_ref, f"fbstep/k{k}")
                assert _close_to_aligned(d, d0), (k, d, d0)
                assert _gfb_err(gfb, ref_fb) <= TOL
                if xk is x:
                    assert torch.equal(lay.mel_fb.grad, fb0)           # the GEMM's order does not hang on the address


def test_a_slice_of_the_gradient_of_torch_cat_arrives_misaligned():
    """The route: two layers' outputs concatenated for a joint loss.  The second layer receives a narrow slice of the joint gradient,
    contiguous, wherever the first output's element count put it -- an odd count here."""
    sr = 16000
    c1 = C._case("cat1", 1, 4000, sr, 40.0, 100, 7, seed=180)
    c2 = C._case("cat2", 1, 4000, sr, 128.0, 100, 48, seed=180)
    x_np = C.make_input(c1).astype(np.float32)
    x = torch.from_numpy(x_np).to(DEV)
    l1, l2 = _mk(c1, True), _mk(c2, True)
    y1, y2 = l1(x), l2(x)
    n1 = y1.numel()
    assert n1 % 2 == 1
    from dmel_amd import synth
    w_np = _cotangent((n1 + y2.numel(),), 181)
    w = torch.from_numpy(w_np).to(DEV)
    seen = []
    y2.register_hook(lambda gr: seen.append((gr.data_ptr() % 16, gr.is_contiguous())))
    (torch.cat([y1.flatten(), y2.flatten()]) * w).sum().backward()
    g1, g2 = w_np[:n1].reshape(y1.shape), w_np[n1:].reshape(y2.shape)
    arrived = seen == [((4 * n1) % 16, True)]
    print(f"torch.cat backward: grad of y2 arrived with (data_ptr % 16, contiguous) = {seen}; misaligned slice: {arrived}")
    if not arrived:
        # this torch build copies the slice: the same check rests on the placed gradient
        print("torch.cat's backward copied the slice; falling back to y.backward(_placed(g, 3))")
        l2.lambd.grad = None
        l2(x).backward(_placed(torch.from_numpy(g2).to(DEV), 3))
    else:
        assert seen[0][0] != 0
    for lay, case, gg in ((l1, c1, g1), (l2, c2, g2)):
        _, t_ref = _oracle(case, x_np, True)
        d = float(lay.lambd.grad)
        assert np.isfinite(d)
        _dlam(d, O.backward(np.ascontiguousarray(gg), t_ref), np.ascontiguousarray(gg), t_ref, case["name"])


# ---- c. optional gradients with x and grad_out both placed ----------------------------------------------------------------------------
XG_CASES = [
    C._case("xg_wave_n128", 2, 4001, 8000, 13.0, 80, 40, seed=190),
    C._case("xg_wave_n1024", 2, 8002, 16000, 128.0, 256, 64, seed=191),
    C._case("xg_wave_n2048", 2, 8003, 16000, 300.0, 300, 64, seed=192, normalize_window=True),
    C._case("xg_lds_n4096", 1, 12001, 16000, 600.0, 600, 40, seed=193),
]


@pytest.mark.parametrize("case", XG_CASES, ids=[c["name"] for c in XG_CASES])
def test_waveform_and_filterbank_gradients_with_x_and_grad_out_placed(case):
    """x.grad (wave kernels up to n_fft 2048 with their own clip mean, the LDS kernels beyond) against O.backward_x, and
    dmel_backward_fb (f4u loads of grad_out and of the saved output at a misaligned base) against O.backward_fb, log and linear"""
    from dmel_amd import capi
    x_np = C.make_input(case).astype(np.float32)
    g_np = _cotangent(C.out_shape(case), 1000 + case["seed"])
    x0 = torch.from_numpy(x_np).to(DEV)
    g0 = torch.from_numpy(g_np).to(DEV)
    n = capi.n_fft(case["lambd"])
    st = torch.cuda.current_stream().cuda_stream
    for log in (False, True):
        for sync in (False, True):
            lay = _mk(case, log, sync)
            for k in (0, 1, 2, 3):
                xk = _placed(x0, k).requires_grad_(True)
                gk = _placed(g0, (k + 1) % 4)
                lay.lambd.grad = None
                y = lay(xk)
                y.backward(gk)
                gx = xk.grad.cpu().numpy()
                y_np = y.detach().cpu().numpy()
                assert np.isfinite(gx).all() and np.isfinite(float(lay.lambd.grad))
                ref_x = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y_np if log else None, case["f_min"], case["f_max"],
                                     case["normalize_window"])
                assert _gx_err(gx, ref_x) <= TOL, (case["name"], log, sync, k)
                assert float(np.abs(gx.sum(1)).max()) <= 1e-4 * float(np.abs(gx).sum(1).max())      # the adjoint of the DC removal
                if sync:
                    continue
                plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
                yk = _placed(y.detach(), (k + 2) % 4) if log else None
                gfb = torch.full((n // 2 + 1, case["n_mels"]), float("nan"), device=DEV)
                plan.backward_fb(xk.detach().data_ptr(), case["B"], case["lambd"], gk.data_ptr(), yk.data_ptr() if log else None, gfb.data_ptr(),
                                 log, st)
                torch.cuda.synchronize()
                ref_fb = O.backward_fb(x_np, case["lambd"], case["hop"], g_np, y_np if log else None, case["normalize_window"])
                got = gfb.cpu().numpy()
                assert np.isfinite(got).all() and _gfb_err(got, ref_fb) <= TOL, (case["name"], log, k)


def test_multi_window_waveform_gradient_with_x_and_grad_out_placed():
    from dmel_amd import MultiWindowMelSpectrogram, synth
    B, L, sr, hop, M = 2, 8002, 16000, 200, 48
    T = L // hop + 1
    lams = [700.0, 128.0, 40.0]                     # n_fft 4096 (LDS path: staged rows), 1024, 256 (wave kernels)
    x_np = synth.waveforms(B, L, seed=200)
    g_np = synth.cotangent((B, len(lams), M, T), seed=201)
    x0, g0 = torch.from_numpy(x_np).to(DEV), torch.from_numpy(g_np).to(DEV)
    for log in (False, True):
        lay = MultiWindowMelSpectrogram(lams, M, L, sr, hop_length=hop, log=log, waveform_grad=True).to(DEV)
        for k in (0, 1, 2, 3):
            xk = _placed(x0, k).requires_grad_(True)
            lay.lambd.grad = None
            y = lay(xk)
            y.backward(_placed(g0, (k + 1) % 4))
            y_np = y.detach().cpu().numpy()
            ref = sum(O.backward_x(x_np, lam, hop, sr, np.ascontiguousarray(g_np[:, c:c + 1]),
                                   np.ascontiguousarray(y_np[:, c:c + 1]) if log else None) for c, lam in enumerate(lams))
            gx = xk.grad.cpu().numpy()
            assert np.isfinite(gx).all() and torch.isfinite(lay.lambd.grad).all()
            assert _gx_err(gx, ref) <= TOL, (log, k)


@pytest.mark.parametrize("name", ["g7_mel_nonopt_256", "g7_mel_nonopt_601"])
def test_full_window_waveform_gradient_with_x_and_grad_out_placed(name):
    """optimized=False (n_fft = 2 L; 601 samples: chirp-z round trips) against torch autograd through the reference (g10_xgrad_g7_*.npz)"""
    case = C.BY_NAME[name]
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g10_xgrad_{name}.npz"))
    x0 = torch.from_numpy(C.make_input(case).astype(np.float32)).to(DEV)
    g0 = torch.from_numpy(C.make_cotangent(case)).to(DEV)
    for log, key in ((False, "gx_lin"), (True, "gx_log")):
        layer = _mk(case, log)
        for k in (0, 1, 2, 3):
            xk = _placed(x0, k).requires_grad_(True)
            layer.lambd.grad = None
            layer(xk).backward(_placed(g0, (k + 1) % 4))
            gx = xk.grad.cpu().numpy()
            n = gold[key].shape[0]
            assert np.isfinite(gx).all() and _gx_err(gx[:n], gold[key].astype(np.float64)) <= TOL, (name, log, k)
            assert np.isfinite(float(layer.lambd.grad))


def test_dspec_waveform_gradient_with_x_and_grad_out_placed():
    from dmel_amd import SpectrogramLayer, synth
    for L, fixture in ((128, "g7_dspec_xgrad.npz"), (100, "g7_dspec_xgrad_100.npz")):
        gold = np.load(os.path.join(os.path.dirname(C.__file__), fixture))
        x0 = torch.from_numpy(synth.waveforms(2, L, seed=77, scale=1.0)).to(DEV)
        lay = SpectrogramLayer(torch.tensor(6.38), optimized=False, hop_length=1).to(DEV)
        for k in (0, 1, 2, 3):
            xk = _placed(x0, k).requires_grad_(True)
            lay.lambd.grad = None
            s = lay(xk)
            g0 = torch.from_numpy(synth.cotangent(tuple(s.shape), seed=78)).to(DEV)
            s.backward(_placed(g0, (k + 1) % 4))
            gx = xk.grad.cpu().numpy()
            assert np.isfinite(gx).all() and _gx_err(gx, gold["gx"].astype(np.float64)) <= TOL, (L, k)
            assert np.isfinite(float(lay.lambd.grad))


# ---- e. SlotInput and GraphedStep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam0,L", [(10.0, 4001), (128.0, 16000), (300.0, 8003), (128.0, 40001), (5000.0, 16001), (2.0, 2001)],
                         ids=["n64", "n1024", "n2048", "prep_long_clip", "global_n32768", "direct_dft"])
def test_a_cell_with_a_misaligned_address_gives_the_bits_of_the_view(lam0, L):
    from dmel_amd import MelSpectrogramLayer, SlotInput
    B, hop, M, sr = 3, 500, 40, 16000
    gen = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, L, generator=gen).to(DEV)
    g = torch.randn(B, 1, M, L // hop + 1, generator=gen).to(DEV)
    layer = MelSpectrogramLayer(torch.tensor(lam0), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True, log=True).to(DEV)
    cell = torch.zeros(1, dtype=torch.int64, device=DEV)
    slot = SlotInput(cell, (B, L))
    for k in range(4):
        xk = _placed(x0, k)
        cell.fill_(xk.data_ptr())
        want, got = layer(xk), layer(slot)
        assert torch.isfinite(want).all() and torch.equal(got, want), k
        layer.lambd.grad = None
        want.backward(g)
        d0 = layer.lambd.grad.clone()
        layer.lambd.grad = None
        got.backward(g)
        assert torch.equal(layer.lambd.grad, d0)
        with torch.no_grad():
            assert torch.equal(layer(slot), layer(xk))
    assert layer.lambd_status()["error"] == 0


def test_a_captured_step_is_fed_batches_at_every_alignment():
    """One capture, batches handed over by address at k = 0, 1, 2, 3 in turn: after each replay the step equals the eager
    lambd_sync=True step on that view bit for bit -- the dispatch reads the address when the kernel RUNS, not when it was captured."""
    from dmel_amd import GraphedStep, MelSpectrogramLayer
    B, L, hop, M, sr, lam0 = 3, 4001, 128, 32, 8000, 40.0
    T = L // hop + 1
    gen = torch.Generator().manual_seed(31)
    n = 16
    data = [(_placed(torch.randn(B, L, generator=gen).to(DEV), i % 4), torch.randn(B, 1, M, T, generator=gen).to(DEV)) for i in range(n)]

    def make(sync):
        layer = MelSpectrogramLayer(torch.tensor(lam0), n_mels=M, n_points=L, sample_rate=sr, hop_length=hop, device=DEV, optimized=True,
                                    log=True, lambd_sync=sync).to(DEV)
        return layer, torch.optim.Adam([layer.lambd], lr=0.05, capturable=True)

    ref_layer, ref_opt = make(True)
    ref, ref_y = [], []
    for x, g in data:
        ref_opt.zero_grad(set_to_none=False)
        y = ref_layer(x)
        y.backward(g)
        ref_opt.step()
        ref.append(ref_layer.lambd.detach().clone())
        ref_y.append(y.detach().clone())
    torch.cuda.synchronize()

    layer, opt = make(False)
    y_out = torch.empty_like(ref_y[0])

    def step(x, g):
        opt.zero_grad(set_to_none=False)
        y = layer(x)
        y.backward(g)
        y_out.copy_(y.detach())
        opt.step()

    gs = GraphedStep(step, [layer], steps_per_replay=1, inputs=[data[0][0], data[0][1]], zero_copy=[True, False])
    for i, (x, g) in enumerate(data):
        assert x.data_ptr() % 16 == ((4 + i % 4) * 4) % 16
        assert gs.feed(x, g)
        torch.cuda.synchronize()
        assert torch.equal(layer.lambd.detach(), ref[i]), (i, layer.lambd.detach(), ref[i])
        assert torch.equal(y_out, ref_y[i]), i
    assert layer.lambd_status()["error"] == 0
    # ONE captured graph served every alignment class: some capture was followed by at least four replays in a row (k cycles 0 ... 3)
    marks = sorted(gs.capture_calls) + [gs.calls]
    print(f"captured step: {gs.captures} captures at calls {gs.capture_calls} of {gs.calls}")
    assert max(b - a for a, b in zip(marks, marks[1:])) >= 5, (gs.capture_calls, gs.calls)


# ---- the C ABI's output pointers (include/dmel.h, "Alignment") --------------------------------------------------------------------------
def _refused(fn, arg):
    from dmel_amd import capi
    with pytest.raises(capi.DmelError) as ei:
        fn()
    assert ei.value.status == capi.DMEL_ERR_INVALID_ARGUMENT, ei.value
    msg = str(ei.value)
    assert f": {arg} must be 16-byte aligned" in msg, msg
    return msg


def test_c_abi_refuses_misaligned_output_pointers_and_serves_the_next_call():
    """every entry point that stores through a pointer refuses a misaligned one on the host, naming the argument, before anything is
    launched; an aligned call right after a refused one on the same plan is correct"""
    from dmel_amd import capi
    case = C._case("capi_align", 2, 4001, 16000, 80.0, 128, 48, seed=210)
    B, L, hop, M, sr, lam = case["B"], case["L"], case["hop"], case["n_mels"], case["sr"], case["lambd"]
    T = L // hop + 1
    x_np = C.make_input(case).astype(np.float32)
    x = _placed(torch.from_numpy(x_np).to(DEV), 1)                       # (inputs need their element's alignment only)
    st = torch.cuda.current_stream().cuda_stream
    plan = capi.Plan(L, hop, M, sr)
    lam_d = torch.tensor(lam, device=DEV)
    lams, edges = [300.0, 80.0, 40.0], [0, 5, 30, 48]
    K = len(lams)
    lams_d = torch.tensor(lams, device=DEV)
    lengths = torch.tensor([L, 2000], dtype=torch.int32, device=DEV)
    nan = float("nan")
    out = torch.full((B * K * M * T + 8,), nan, device=DEV)
    tan = torch.full((B * K * M * T + 8,), nan, device=DEV)
    scr = torch.zeros((max(plan.scratch_bytes(B), plan.scratch_bytes_multi(B, K)) + 32,), dtype=torch.uint8, device=DEV)
    n = capi.n_fft(lam)
    spec = torch.full((B * (n // 2 + 1) * T + 8,), nan, device=DEV)
    o, t, s, sp = out.data_ptr(), tan.data_ptr(), scr.data_ptr(), spec.data_ptr()
    assert o % 16 == 0 and t % 16 == 0 and s % 16 == 0 and sp % 16 == 0
    for off in (4, 8, 12):
        m = _refused(lambda: plan.forward(x.data_ptr(), B, lam, o + off, t, True, 1e-10, st), "out")
        assert m.split(": ")[2] == "dmel_forward" and f"ends in {off} modulo 16" in m
        _refused(lambda: plan.forward(x.data_ptr(), B, lam, o, t + off, True, 1e-10, st), "tangent")
        _refused(lambda: plan.forward_dev(x.data_ptr(), B, lam_d.data_ptr(), o + off, t, True, 1e-10, st, s), "out")
        _refused(lambda: plan.forward_dev(x.data_ptr(), B, lam_d.data_ptr(), o, t + off, True, 1e-10, st, s), "tangent")
        _refused(lambda: plan.forward_dev(x.data_ptr(), B, lam_d.data_ptr(), o, t, True, 1e-10, st, s + off), "scratch")
        _refused(lambda: plan.forward_lengths(x.data_ptr(), lengths.data_ptr(), B, lam, o + off, t, True, 1e-10, st), "out")
        _refused(lambda: plan.forward_lengths(x.data_ptr(), lengths.data_ptr(), B, lam, o, t + off, True, 1e-10, st), "tangent")
        _refused(lambda: plan.forward_multi(x.data_ptr(), B, lams, o + off, t, True, 1e-10, st, s), "out")
        _refused(lambda: plan.forward_multi(x.data_ptr(), B, lams, o, t + off, True, 1e-10, st, s), "tangent")
        _refused(lambda: plan.forward_multi(x.data_ptr(), B, lams, o, t, True, 1e-10, st, s + off), "scratch")
        _refused(lambda: plan.forward_multi_dev(x.data_ptr(), B, lams_d.data_ptr(), K, o + off, t, True, 1e-10, st, s), "out")
        _refused(lambda: plan.forward_band(x.data_ptr(), B, lams, edges, o + off, t, True, 1e-10, st, s), "out")
        _refused(lambda: plan.forward_band(x.data_ptr(), B, lams, edges, o, t + off, True, 1e-10, st, s), "tangent")
        _refused(lambda: plan.forward_band_dev(x.data_ptr(), B, lams_d.data_ptr(), edges, o, t, True, 1e-10, st, s + off), "scratch")
        _refused(lambda: plan.spectrogram_ex(x.data_ptr(), B, lam, n, sp + off, None, st), "spec")
        _refused(lambda: plan.spectrogram_ex(x.data_ptr(), B, lam, n, sp, t + off, st), "tangent")
        _refused(lambda: plan.spectrogram(x.data_ptr(), B, lam, sp + off, st), "spec")
        _refused(lambda: plan.backward_x(x.data_ptr(), B, lam, t, None, o + off, False, st), "grad_x")
        _refused(lambda: plan.backward_fb(x.data_ptr(), B, lam, t, None, o + off, False, st), "grad_fb")
    bf = _refused(lambda: plan.forward(x.data_ptr(), B, lam, o + 2, t, True, 1e-10, st, extra_flags=capi.DMEL_FLAG_OUT_BF16), "out")
    assert "ends in 2 modulo 16" in bf
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(tan).all() and torch.isnan(spec).all() and not scr.any(), "a refused call wrote something"

    # the aligned call right after, on the same plan: correct (and equal to a plan that never refused anything)
    y_ref, t_ref = O.forward(x_np, lam, hop, M, sr, apply_log=True)
    plan.forward(x.data_ptr(), B, lam, o, t, True, 1e-10, st)
    fresh = capi.Plan(L, hop, M, sr)
    o2, t2 = torch.empty(B * M * T, device=DEV), torch.empty(B * M * T, device=DEV)
    fresh.forward(x.data_ptr(), B, lam, o2.data_ptr(), t2.data_ptr(), True, 1e-10, st)
    torch.cuda.synchronize()
    got = out[:B * M * T].view(B, 1, M, T)
    assert torch.equal(got.flatten(), o2) and torch.equal(tan[:B * M * T], t2)
    assert _log_err(got.cpu().numpy(), y_ref) <= TOL
    tscale = np.abs(t_ref).max() + 1e-30
    assert float(np.abs(tan[:B * M * T].view(B, 1, M, T).cpu().numpy() - t_ref).max()) / tscale <= TOL
    _refused(lambda: plan.forward_multi(x.data_ptr(), B, lams, o + 4, t, True, 1e-10, st, s), "out")
    plan.forward_multi(x.data_ptr(), B, lams, o, t, True, 1e-10, st, s)
    torch.cuda.synchronize()
    ym = out[:B * K * M * T].view(B, K, M, T).cpu().numpy()
    for c, lc in enumerate(lams):
        yc, _ = O.forward(x_np, lc, hop, M, sr, apply_log=True)
        assert _log_err(ym[:, c:c + 1], yc) <= TOL
    _refused(lambda: plan.spectrogram_ex(x.data_ptr(), B, lam, n, sp + 4, None, st), "spec")
    plan.spectrogram_ex(x.data_ptr(), B, lam, n, sp, None, st)
    torch.cuda.synchronize()
    ref = O.spectrogram(x_np, lam, hop, remove_dc=True)
    assert _rel_err(spec[:ref.size].view(ref.shape).cpu().numpy(), ref, floor=1e-5) <= TOL
    assert capi.load().dmel_abi_version() == 5
