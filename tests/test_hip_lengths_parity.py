"""MelSpectrogramLayer.forward(x, lengths) against independent references at partial lengths (frames t < Lc // hop + 1 of
clip b are what the reference layer returns for x[b, :Lc] alone).  Every reference fixture placed in wider zero-padded rows; a seeded sweep
clip by clip against the fp64 oracle (n_fft 32 ... 16384, lengths on the tile and hop edges); the tangent through the C ABI; bf16; samples
past a clip never read on any path; DC-dominated clips cut short; int64 lengths; device lambd at the edges of the lengths range.
Tolerances and metrics are those of tests/test_hip_parity.py."""
import numpy as np
import pytest
import torch

import cases as C
from dmel_amd import synth
from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from tangent_cases import assert_tangent
from test_hip_parity import TOL, _dlam_tol, _log_err, _rel_err, assert_parity, explain_by_clip_mean, parity_stats, record_parity
from test_hip_random_shapes import _assert_dlam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-10


def _mk(c, W, log=False, sync=False, bf16=False):
    """the layer of configuration `c` (a cases.py-style dict) on rows of W samples"""
    from dmel_amd import MelSpectrogramLayer
    return MelSpectrogramLayer(torch.tensor(float(c["lambd"]), dtype=torch.float32), n_mels=c["n_mels"], n_points=W, sample_rate=c["sr"],
                               f_min=c["f_min"], f_max=c["f_max"], hop_length=c["hop"], device=DEV, optimized=True,
                               normalize_window=c["normalize_window"], log=log, out_dtype=torch.bfloat16 if bf16 else torch.float32,
                               lambd_sync=sync).to(DEV)


def _run(lay, x, lengths, g=None):
    """(out, lambd.grad): a training forward + backward to lambd with upstream gradient g, or (g is None) an inference forward"""
    lay.lambd.grad = None
    if g is None:
        with torch.no_grad():
            return lay(x, lengths), None
    y = lay(x, lengths)
    (y.float() * g).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), float(lay.lambd.grad)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.element_size() == 4 else torch.int64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows(x_np, W, fill):
    """the clips of x_np (B, L) at the start of rows of W samples, the rest of each row `fill`"""
    B, L = x_np.shape
    out = np.full((B, W), fill, dtype=x_np.dtype)
    out[:, :L] = x_np
    return out


def _silent(lay, train):
    """None for a linear layer; for a log layer the one value every element of its output takes for an all-zero clip, in the same mode
    (training or inference)"""
    if not lay.log:
        return None
    W = lay.n_points
    z = torch.zeros(1, W, device=DEV)
    y, _ = _run(lay, z, torch.full((1,), W, dtype=torch.int32, device=DEV), torch.ones(1, 1, lay.n_mels, W // lay.hop_length + 1, device=DEV) if train else None)
    v = float(y.reshape(-1)[0])
    assert torch.equal(y, torch.full_like(y, v))
    return v


def _check_pad(y, tc, silent):
    """frames t >= tc[b] of clip b: exactly +0.0 (linear output: silent is None) or exactly the silent clip's log value"""
    for b, t in enumerate(tc):
        p = y[b, :, :, t:]
        if silent is None:
            assert torch.equal(_bits(p), torch.zeros_like(_bits(p))), (b, t)
        else:
            assert torch.equal(p, torch.full_like(p, silent)), (b, t)


# ---- 1. every reference fixture in a zero-padded batch -------------------------------------------------------------------------------------
FIXTURES = [c for c in C.CASES + C.DC_CASES if c["optimized"] and O.n_fft(c["lambd"]) <= 16384]


def _widths(L):
    """row widths around a clip of L samples: one that stays <= 32768 (the fused kernel sums the clip itself), one past it (dmel_prep_kernel's
    partial sums); both odd, so that rows after the first do not start 16-byte aligned"""
    ws = [min(L + 1001 + (L % 2), 32767)] if L + 2 <= 32767 else []
    return ws + [max(L + 2049 + (L % 2), 32769 + 2 * (L % 2 == 0))]


def _fixture_criteria(case, gold, got, log, xin, mean_ref, mean_cr, tag):
    """the criteria of test_matches_reference_golden / test_matches_reference_dc_dominated on the frames :T of a padded output `got`
    (B, 1, M, Tw); returns the means the kernel used (for d lambd)"""
    T = case["L"] // case["hop"] + 1
    y = got[:, :, :, :T].astype(np.float64)
    idx = C.sample_index(case)
    e = EPS if log else 0.0
    lin = np.exp(y) if log else y
    if case["kind"] == "dc":
        exp = gold["mel"].astype(np.float64)
        if case["dtype"] == "float64":
            rel = float((np.abs(lin - (exp + e)) / np.abs(exp + e)).max())
            record_parity(tag, {"n": int(exp.size), "plain_max_rel_vs_fixture": rel})
            assert rel <= TOL, (tag, rel)
            return mean_ref
        _, mean_used, rel_fix = explain_by_clip_mean(case, gold, lin, e, xin, mean_ref, mean_cr)
        record_parity(tag, {"n": int(exp.size), "plain_max_rel_vs_fixture": float(rel_fix.max())})
        return mean_used
    flat = y.reshape(-1) if idx is None else y[np.unravel_index(idx, C.out_shape(case))]
    exp = gold["mel"].reshape(-1) if idx is None else gold["mel_sampled"]
    if log:
        expy = np.log(exp.astype(np.float32) + np.float32(EPS))
        assert _log_err(flat, expy) <= TOL, tag
        got_c, exp_c = np.exp(flat), np.exp(expy.astype(np.float64))
    else:
        assert _rel_err(flat, exp) <= TOL, tag
        got_c, exp_c = flat, exp
    # g6_tone_dc (bins 120 dB down between the tones): where the plain bar fails, the last ulp of the clip mean must explain it, against the
    # oracle at the correctly rounded mean in the fixture's place.  (In a wider row the kernel's sum of the clip may land an ulp away from the
    # default path's: measured, clip 0 is then 1.23e-4 off the fixture while within 1e-4 of the oracle at the reference's mean.)
    if "mean_ref" in gold and idx is None and parity_stats(got_c, exp_c)["plain_max_rel"] > TOL:
        ref_cr = O.forward(xin, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"],
                           mean=mean_cr)[0]
        _, mean_used, _ = explain_by_clip_mean(case, {"mel": ref_cr}, lin, e, xin, mean_cr, mean_cr)
        return mean_used
    assert_parity(tag, got_c, exp_c, allow_floor=False)
    return mean_ref


@pytest.mark.parametrize("case", FIXTURES, ids=[c["name"] for c in FIXTURES])
def test_reference_fixture_in_a_zero_padded_batch(case):
    from test_oracle_golden import dc_reference_input
    gold = C.load(case)
    B, L, hop, M = case["B"], case["L"], case["hop"], case["n_mels"]
    T = L // hop + 1
    x_np = C.make_input(case)
    g_fix = C.make_cotangent(case)
    if case["kind"] == "dc":
        xin, mean_ref = dc_reference_input(case, gold)
        mean_cr = mean_ref.copy() if case["dtype"] == "float64" else np.float32(x_np.astype(np.float64).mean(1))
    elif "mean_ref" in gold:
        xin, mean_ref = x_np.astype(np.float32), gold["mean_ref"].astype(np.float32)
        mean_cr = np.float32(x_np.astype(np.float64).mean(1))
    else:
        xin, mean_ref, mean_cr = x_np.astype(np.float32), None, None
    t_refs = {}
    lengths = torch.full((B,), L, dtype=torch.int32, device=DEV)
    for W in _widths(L):
        Tw = W // hop + 1
        x = torch.from_numpy(_rows(x_np, W, np.nan)).to(DEV)
        g_np = np.random.default_rng(W).standard_normal((B, 1, M, Tw)).astype(np.float32)      # random on the pad frames ...
        g_np[:, :, :, :T] = g_fix                                                                # ... the fixture's cotangent on the clip
        g = torch.from_numpy(g_np).to(DEV)
        for log in (False, True):
            for mode in ("train", "infer", "sync"):
                lay = _mk(case, W, log=log, sync=mode == "sync")
                y, d = _run(lay, x, lengths, None if mode == "infer" else g)
                assert y.shape == (B, 1, M, Tw) and lay.n_fft() == int(gold["n_fft"])
                _check_pad(y, [T] * B, _silent(lay, mode != "infer"))
                tag = f"lengths/{case['name']}/W{W}/{mode}/" + ("exp_logmel" if log else "mel")
                mean_used = _fixture_criteria(case, gold, y.cpu().numpy(), log, xin, mean_ref, mean_cr, tag)
                if d is None:
                    continue
                if case["kind"] == "zero":
                    assert d == 0.0, d
                    continue
                same_mean = mean_ref is None or bool((mean_used == mean_ref).all())
                key = (log, None if same_mean else tuple(mean_used.tolist()))
                if key not in t_refs:
                    t_refs[key] = O.forward(xin, case["lambd"], hop, M, case["sr"], case["f_min"], case["f_max"], case["normalize_window"],
                                            apply_log=log, mean=None if mean_ref is None else mean_used)[1]
                t_ref = t_refs[key]
                exp_d = float(gold["dlam_log" if log else "dlam_lin"]) if same_mean else O.backward(g_fix, t_ref)
                if case["kind"] == "dc":
                    assert abs(d - exp_d) <= _dlam_tol(exp_d, g_fix, t_ref), (case["name"], W, mode, log, d, exp_d)
                else:
                    _assert_dlam(d, exp_d, g_fix, t_ref, f"{case['name']}/W{W}/{mode}/log{int(log)}")


# ---- 2. a seeded sweep, clip by clip against the oracle --------------------------------------------------------------------------------------
NFFTS = [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]


def _sweep_cases(n, seed):
    """_random_cases (tests/test_hip_random_shapes.py) for zero-padded rows: every n_fft 32 ... 16384 at least three times, rows up to
    ~60000 samples (some past 32768, some with W % 4 != 0), hop < N/2, N/2 < hop <= N and hop > N, B 1 ... 6"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        nft = NFFTS[i % len(NFFTS)] if i < 3 * len(NFFTS) else int(rng.choice(NFFTS))
        lam = float(rng.uniform(0.55, 0.99) * nft / 6.0) * (1.0 if rng.random() < 0.8 else -1.0)
        nf = O.n_fft(lam)
        kind = i % 3
        hop = (int(rng.integers(max(1, nf // 16), max(2, nf // 2))) if kind == 0 else
               int(rng.integers(nf // 2 + 1, nf + 1)) if kind == 1 else int(rng.integers(nf + 1, 2 * nf + 2)))
        lo = max(16, nf // 4, 2 * hop)
        W = int(rng.integers(max(lo, 32769), 60000)) if rng.random() < 0.35 and lo < 59000 else int(rng.integers(lo, max(lo + 64, min(6 * nf, 30000))))
        if rng.random() < 0.5:
            W += (4 - W % 4) % 4 + int(rng.integers(1, 4))                       # W % 4 != 0: rows after the first not 16-byte aligned
        T = W // hop + 1
        if T > 400:
            hop = max(hop, W // 300)
            T = W // hop + 1
        sr = int(rng.choice([8000, 16000, 22050, 44100]))
        n_mels = int(rng.choice([1, 7, 16, 40, 64, 80, 128, 130]))
        f_min = float(rng.choice([0.0, 0.0, 50.0, 300.0]))
        f_max = None if rng.random() < 0.6 else float(rng.uniform(0.3, 0.5) * sr)
        if f_max is not None and f_max <= f_min + 100.0:
            f_max = None
        B = int(rng.integers(1, 7))
        if B * T * nf > 6_000_000:                                            # keep the oracle in seconds
            continue
        out.append(dict(C.BY_NAME["g1_c1"], name=f"l{i}_n{nf}_W{W}_h{hop}_m{n_mels}_B{B}", B=B, L=W, lambd=lam, hop=hop, n_mels=n_mels, sr=sr,
                        f_min=f_min, f_max=f_max, normalize_window=bool(rng.random() < 0.4), seed=5000 + i))
    return out


SWEEP = _sweep_cases(40, seed=20261016) + [
    # kTrainW (the wave-local contraction) at n_fft 1024 and 2048, with the HTK bank of BASELINE's configs
    dict(C.BY_NAME["g1_c1"], name="w1024_W16003_h256_m128", B=4, L=16003, lambd=128.0, hop=256, n_mels=128, seed=5100),
    dict(C.BY_NAME["g1_c1"], name="w2048_W40001_h512_m128", B=3, L=40001, lambd=256.0, hop=512, n_mels=128, seed=5101),
]


def _edge_lengths(c, fpts, rng):
    """B lengths, alternately from the sample edges (1, 2, hop-1, hop, hop+1, N/2-1, N/2+1, W-1, W) and from the tile edges: lengths whose Tc
    is k FPT - 1, k FPT or k FPT + 1 for the frames per tile of each mode (the tile skip)"""
    W, hop, N = c["L"], c["hop"], O.n_fft(c["lambd"])
    T = W // hop + 1
    edges = sorted(v for v in {1, 2, hop - 1, hop, hop + 1, N // 2 - 1, N // 2 + 1, W - 1, W} if 1 <= v <= W)
    tiles = set()
    for fpt in fpts:
        for k in range(1, T // fpt + 2):
            for tc in (k * fpt - 1, k * fpt, k * fpt + 1):
                if 1 <= tc <= T:
                    tiles.add(min(W, (tc - 1) * hop + int(rng.integers(0, hop))))
    tiles = sorted(tiles)
    return [int(rng.choice(edges if b % 2 == 0 or not tiles else tiles)) for b in range(c["B"])]


def _reference_fp32_dlam(c, x, g, log):
    """d lambd of the reference's own fp32 arithmetic (oracle/torch_restatement.py: torch.stft + autograd on the CPU) for one clip"""
    from oracle import torch_restatement as R
    lam = torch.tensor(float(c["lambd"]), requires_grad=True)
    out = R.forward(torch.from_numpy(np.ascontiguousarray(x)), lam, c["hop"], c["n_mels"], c["sr"], c["f_min"], c["f_max"], c["normalize_window"],
                    log=log)
    (dl,) = torch.autograd.grad((out * torch.from_numpy(np.ascontiguousarray(g))).sum(), lam)
    return float(dl)


@pytest.mark.parametrize("c", SWEEP, ids=[c["name"] for c in SWEEP])
def test_sweep_clip_by_clip_against_the_oracle(c):
    B, W, hop, M = c["B"], c["L"], c["hop"], c["n_mels"]
    T = W // hop + 1
    x_np = C.make_input(c).astype(np.float32)
    g_np = C.make_cotangent(c)
    x, g = torch.from_numpy(x_np).to(DEV), torch.from_numpy(g_np).to(DEV)
    fpts = []
    for train in (True, False):
        lay = _mk(c, W)
        _run(lay, x, torch.full((B,), W, dtype=torch.int32, device=DEV), g if train else None)
        fpts.append(lay.plan_info()["frames_per_tile"])
    lens = _edge_lengths(c, fpts, np.random.default_rng(c["seed"]))
    tc = [lb // hop + 1 for lb in lens]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for log in (False, True):
        refs = [O.forward(x_np[b:b + 1, :lens[b]], c["lambd"], hop, M, c["sr"], c["f_min"], c["f_max"], c["normalize_window"], apply_log=log)
                for b in range(B)]
        g_real = np.concatenate([g_np[b, :, :, :tc[b]].reshape(-1) for b in range(B)])
        t_real = np.concatenate([refs[b][1].reshape(-1) for b in range(B)])
        exp_d = sum(O.backward(g_np[b:b + 1, :, :, :tc[b]], refs[b][1]) for b in range(B))
        d32 = sum(_reference_fp32_dlam(c, x_np[b:b + 1, :lens[b]], g_np[b:b + 1, :, :, :tc[b]], log) for b in range(B))
        # d lambd: _assert_dlam (the plain 1e-4 wherever the sum does not cancel) on the linear output; out of reach of fp32 arithmetic is the
        # log output's, where t / (mel + eps) amplifies the rounding of small bands: the reference's own fp32 result misses that bar
        # (measured: l2, lengths 184 / 182 / 516, 1.3e-4 off the oracle, by an amount that varies with the CPU that runs it) -- there the bar
        # of _dlam_tol, widened by twice the reference's own distance from the oracle
        strict = not log
        for train in (True, False):
            lay = _mk(c, W, log=log)
            y, d = _run(lay, x, lengths, g if train else None)
            assert y.shape == (B, 1, M, T)
            _check_pad(y, tc, _silent(lay, train))
            y = y.cpu().numpy()
            for b in range(B):
                got, exp = y[b:b + 1, :, :, :tc[b]], refs[b][0]
                tag = f"lengths_sweep/{c['name']}/b{b}_L{lens[b]}/{'train' if train else 'infer'}/" + ("exp_logmel" if log else "mel")
                if log:
                    assert_parity(tag, np.exp(got.astype(np.float64)), np.exp(exp.astype(np.float64)), allow_floor=False)
                else:
                    assert_parity(tag, got, exp, allow_floor=False)
            if train:
                if strict:
                    _assert_dlam(d, exp_d, g_real, t_real, f"{c['name']}/log{int(log)} lengths={lens}")
                else:
                    # the bar of _dlam_tol, widened by twice the fp32 reference's own distance from the oracle
                    tol = _dlam_tol(exp_d, g_real, t_real) + 2.0 * abs(d32 - exp_d)
                    assert abs(d - exp_d) <= tol, (c["name"], log, lens, d, exp_d, d32)


# ---- 3. the tangent through the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,lens", [("g1_c1", 16003, [16000, 1, 4097, 255, 9999]), ("g6_n32", 2001, [2000, 17, 16, 1500]),
                                         ("g5_n4096", 40003, [40000, 3000, 12345, 40003]), ("g6_normwin", 16001, [8000, 257, 16000])])
def test_c_abi_tangent_at_partial_lengths(name, W, lens):
    from dmel_amd import capi
    c = C.BY_NAME[name]
    B, hop, M = len(lens), c["hop"], c["n_mels"]
    T = W // hop + 1
    x_np = synth.waveforms(B, W, seed=c["seed"] + 50)
    x = torch.from_numpy(x_np).to(DEV)
    plan = capi.Plan(W, hop, M, c["sr"], c["f_min"], float(c["f_max"] or c["sr"] // 2), c["normalize_window"])
    lib, s = capi.load(), torch.cuda.current_stream().cuda_stream
    lam_dev = torch.tensor([c["lambd"]], dtype=torch.float32, device=DEV)
    tc = [lb // hop + 1 for lb in lens]

    def both(lengths, log):
        res = []
        for dev in (False, True):
            out, tan = torch.full((B, 1, M, T), 7.0, device=DEV), torch.full((B, 1, M, T), 7.0, device=DEV)
            flags = capi.DMEL_FLAG_LOG if log else 0
            if dev:
                rc = lib.dmel_forward_dev_lengths(plan.handle, x.data_ptr(), lengths.data_ptr(), B, lam_dev.data_ptr(), flags, EPS,
                                                  out.data_ptr(), tan.data_ptr(), None, s)
            else:
                rc = lib.dmel_forward_lengths(plan.handle, x.data_ptr(), lengths.data_ptr(), B, capi.C.c_float(c["lambd"]), flags, EPS,
                                              out.data_ptr(), tan.data_ptr(), None, s)
            capi._check(rc)
            torch.cuda.synchronize()
            res.append((out, tan))
        assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])
        return res[0]

    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for log in (False, True):
        out, tan = both(lengths, log)
        lay = _mk(dict(c, L=W), W, log=log)
        assert _same(_run(lay, x, lengths, torch.ones(B, 1, M, T, device=DEV))[0], out)
        o, t = out.cpu().numpy(), tan.cpu().numpy()
        for b, lb in enumerate(lens):
            o_ref, t_ref = O.forward(x_np[b:b + 1, :lb], c["lambd"], hop, M, c["sr"], c["f_min"], c["f_max"], c["normalize_window"], apply_log=log)
            if log:
                assert _log_err(o[b:b + 1, :, :, :tc[b]], o_ref) <= TOL, (name, b)
            else:
                assert_parity(f"lengths_capi/{name}/b{b}/mel", o[b:b + 1, :, :, :tc[b]], o_ref, allow_floor=False)
            tscale = np.abs(t_ref).max() + 1e-30
            assert float(np.abs(t[b:b + 1, :, :, :tc[b]] - t_ref).max()) / tscale <= TOL, (name, b, log)
            # ... and every element against its own cancellation-free magnitude (tests/tangent_cases.py)
            _, _, sc = R.tangent_fp64(x_np[b:b + 1, :lb], c["lambd"], hop, M, c["sr"], c["f_min"], c["f_max"], c["normalize_window"], log=log)
            assert_tangent(f"tangent/lengths_capi/{name}/b{b}_L{lb}/{'log' if log else 'lin'}", t[b:b + 1, :, :, :tc[b]], t_ref, sc, shape=t_ref.shape)
            assert (t[b, :, :, tc[b]:] == 0.0).all(), (name, b, log)
        # an invalid length: its own clip's output and tangent are NaN, the other clips keep their bits
        bad = lengths.clone()
        bad[1] = W + 1
        out_b, tan_b = both(bad, log)
        assert torch.isnan(out_b[1]).all() and torch.isnan(tan_b[1]).all()
        keep = [b for b in range(B) if b != 1]
        assert _same(out_b[keep], out[keep]) and _same(tan_b[keep], tan[keep])


# ---- 4. bf16 at partial lengths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,W,hop,lens", [(128.0, 16001, 256, [16001, 3000, 1, 8192]), (5.0, 2003, 16, [700, 2003, 31]),
                                            (1300.0, 40001, 1000, [40001, 999, 33000])])
def test_bf16_is_the_rounded_fp32_lengths_output(lam, W, hop, lens):
    c = dict(C.BY_NAME["g1_c1"], lambd=lam, hop=hop, L=W)
    B, M = len(lens), c["n_mels"]
    x = torch.from_numpy(synth.waveforms(B, W, seed=61)).to(DEV)
    g32 = torch.from_numpy(synth.cotangent((B, 1, M, W // hop + 1), seed=62)).to(DEV)
    g16 = g32.to(torch.bfloat16)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for log in (False, True):
        for train in (True, False):
            y32, d32 = _run(_mk(c, W, log=log), x, lengths, g16.float() if train else None)
            y16, d16 = _run(_mk(c, W, log=log, bf16=True), x, lengths, g16 if train else None)
            assert y16.dtype == torch.bfloat16 and _same(y16, y32.to(torch.bfloat16)), (log, train)
            assert d16 == d32, (log, train, d16, d32)


# ---- 5. samples past a clip are never read -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,W,hop", [(5.0, 4001, 40), (20.0, 6003, 64), (300.0, 20001, 256), (600.0, 33001, 500), (1200.0, 40003, 1000),
                                       (2500.0, 50001, 2000)], ids=["nfft32", "nfft128", "nfft2048", "nfft4096", "nfft8192", "nfft16384"])
def test_tails_are_never_read(lam, W, hop):
    c = dict(C.BY_NAME["g1_c1"], lambd=lam, hop=hop, L=W)
    B, M = 4, c["n_mels"]
    x = torch.from_numpy(synth.waveforms(B, W, seed=71)).to(DEV)
    lens = [W - 1, 1, W // 3, 2 * hop + 1]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = torch.randn(B, 1, M, W // hop + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(72))
    tail = torch.arange(W, device=DEV)[None, :] >= lengths[:, None]
    for train in (True, False):
        lay = _mk(c, W, log=True)
        ref = _run(lay, x.masked_fill(tail, 0.0), lengths, g if train else None)
        assert torch.isfinite(ref[0]).all()
        for fill in (float("nan"), 1e30):
            got = _run(lay, x.masked_fill(tail, fill), lengths, g if train else None)
            assert _same(ref[0], got[0]) and ref[1] == got[1], (train, fill)


def test_batch_by_address_past_32768_samples():
    """dmel_prep_kernel reads the batch through the pointer cell: bit-equal to the direct call"""
    from dmel_amd import SlotInput
    c = dict(C.BY_NAME["g1_c1"], lambd=1200.0, hop=1000, L=40001)
    B, W, M, hop = 3, 40001, c["n_mels"], c["hop"]
    x = torch.from_numpy(synth.waveforms(B, W, seed=73)).to(DEV)
    lengths = torch.tensor([40001, 20000, 33333], dtype=torch.int32, device=DEV)
    x = x.masked_fill(torch.arange(W, device=DEV)[None, :] >= lengths[:, None], float("nan"))
    g = torch.randn(B, 1, M, W // hop + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(74))
    cell = torch.tensor([x.data_ptr()], dtype=torch.int64, device=DEV)
    for train in (True, False):
        lay = _mk(c, W, log=True)
        a = _run(lay, x, lengths, g if train else None)
        b = _run(lay, SlotInput(cell, x.shape), lengths, g if train else None)
        assert torch.isfinite(a[0]).all() and _same(a[0], b[0]) and a[1] == b[1], train


# ---- 6. DC-dominated clips cut short ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.DC_CASES, ids=[c["name"] for c in C.DC_CASES])
def test_dc_dominated_clips_at_partial_lengths(case):
    """fp32: the kernel is the oracle at a mean within 2 ulp of the correctly rounded mean of x[b, :Lc] (explain_by_clip_mean's logic, with
    the oracle at that mean in the fixture's place); fp64: plain 1e-4 against the oracle on the clip centred in fp64"""
    B, L, hop = case["B"], case["L"], case["hop"]
    x_np = C.make_input(case)
    lens = [L - 1 - 997 * b for b in range(B)]
    lens[-1] = L // 3 + 1
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    x = torch.from_numpy(_rows(x_np, L, np.nan)).to(DEV)
    x = torch.where(torch.arange(L, device=DEV)[None, :] < lengths[:, None], x, torch.full_like(x, float("nan")))
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to(DEV)
    f64 = case["dtype"] == "float64"
    for log in (False, True):
        e = EPS if log else 0.0
        y, d = _run(_mk(case, L, log=log), x, lengths, g)
        y = y.cpu().numpy().astype(np.float64)
        lin = np.exp(y) if log else y
        exp_d, gs, ts = 0.0, [], []
        for b, lb in enumerate(lens):
            tcb = lb // hop + 1
            clip = x_np[b:b + 1, :lb]
            cb = dict(case, B=1, L=lb)
            if f64:
                xin, mean = (clip - clip.mean(1, keepdims=True)).astype(np.float32), None
            else:
                xin, mean_cr = clip, np.float32(clip.astype(np.float64).mean(1))
                ref_cr = O.forward(xin, case["lambd"], hop, case["n_mels"], case["sr"], apply_log=False, mean=mean_cr)[0]
                _, mean, _ = explain_by_clip_mean(cb, {"mel": ref_cr}, lin[b:b + 1, :, :, :tcb], e, xin, mean_cr, mean_cr)
            o_ref, t_ref = O.forward(xin, case["lambd"], hop, case["n_mels"], case["sr"], apply_log=log, mean=mean)
            if f64:
                lo = np.exp(o_ref.astype(np.float64)) if log else o_ref.astype(np.float64)
                rel = float((np.abs(lin[b:b + 1, :, :, :tcb] - lo) / np.abs(lo)).max())
                assert rel <= TOL, (case["name"], b, lb, log, rel)
            exp_d += O.backward(g_np[b:b + 1, :, :, :tcb], t_ref)
            gs.append(g_np[b, :, :, :tcb].reshape(-1))
            ts.append(t_ref.reshape(-1))
        g_real, t_real = np.concatenate(gs), np.concatenate(ts)
        assert abs(d - exp_d) <= _dlam_tol(exp_d, g_real, t_real), (case["name"], log, d, exp_d)


# ---- 7. int64 lengths --------------------------------------------------------------------------------------------------------------------------------
def test_int64_lengths_out_of_range_poison_their_clip():
    c = dict(C.BY_NAME["g1_c1"], L=16000)
    B, W, M, hop = 6, 16000, c["n_mels"], c["hop"]
    x = torch.from_numpy(synth.waveforms(B, W, seed=81)).to(DEV)
    g = torch.randn(B, 1, M, W // hop + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(82))
    l64 = torch.tensor([2 ** 32 + 4000, 8000, -2 ** 32 + 16000, 12000, 2 ** 31, 16000], dtype=torch.int64, device=DEV)
    l32 = torch.tensor([4000, 8000, 16000, 12000, 3000, 16000], dtype=torch.int32, device=DEV)
    bad, good = [0, 2, 4], [1, 3, 5]
    for train in (True, False):
        lay = _mk(c, W, log=True)
        a, _ = _run(lay, x, l32, g if train else None)
        b, _ = _run(lay, x, l64, g if train else None)
        b_cpu, _ = _run(lay, x, l64.cpu(), g if train else None)
        assert _same(b, b_cpu)
        for k in bad:
            assert torch.isnan(b[k]).all(), (train, k)
        assert _same(a[good], b[good]), train


# ---- 8. device lambd at the edges of the lengths range -------------------------------------------------------------------------------------------
def test_sync_free_steps_across_4096_8192_with_lengths():
    """eager steps whose lambd crosses 6 lambd = 4096 up and back down on a batch past 32768 samples (guard launches sharing the prep kernel's
    sums): every step bit-equal to lambd_sync=True"""
    c = dict(C.BY_NAME["g1_c1"], lambd=681.0, hop=500, L=40000, n_mels=64)
    B, W, M = 3, 40000, 64
    x = torch.from_numpy(synth.waveforms(B, W, seed=91)).to(DEV)
    lengths = torch.tensor([40000, 17001, 33000], dtype=torch.int32, device=DEV)
    g = torch.randn(B, 1, M, W // c["hop"] + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(92))
    free, sync = _mk(c, W, log=True), _mk(c, W, log=True, sync=True)
    seen = set()
    for delta in (0.7, 0.7, 0.7, 0.7, -0.7, -0.7, -0.7, -0.7, 0.7):
        a, b = _run(free, x, lengths, g), _run(sync, x, lengths, g)
        seen.add(sync.n_fft())
        assert _same(a[0], b[0]) and a[1] == b[1], (float(sync.lambd), a[1], b[1])
        with torch.no_grad():
            free.lambd.add_(delta)
            sync.lambd.add_(delta)
    torch.cuda.synchronize()
    assert seen == {4096, 8192} and free.lambd_status()["error"] == 0


@pytest.mark.parametrize("lam,jump,valid", [(2700.0, 40.0, 2000.0), (5.0, -3.0, 4.0)], ids=["16384_to_32768", "32_to_16"])
def test_device_lambd_leaving_the_lengths_range_fails_loudly_then_recovers(lam, jump, valid):
    c = dict(C.BY_NAME["g1_c1"], lambd=lam, hop=256, L=20000)
    B, W = 2, 20000
    x = torch.from_numpy(synth.waveforms(B, W, seed=93)).to(DEV)
    lengths = torch.tensor([20000, 7000], dtype=torch.int32, device=DEV)
    lay = _mk(c, W, log=True)
    y0, _ = _run(lay, x, lengths)
    assert torch.isfinite(y0).all()
    with torch.no_grad():
        lay.lambd.add_(jump)                                  # out of 32 ... 16384 on the device: no launch of the lengths path covers it
    y1, _ = _run(lay, x, lengths)
    torch.cuda.synchronize()
    assert torch.isnan(y1).all() and lay.lambd_status()["error"] != 0
    with pytest.raises(RuntimeError):
        _run(lay, x, lengths)
    with torch.no_grad():
        lay.lambd.fill_(valid)
    lay.resync()
    y2, _ = _run(lay, x, lengths)
    assert _same(y2, _run(_mk(dict(c, lambd=valid), W, log=True, sync=True), x, lengths)[0])
