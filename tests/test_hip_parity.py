"""GPU parity tests: the HIP path (through the C ABI / nn.Module) against
  (1) the golden vectors captured from the reference (tests/golden/*.npz), and
  (2) the CPU oracle on the same seeded inputs.
Tolerances (BASELINE.json north_star): rel <= 1e-4 on mel, abs <= 1e-4 on log-mel,
rel <= 1e-4 on d lambd.
"""
import numpy as np
import pytest
import torch

import cases as C
from oracle import dmel_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _layer(case, log=False, trainable=True):
    from dmel_amd import MelSpectrogramLayer
    layer = MelSpectrogramLayer(torch.tensor(float(case["lambd"]), dtype=torch.float32), n_mels=case["n_mels"],
                                n_points=case["L"], sample_rate=case["sr"], f_min=case["f_min"], f_max=case["f_max"],
                                hop_length=case["hop"], device="cuda:0", optimized=case.get("optimized", True),
                                normalize_window=case["normalize_window"], log=log).to("cuda:0")
    layer.requires_grad_(trainable)
    return layer


FLOOR = 1e-6        # of the loudest value: 120 dB


def parity_stats(got, exp, floor=FLOOR):
    """What the comparison of `got` with the reference `exp` (mel power) looks like, with nothing hidden:
      plain_max_rel          max |got - exp| / |exp| over EVERY element with exp != 0 (north_star's bar read literally)
      frac_below_floor       share of elements more than 120 dB below the loudest one (|exp| < floor max|exp|)
      max_rel_above_floor    plain relative error of everything at or above that floor
      floored_max_rel        the metric asserted since round 1: |got - exp| / max(|exp|, floor max|exp|)
    Elements 120 dB down are fp32 noise in the reference itself (its own fp32 STFT sits 1e-5 relative to the LOUDEST bin off an
    fp64 evaluation), so a plain relative error there compares two roundings."""
    g, e = got.astype(np.float64).reshape(-1), exp.astype(np.float64).reshape(-1)
    ae = np.abs(e)
    top = float(ae.max()) if ae.size else 0.0
    err = np.abs(g - e)
    nz = ae > 0
    above = ae >= floor * top
    return {"n": int(e.size), "plain_max_rel": float((err[nz] / ae[nz]).max()) if nz.any() else 0.0,
            "frac_below_floor": float(1.0 - above.mean()) if e.size else 0.0,
            "max_rel_above_floor": float((err[above & nz] / ae[above & nz]).max()) if (above & nz).any() else 0.0,
            "floored_max_rel": float((err / np.maximum(ae, floor * top + 1e-30)).max()) if e.size else 0.0,
            "max_abs_where_exp_is_zero": float(err[~nz].max()) if (~nz).any() else 0.0}


_REPORT = {}


def record_parity(name, st):
    """collected over the session and written to gpurun_out/r04_parity_report.json (tests/conftest.py) -- the numbers behind the
    asserts, for DESIGN.md section 6"""
    _REPORT[name] = {k: (round(v, 9) if isinstance(v, float) else v) for k, v in st.items()}


def assert_parity(name, got, exp, tol=None, max_frac_below=0.02, allow_floor=True):
    """rel <= 1e-4 as a PLAIN relative error on every element (north_star's bar read literally; with allow_floor=False that is
    all there is: measured in round 4, it holds on every element of all 27 reference fixtures and all 72 random configurations,
    lin and log, worst case 6.9e-5 -- profiles/r04_parity_report.json).  With allow_floor: otherwise plain on everything at or
    above the 120 dB floor, the floored metric below it, and a bound on how much of the tensor the floor covers (so that it cannot
    hide a broken band)"""
    tol = TOL if tol is None else tol
    st = parity_stats(got, exp)
    st["floor_needed"] = bool(st["plain_max_rel"] > tol)
    record_parity(name, st)
    assert st["max_abs_where_exp_is_zero"] <= 1e-30, (name, st)          # an exact zero of the reference is an exact zero here
    if not st["floor_needed"]:
        return st
    assert allow_floor, (name, "plain relative error above the bar", st)
    assert st["max_rel_above_floor"] <= tol, (name, st)
    assert st["floored_max_rel"] <= tol, (name, st)
    assert st["frac_below_floor"] <= max_frac_below, (name, st)
    return st


def _rel_err(got, exp, floor=FLOOR):
    # rel error on mel; bins more than 120 dB below the loudest one are fp32 noise in the reference
    # itself (its own floor), so they are measured against that floor
    scale = np.maximum(np.abs(exp), floor * np.abs(exp).max() + 1e-30)
    return float((np.abs(got.astype(np.float64) - exp.astype(np.float64)) / scale).max())


def _log_err(got_y, exp_y, eps=1e-10):
    """abs error on log-mel == rel error on (mel + eps), with the same 120 dB floor as _rel_err."""
    return _rel_err(np.exp(got_y.astype(np.float64)), np.exp(exp_y.astype(np.float64)))


def _dlam_tol(exp_d, g_np, t_ref):
    """rel 1e-4 on d lambd, plus the fp32 floor of the sum itself: d lambd = sum g*t cancels heavily
    (sum|g*t| / |d lambd| reaches 2.5e4 in the fixtures), and the reference's own fp32 autograd value
    carries ~1e-8 * sum|g*t| of rounding noise."""
    return TOL * abs(exp_d) + 2e-8 * float(np.abs(g_np.astype(np.float64) * t_ref.astype(np.float64)).sum()) + 1e-7


def explain_by_clip_mean(case, gold, lin, e, xin, mean_ref, mean_cr, max_ulps=2):
    """For fixtures that store the clip means the reference subtracted (``mean_ref``): per clip, the smallest |k| <= max_ulps such that
    the kernel's result `lin` (mel, or mel + eps for the log output: `e`) is -- on EVERY element, to a plain 1e-4 -- the reference's
    path evaluated at the mean `mean_cr + k ulp` (the oracle, pinned to these fixtures at the reference's own mean).  Where that mean is
    the reference's, the kernel must match the fixture itself.  Returns (k per clip, the means)."""
    exp = gold["mel"].astype(np.float64)
    rel_fix = np.abs(lin - (exp + e)) / np.abs(exp + e)
    used = np.zeros(case["B"], dtype=np.int64)
    mean_used = mean_cr.copy()
    for b in range(case["B"]):
        ulp = np.spacing(np.abs(mean_cr[b]))                       # (of THIS clip's mean: 0.49999... sits in the binade below 0.5)
        best = None
        for k in sorted(range(-max_ulps, max_ulps + 1), key=abs):
            cand = mean_cr[b:b + 1] + np.float32(k) * ulp
            o_k, _ = O.forward(xin[b:b + 1], case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                               case["normalize_window"], apply_log=False, mean=cand)
            r = float((np.abs(lin[b] - (o_k[0].astype(np.float64) + e)) / np.abs(o_k[0].astype(np.float64) + e)).max())
            if best is None or r < best[0]:
                best = (r, k, cand[0])
            if r <= TOL:
                break
        assert best[0] <= TOL, (case["name"], b, f"no mean within {max_ulps} ulp of the correctly rounded one explains this clip", best)
        used[b], mean_used[b] = best[1], best[2]
        if mean_used[b] == mean_ref[b]:
            assert rel_fix[b].max() <= TOL, (case["name"], b, "same mean as the reference, other output", float(rel_fix[b].max()))
    return used, mean_used, rel_fix


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_matches_reference_golden(case):
    gold = C.load(case)
    x = torch.from_numpy(C.make_input(case)).to("cuda:0")
    g = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")
    idx = C.sample_index(case)
    exp = gold["mel"].reshape(-1) if idx is None else gold["mel_sampled"]

    lin = _layer(case, log=False)
    assert lin.n_fft() == int(gold["n_fft"])
    mel = lin(x)
    assert mel.shape == C.out_shape(case) and mel.dtype == torch.float32
    (mel * g).sum().backward()
    mel_np = mel.detach().cpu().numpy()
    got = mel_np.reshape(-1) if idx is None else mel_np.reshape(-1)[idx]
    assert _rel_err(got, exp) <= TOL
    # a fixture that stores the means the reference subtracted (g6_tone_dc: tones + an offset, bins 120 dB down between the tones): where the
    # plain bar fails, the last ulp of the clip mean must explain it (see test_matches_reference_dc_dominated)
    by_mean = "mean_ref" in gold and idx is None and parity_stats(got, exp)["plain_max_rel"] > TOL
    if by_mean:
        x32m = C.make_input(case).astype(np.float32)
        mean_cr = np.float32(x32m.astype(np.float64).mean(1))
        k_lin, _, _ = explain_by_clip_mean(case, gold, mel_np.astype(np.float64), 0.0, x32m, gold["mean_ref"].astype(np.float32), mean_cr)
        record_parity("golden/" + case["name"] + "/mel", dict(parity_stats(got, exp), kernel_mean_ulps_from_correctly_rounded=[int(v) for v in k_lin]))
    else:
        assert_parity("golden/" + case["name"] + "/mel", got, exp, allow_floor=False)
    np.testing.assert_allclose(mel_np.astype(np.float64).reshape(case["B"], -1).sum(1), gold["mel_sum"], rtol=TOL, atol=1e-12)
    dl_lin = float(lin.lambd.grad)

    lg = _layer(case, log=True)
    y = lg(x)
    (y * g).sum().backward()
    y_np = y.detach().cpu().numpy()
    goty = y_np.reshape(-1) if idx is None else y_np.reshape(-1)[idx]
    expy = np.log(exp.astype(np.float32) + np.float32(1e-10))
    assert _log_err(goty, expy) <= TOL
    # (log domain: exp() of both sides, i.e. the relative error of mel + 1e-10 -- the abs error of the log output)
    if by_mean:
        explain_by_clip_mean(case, gold, np.exp(y_np.astype(np.float64)), 1e-10, x32m, gold["mean_ref"].astype(np.float32), mean_cr)
    else:
        assert_parity("golden/" + case["name"] + "/exp_logmel", np.exp(goty.astype(np.float64)), np.exp(expy.astype(np.float64)), allow_floor=False)
    dl_log = float(lg.lambd.grad)

    x32 = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    for got_d, exp_d, log in ((dl_lin, float(gold["dlam_lin"]), False), (dl_log, float(gold["dlam_log"]), True)):
        if case["kind"] == "zero":
            assert got_d == 0.0 and np.isfinite(got_d)
        else:
            _, t_ref = O.forward(x32, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                 case["normalize_window"], apply_log=log, optimized=case["optimized"])
            assert abs(got_d - exp_d) <= _dlam_tol(exp_d, g_np, t_ref), (got_d, exp_d)
            # north_star's bar is a plain relative 1e-4: wherever the sum is not dominated by cancellation (|d lambd| more than
            # 1e-3 of sum |g t|: every noise fixture) it is asserted as such, without the floor term of _dlam_tol
            cancel = float(np.abs(g_np.astype(np.float64) * t_ref.astype(np.float64)).sum())
            if abs(exp_d) > 1e-3 * cancel:
                assert abs(got_d - exp_d) <= TOL * abs(exp_d), (case["name"], got_d, exp_d, abs(got_d - exp_d) / abs(exp_d))


@pytest.mark.parametrize("case", C.DC_CASES, ids=[c["name"] for c in C.DC_CASES])
def test_matches_reference_dc_dominated(case):
    """G13 (tests/golden/cases.py: DC_CASES): clips whose offset is 10 ... 500 x their signal, outputs of the reference's own layer.
    One ulp of the fp32 clip mean (models.py:38) moves the lowest mel bands by up to 3e-2 there, and torch's own fp32 sum is one ulp
    off the correctly rounded mean in a third of these clips (tests/test_oracle_golden.py) -- bit parity with torch.mean is not a
    property of the algorithm; staying within an ulp or two of it is (csrc/dmel_kernels.h: "the clip mean": pairwise fp32 tree, the
    quotient by L rounded once).  Asserted, per clip, on EVERY element and to a plain 1e-4:
      * the kernel is the reference's path (the oracle, pinned to these very fixtures AT the reference's mean) evaluated at a mean
        no more than TWO ulp from the correctly rounded one -- which one (0 or +-1 expected) is recorded in the parity report;
      * wherever that mean IS the one the reference subtracted, the kernel matches the fixture itself.
    fp64 clips: the reference subtracts in fp64; so does the layer (before its cast to fp32): plain 1e-4 against the fixture."""
    from test_oracle_golden import dc_reference_input
    gold = C.load(case)
    x_np = C.make_input(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to("cuda:0")
    exp = gold["mel"].astype(np.float64)
    xin, mean_ref = dc_reference_input(case, gold)
    f64 = case["dtype"] == "float64"
    mean_cr = mean_ref.copy() if f64 else np.float32(x_np.astype(np.float64).mean(1))
    for log in (False, True):
        e = 1e-10 if log else 0.0
        layer = _layer(case, log=log)
        assert layer.n_fft() == int(gold["n_fft"])
        out = layer(x)
        (out * g).sum().backward()
        got = out.detach().cpu().numpy().astype(np.float64)
        got_d = float(layer.lambd.grad)
        lin = np.exp(got) if log else got                        # the log output is compared as mel + eps (abs error of the log)
        if f64:
            rel_fix = np.abs(lin - (exp + e)) / np.abs(exp + e)
            assert rel_fix.max() <= TOL, (case["name"], float(rel_fix.max()))
            used, mean_used = np.zeros(case["B"], dtype=np.int64), mean_cr.copy()
        else:
            used, mean_used, rel_fix = explain_by_clip_mean(case, gold, lin, e, xin, mean_ref, mean_cr)
        record_parity("golden/" + case["name"] + ("/exp_logmel" if log else "/mel"),
                      {"n": int(exp.size), "plain_max_rel_vs_fixture": float(rel_fix.max()),
                       "kernel_mean_ulps_from_correctly_rounded": [int(v) for v in used],
                       "reference_mean_ulps_from_correctly_rounded": [int(round(float((np.float64(mean_ref[b]) - np.float64(mean_cr[b])) / np.spacing(np.abs(mean_cr[b]))))) for b in range(case["B"])]})
        # d lambd against the oracle at the means the kernel used (= the fixture's value when they are the reference's)
        _, t_ref = O.forward(xin, case["lambd"], case["hop"], case["n_mels"], case["sr"], apply_log=log, mean=mean_used)
        same = bool((mean_used == mean_ref).all())
        exp_d = float(gold["dlam_log" if log else "dlam_lin"]) if same else O.backward(g_np, t_ref)
        assert abs(got_d - exp_d) <= _dlam_tol(exp_d, g_np, t_ref), (case["name"], log, got_d, exp_d)


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g5_n128", "g5_n4096", "g6_n256_ragged", "g6_n64", "g6_n32",
                                  "g6_n2048_short", "g6_normwin", "g6_tone_dc"])
def test_matches_oracle_elementwise(name):
    """Every element (not just the stored sample) against the fp64-accumulating oracle, and the
    tangent d out / d lambd itself, which the golden fixtures only pin through its dot product."""
    case = C.BY_NAME[name]
    x_np = C.make_input(case).astype(np.float32)
    x = torch.from_numpy(x_np).to("cuda:0")
    from dmel_amd import capi
    plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
    for log in (False, True):
        out = torch.empty(C.out_shape(case), dtype=torch.float32, device="cuda:0")
        tan = torch.empty_like(out)
        plan.forward(x.data_ptr(), case["B"], case["lambd"], out.data_ptr(), tan.data_ptr(), log, 1e-10,
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                 case["normalize_window"], apply_log=log)
        o, t = out.cpu().numpy(), tan.cpu().numpy()
        if log:
            assert _log_err(o, o_ref) <= TOL
        else:
            assert _rel_err(o, o_ref) <= TOL
        # tangent: signed sums cancel, so measure against the frame's own scale
        tscale = np.abs(t_ref).max() + 1e-30
        assert float(np.abs(t - t_ref).max()) / tscale <= TOL
        # ... and every element against its own cancellation-free magnitude (tests/tangent_cases.py): the measure above accepts anything
        # for the elements below 1e-4 of the largest.  Not g6_tone_dc (tones and an offset, bins 120 dB down between the tones): there the
        # references themselves leave less room than that bar needs -- oracle 2.5e-5, the reference's fp32 arithmetic 4.3e-5 off the fp64
        # evaluation, TOL / 4 asked -- and tests/test_hip_tangent.py holds a loud tone without an offset to it (loud_tone_n1024)
        if name != "g6_tone_dc":
            from oracle import torch_restatement as R
            from tangent_cases import assert_tangent
            _, _, sc = R.tangent_fp64(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                      case["normalize_window"], log=log)
            assert_tangent(f"tangent/elementwise/{name}/{'log' if log else 'lin'}", t, t_ref, sc, shape=t.shape)


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g6_n256_ragged", "g5_n128", "g6_n32", "g6_n2048_short", "g3_c3", "g5_n4096"])
def test_inference_path_equals_training_path(name):
    """Without a trainable lambd two frames share one FFT; results must agree with the tangent-carrying kernel."""
    case = C.BY_NAME[name]
    x = torch.from_numpy(C.make_input(case).astype(np.float32)).to("cuda:0")
    a = _layer(case, log=True, trainable=True)(x)
    with torch.no_grad():
        b = _layer(case, log=True, trainable=False)(x)
    assert not b.requires_grad
    assert float((a.detach() - b).abs().max()) <= 2e-5


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g5_n128", "g6_n256_ragged", "g6_n2048_short", "g5_n4096"])
def test_spectrogram_stage(name):
    """Framing + window + FFT + |.|^2 alone (time_frequency.py:32-58) against the oracle."""
    case = C.BY_NAME[name]
    x_np = C.make_input(case).astype(np.float32)
    from dmel_amd import capi
    plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"])
    n = capi.n_fft(case["lambd"])
    spec = torch.empty((case["B"], n // 2 + 1, case["L"] // case["hop"] + 1), dtype=torch.float32, device="cuda:0")
    x = torch.from_numpy(x_np).to("cuda:0")
    for dc in (False, True):
        plan.spectrogram(x.data_ptr(), case["B"], case["lambd"], spec.data_ptr(), torch.cuda.current_stream().cuda_stream, remove_dc=dc)
        torch.cuda.synchronize()
        ref = O.spectrogram(x_np, case["lambd"], case["hop"], remove_dc=dc)
        # single FFT bins (no mel averaging) sit on the fp32 FFT noise floor earlier than mel bands do: torch's own
        # CPU fp32 stft is 1.16e-4 off the fp64 oracle on g2_c2 with the 1e-6 floor and 2.4e-5 with 1e-5
        assert _rel_err(spec.cpu().numpy(), ref, floor=1e-5) <= TOL


def test_tiny_nfft_uses_direct_dft_kernel():
    for lam, n in ((2.0, 16), (0.7, 4), (0.0, 2), (0.2, 1)):
        case = dict(C.BY_NAME["g6_n32"], lambd=lam)
        x_np = C.make_input(case).astype(np.float32)
        layer = _layer(case, log=True)
        assert layer.n_fft() == n
        y = layer(torch.from_numpy(x_np).to("cuda:0"))
        assert layer.plan_info()["kernel_path"] == 1
        y_ref, t_ref = O.forward(x_np, lam, case["hop"], case["n_mels"], case["sr"], apply_log=True)
        assert float(np.abs(y.detach().cpu().numpy() - y_ref).max()) <= TOL
        g = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")
        (y * g).sum().backward()
        ref = O.backward(C.make_cotangent(case), t_ref)
        assert abs(float(layer.lambd.grad) - ref) <= TOL * abs(ref) + 1e-6


def test_dense_custom_filterbank():
    """A dense (non-banded) matrix exercises every MFMA block: mel = fb^T P with P from the spectrogram stage."""
    case = C.BY_NAME["g6_n256_ragged"]
    from dmel_amd import capi
    x_np = C.make_input(case).astype(np.float32)
    x = torch.from_numpy(x_np).to("cuda:0")
    n = capi.n_fft(case["lambd"])
    F, M, T, B = n // 2 + 1, case["n_mels"], case["L"] // case["hop"] + 1, case["B"]
    rng = np.random.default_rng(5)
    fb = rng.uniform(-1.0, 1.0, size=(F, M)).astype(np.float32)
    plan = capi.Plan(case["L"], case["hop"], M, case["sr"])
    plan.set_filterbank(n, fb)
    out = torch.empty((B, 1, M, T), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    plan.forward(x.data_ptr(), B, case["lambd"], out.data_ptr(), None, False, 1e-10, s)
    torch.cuda.synchronize()
    info = plan.info()
    assert info["fb_blocks"] == info["fb_blocks_dense"]
    P = O.spectrogram(x_np, case["lambd"], case["hop"], remove_dc=True).astype(np.float64)      # (B,F,T)
    ref = np.einsum("fm,bft->bmt", fb.astype(np.float64), P)[:, None]
    err = np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err <= 2e-5
    plan.set_filterbank(n, None)
    plan.forward(x.data_ptr(), B, case["lambd"], out.data_ptr(), None, False, 1e-10, s)
    torch.cuda.synchronize()
    o_ref, _ = O.forward(x_np, case["lambd"], case["hop"], M, case["sr"], want_tangent=False)
    assert _rel_err(out.cpu().numpy(), o_ref) <= TOL


def test_error_behaviour():
    from dmel_amd import MelSpectrogramLayer, capi
    case = C.BY_NAME["g1_c1"]
    layer = _layer(case)
    with pytest.raises(RuntimeError):       # the reference raises RuntimeError on a length mismatch too
        layer(torch.zeros(2, case["L"] + 1, device="cuda:0"))
    with pytest.raises(ValueError):
        layer(torch.zeros(case["L"], device="cuda:0"))
    with pytest.raises(RuntimeError):
        layer(torch.zeros(2, case["L"]))      # CPU tensor: no fallback
    big = _layer(dict(case, lambd=200000.0), trainable=False)   # n_fft 2097152: beyond the 2^20-point FFT of the big path
    big.lambd_sync = True
    with pytest.raises(RuntimeError, match="the HIP path stops at"):
        big(torch.zeros(1, case["L"], device="cuda:0"))
    # empty batch and non-contiguous / fp64 input are fine
    assert layer(torch.zeros(0, case["L"], device="cuda:0")).shape == (0, 1, case["n_mels"], case["L"] // case["hop"] + 1)
    x = torch.from_numpy(C.make_input(case)).to("cuda:0")
    xt = torch.stack([x, x], dim=2)[:, :, 0]
    assert not xt.is_contiguous()
    assert torch.equal(layer(xt), layer(x))
    # (fp64 clips lose their mean in fp64 before the cast, as models.py:38 does in the input dtype: the same values up to the rounding of x - mean)
    yd, yf = layer(x.double()).detach(), layer(x).detach()
    assert float(((yd - yf).abs() / yf.abs().clamp_min(1e-30)).max()) <= 2e-5


def test_state_dict_and_param_groups():
    case = C.BY_NAME["g1_c1"]
    layer = _layer(case)
    assert list(layer.state_dict().keys()) == ["lambd"]                  # utils.py:270 strict load
    other = _layer(dict(case, lambd=10.0))
    other.load_state_dict(layer.state_dict(), strict=True)
    assert float(other.lambd) == case["lambd"]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.spectrogram_layer = layer
            self.fc = torch.nn.Linear(4, 2)
    names = [n for n, _ in Net().named_parameters()]
    assert "spectrogram_layer.lambd" in names                            # main.py:39


# ---- full BASELINE size (config 2): properties that need no oracle at that size ----------------
def _c2_layer(log=True):
    case = dict(C.BY_NAME["g2_c2"])
    return _layer(case, log=log), case


def test_c2_full_size_properties():
    from dmel_amd import synth
    layer, case = _c2_layer(log=False)
    B = 256
    x_np = synth.waveforms(B, case["L"], seed=0)
    x = torch.from_numpy(x_np).to("cuda:0")
    g = torch.from_numpy(synth.cotangent((B, 1, case["n_mels"], case["L"] // case["hop"] + 1), seed=1)).to("cuda:0")
    mel = layer(x)
    (mel * g).sum().backward()
    d_full = float(layer.lambd.grad)
    # (1) |.|^2 is homogeneous of degree 2 and every step scales exactly by powers of two
    mel2 = layer(2.0 * x)
    assert torch.equal(mel2, 4.0 * mel)
    # (2) clips are independent: permuting the batch permutes the output bit for bit
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    assert torch.equal(layer(x[perm]), mel[perm])
    # (3) the gradient is additive over batch shards (what the multi-GPU all-reduce relies on)
    parts = 0.0
    for sl in (slice(0, 96), slice(96, 256)):
        layer.lambd.grad = None
        (layer(x[sl]) * g[sl]).sum().backward()
        parts += float(layer.lambd.grad)
    assert abs(parts - d_full) <= 1e-5 * abs(d_full) + 1e-6
    # (4) eight clips spread over the batch against the oracle
    pick = [0, 1, 37, 100, 128, 200, 254, 255]
    ref, tref = O.forward(x_np[pick], case["lambd"], case["hop"], case["n_mels"], case["sr"])
    assert _rel_err(mel.detach().cpu().numpy()[pick], ref) <= TOL
    # (5) run-to-run determinism, forward and backward
    layer.lambd.grad = None
    m3 = layer(x)
    (m3 * g).sum().backward()
    assert torch.equal(m3, mel) and float(layer.lambd.grad) == d_full
    # (6) finite-difference check of d lambd in fp32 (loose: the loss is fp32)
    lg, _ = _c2_layer(log=True)
    y = lg(x[:32]); (y * g[:32]).sum().backward()
    ana = float(lg.lambd.grad)
    h = 0.25
    with torch.no_grad():
        lp, _ = _c2_layer(log=True); lp.lambd += h
        lm, _ = _c2_layer(log=True); lm.lambd -= h
        num = float(((lp(x[:32]).double() - lm(x[:32]).double()) * g[:32].double()).sum()) / (2 * h)
    assert abs(num - ana) <= 2e-2 * abs(ana) + 1e-3


@pytest.mark.parametrize("cname,B", [("g2_c2", 256), ("g3_c3", 8)])
def test_xgrad_full_size_properties(cname, B, monkeypatch):
    """dL/dx at BASELINE sizes (config 2: n_fft 1024, the kernel adds up its clip itself; config 3: n_fft 2048, partial sums from the
    prep kernel), through properties that need no oracle pass over the whole batch: the wave-FFT kernels against the LDS radix-2
    kernels (two independent implementations of the same adjoint), exact linearity in the cotangent, zero sum per clip (the
    adjoint of the DC removal), independence of the clips, determinism; a few clips against the oracle."""
    from dmel_amd import synth, capi
    case = dict(C.BY_NAME[cname])
    L, hop, M, sr, lam = case["L"], case["hop"], case["n_mels"], case["sr"], case["lambd"]
    T = L // hop + 1
    x_np = synth.waveforms(B, L, seed=11)
    g_np = synth.cotangent((B, 1, M, T), seed=12)
    x = torch.from_numpy(x_np).to("cuda:0")
    g = torch.from_numpy(g_np).to("cuda:0")
    plan = capi.Plan(L, hop, M, sr)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((B, 1, M, T), device="cuda:0")
    plan.forward(x.data_ptr(), B, lam, y.data_ptr(), None, True, 1e-10, st)

    def gx_of(xx, gg, yy, log=True):
        out = torch.empty_like(xx)
        plan.backward_x(xx.data_ptr(), xx.shape[0], lam, gg.data_ptr(), yy.data_ptr(), out.data_ptr(), log, st)
        torch.cuda.synchronize()
        return out

    gx = gx_of(x, g, y)
    scale = float(gx.abs().max())
    assert torch.isfinite(gx).all() and scale > 0
    # (1) the other implementation of the same adjoint (LDS radix-2 transforms, one row per frame, ordered gather)
    monkeypatch.setenv("DMEL_XGRAD_LDS", "1")
    gx_lds = gx_of(x, g, y)
    monkeypatch.delenv("DMEL_XGRAD_LDS")
    assert float((gx - gx_lds).abs().max()) <= TOL * scale                        # (two fp32 transforms of different structure: 3e-5 measured)
    # (2) window and clip mean from the prep kernel instead of the kernel's own prologue (config 2 only takes the latter by default)
    monkeypatch.setenv("DMEL_XGRAD_PREP", "1")
    gx_prep = gx_of(x, g, y)
    monkeypatch.delenv("DMEL_XGRAD_PREP")
    assert float((gx - gx_prep).abs().max()) <= 0.2 * TOL * scale
    # (3) linear in the cotangent, and powers of two pass through every step exactly
    assert torch.equal(gx_of(x, 2.0 * g, y), 2.0 * gx)
    # (4) zero sum per clip
    assert float(gx.double().sum(1).abs().max()) <= 1e-4 * float(gx.double().abs().sum(1).max())
    # (5) clips are independent, run-to-run determinism
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to("cuda:0")
    assert torch.equal(gx_of(x[perm].contiguous(), g[perm].contiguous(), y[perm].contiguous()), gx[perm])
    assert torch.equal(gx_of(x, g, y), gx)
    # (6) a few clips against the oracle
    pick = [0, B // 2, B - 1]
    ref = O.backward_x(x_np[pick], lam, hop, sr, g_np[pick], y.cpu().numpy()[pick], case["f_min"], case["f_max"], case["normalize_window"])
    assert _gx_err(gx.cpu().numpy()[pick], ref) <= TOL


# ---- the nets that call the layer, and the two-LR-group training step ---------------
@pytest.mark.parametrize("net_name", ["MelLinearNet", "MelMlpNet", "MelConvNet"])
def test_caller_nets_train_step(net_name):
    from dmel_amd import nets
    torch.manual_seed(0)
    B, L, sr, hop, M, ncls = 6, 8000, 8000, 80, 64, 10
    net = getattr(nets, net_name)(ncls, torch.tensor(8000 * 0.035 / 6), "cuda:0", M, sr, L, hop_length=hop, optimized=True,
                                  energy_normalize=True).to("cuda:0")
    names = [n for n, _ in net.named_parameters()]
    assert names[0] == "spectrogram_layer.lambd"
    opt = nets.make_optimizer(net, lr_model=1e-4, lr_tf=1.0)
    assert [g["lr"] for g in opt.param_groups][0] == 1.0 and all(g["lr"] == 1e-4 for g in opt.param_groups[1:])
    from dmel_amd import synth
    x = torch.from_numpy(synth.waveforms(B, L, seed=5)).to("cuda:0")
    y = torch.arange(B, device="cuda:0") % ncls
    lam0 = float(net.spectrogram_layer.lambd)
    logits, s = net(x)
    assert logits.shape == (B, ncls) and s.shape == (B, 1, M, L // hop + 1)
    ref, _ = O.forward(x.cpu().numpy(), lam0, hop, M, sr, apply_log=True, want_tangent=False)
    assert float(np.abs(s.detach().cpu().numpy() - ref).max()) <= TOL          # s is log(mel + 1e-10), models.py:73
    loss = torch.nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    g = net.spectrogram_layer.lambd.grad
    assert g is not None and torch.isfinite(g) and float(g) != 0.0
    opt.step()
    assert float(net.spectrogram_layer.lambd) != lam0
    # frozen front end (main.py:27): no tangent is produced and no gradient reaches lambd
    net.spectrogram_layer.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    logits, s = net(x)
    torch.nn.CrossEntropyLoss()(logits, y).backward()
    assert net.spectrogram_layer.lambd.grad is None


# ---- DSPEC SpectrogramLayer -------------------------------------------------------------
def test_dspec_layer_matches_reference_and_oracle():
    import os
    from dmel_amd import SpectrogramLayer, synth
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_dspec.npz"))
    x_np = synth.waveforms(2, 128, seed=77, scale=1.0)
    layer = SpectrogramLayer(torch.tensor(6.38), optimized=False, hop_length=1).to("cuda:0")
    assert list(layer.state_dict().keys()) == ["lambd"]
    s = layer(torch.from_numpy(x_np).to("cuda:0"))
    assert s.shape == (2, 1, 129, 129)
    assert _rel_err(s.detach().cpu().numpy(), gold["spec"]) <= TOL
    g_np = synth.cotangent(tuple(s.shape), seed=78)
    (s * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
    ref_s, ref_t = O.dspec(x_np, 6.38, hop=1)
    assert _rel_err(s.detach().cpu().numpy(), ref_s) <= TOL
    exp_d = float(gold["dlam_lin"])
    assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, ref_t)
    # normalised window, other hop, power-of-two lengths from 16 to 1024
    # (n_fft = 2L: 2048 and 4096 run the compact layout of the fused kernel with the half-length window)
    for L, hop, lam, norm in ((16, 1, 2.5, False), (64, 3, 5.0, True), (256, 8, 20.0, False), (1024, 64, 90.0, True),
                              (1024, 100, -70.0, False), (2048, 128, 200.0, True), (4096, 300, 500.0, False), (8192, 900, -900.0, True)):
        xn = synth.waveforms(3, L, seed=L, scale=1.0)
        lay = SpectrogramLayer(torch.tensor(lam), optimized=False, hop_length=hop, normalize_window=norm).to("cuda:0")
        out = lay(torch.from_numpy(xn).to("cuda:0"))
        rs, rt = O.dspec(xn, lam, hop=hop, normalize_window=norm)
        assert out.shape == rs.shape
        assert _rel_err(out.detach().cpu().numpy(), rs) <= TOL
        gn = synth.cotangent(rs.shape, seed=L + 1)
        (out * torch.from_numpy(gn).to("cuda:0")).sum().backward()
        ref = O.backward(gn, rt)
        assert abs(float(lay.lambd.grad) - ref) <= _dlam_tol(ref, gn, rt)
    # clip lengths that are not powers of two (n_fft = 2L through the chirp-z path): the reference's own output at L = 100,
    # the oracle at an odd length and at Audio-MNIST's 8000 samples (n_fft 16000: the sequence lives in global memory)
    gold100 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_dspec_100.npz"))
    x100 = synth.waveforms(2, 100, seed=77, scale=1.0)
    lay = SpectrogramLayer(torch.tensor(6.38), optimized=False, hop_length=1).to("cuda:0")
    s100 = lay(torch.from_numpy(x100).to("cuda:0"))
    # single FFT bins (no mel averaging) meet the fp32 noise floor of a chirp-z transform earlier than mel bands do: measured
    # against a floor of 1e-5 of the loudest bin, as test_spectrogram_stage does (torch's own fp32 stft is 1.2e-4 off the fp64
    # oracle at a floor of 1e-6)
    assert s100.shape == (2, 1, 101, 101) and _rel_err(s100.detach().cpu().numpy(), gold100["spec"], floor=1e-5) <= TOL
    g100 = synth.cotangent(tuple(s100.shape), seed=78)
    (s100 * torch.from_numpy(g100).to("cuda:0")).sum().backward()
    _, rt100 = O.dspec(x100, 6.38, hop=1)
    assert abs(float(lay.lambd.grad) - float(gold100["dlam_lin"])) <= _dlam_tol(float(gold100["dlam_lin"]), g100, rt100)
    for L, hop, lam, norm in ((77, 5, 9.0, True), (8000, 400, 300.0, False)):
        xn = synth.waveforms(2, L, seed=L, scale=1.0)
        lay = SpectrogramLayer(torch.tensor(lam), optimized=False, hop_length=hop, normalize_window=norm).to("cuda:0")
        out = lay(torch.from_numpy(xn).to("cuda:0"))
        rs, rt = O.dspec(xn, lam, hop=hop, normalize_window=norm)
        assert out.shape == rs.shape and _rel_err(out.detach().cpu().numpy(), rs, floor=1e-5) <= TOL
        gn = synth.cotangent(rs.shape, seed=L + 1)
        (out * torch.from_numpy(gn).to("cuda:0")).sum().backward()
        ref = O.backward(gn, rt)
        assert abs(float(lay.lambd.grad) - ref) <= _dlam_tol(ref, gn, rt)
    # optimized branch: the mel layer's STFT without the filterbank; size must equal (F, T)
    case = C.BY_NAME["g5_n128"]
    xo = C.make_input(case).astype(np.float32)
    n = O.n_fft(case["lambd"])
    lay = SpectrogramLayer(torch.tensor(float(case["lambd"])), optimized=True, size=(n // 2 + 1, case["L"] // case["hop"] + 1),
                           hop_length=case["hop"]).to("cuda:0")
    so = lay(torch.from_numpy(xo).to("cuda:0"))
    assert _rel_err(so.detach().cpu().numpy()[:, 0], O.spectrogram(xo, case["lambd"], case["hop"], remove_dc=True)) <= TOL


@pytest.mark.parametrize("sync", [False, True])
def test_lambd_updates_are_always_seen(sync):
    """Neither path caches lambd on the host: in-place updates, writes through .data (which bump no version counter) and
    a replaced storage all reach the next forward.  (Round 1 cached the host value on (_version, data_ptr).)"""
    from dmel_amd import MelSpectrogramLayer
    case = C.BY_NAME["g1_c1"]
    layer = MelSpectrogramLayer(torch.tensor(64.0), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                hop_length=case["hop"], device="cuda:0", optimized=True, lambd_sync=sync).to("cuda:0")
    layer.set_tracking(8, 1)          # sync-free path: both neighbouring n_fft guarded, so a doubling / halving is covered
    x_np = C.make_input(case)
    x = torch.from_numpy(x_np).to("cuda:0")

    def ref(lam):
        return O.forward(x_np, lam, case["hop"], case["n_mels"], case["sr"], want_tangent=False)[0]

    y0 = layer(x)
    assert layer.n_fft() == 512 and _rel_err(y0.detach().cpu().numpy(), ref(64.0)) <= TOL
    with torch.no_grad():
        layer.lambd.mul_(2.0)                      # what optimizer.step() does: an in-place update
    y1 = layer(x)
    assert layer.n_fft() == 1024 and _rel_err(y1.detach().cpu().numpy(), ref(128.0)) <= TOL
    layer.lambd.data.mul_(0.5)                     # no version bump, same storage
    y2 = layer(x)
    assert _rel_err(y2.detach().cpu().numpy(), ref(64.0)) <= TOL and torch.equal(y2, y0)
    layer.lambd.data.fill_(100.0)
    assert _rel_err(layer(x).detach().cpu().numpy(), ref(100.0)) <= TOL
    layer.lambd.data = torch.tensor(64.0, device="cuda:0")      # replacing the storage is seen too
    assert torch.equal(layer(x), y0)


def test_c3_full_size_properties():
    """BASELINE config 3 at full size (32 x 160000, n_fft 2048): long clips take the partial-sum kernel path."""
    from dmel_amd import synth
    case = dict(C.BY_NAME["g3_c3"])
    layer = _layer(case, log=True)
    B = 32
    x_np = synth.waveforms(B, case["L"], seed=0)
    x = torch.from_numpy(x_np).to("cuda:0")
    T = case["L"] // case["hop"] + 1
    g = torch.from_numpy(synth.cotangent((B, 1, case["n_mels"], T), seed=1)).to("cuda:0")
    y = layer(x)
    (y * g).sum().backward()
    d_full = float(layer.lambd.grad)
    pick = [0, 17, 31]
    ref, tref = O.forward(x_np[pick], case["lambd"], case["hop"], case["n_mels"], case["sr"], apply_log=True)
    assert _log_err(y.detach().cpu().numpy()[pick], ref) <= TOL
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(4)).to("cuda:0")
    assert torch.equal(layer(x[perm]), y[perm])
    layer.lambd.grad = None
    y2 = layer(x); (y2 * g).sum().backward()
    assert torch.equal(y2, y) and float(layer.lambd.grad) == d_full
    parts = 0.0
    for sl in (slice(0, 5), slice(5, 32)):
        layer.lambd.grad = None
        (layer(x[sl]) * g[sl]).sum().backward()
        parts += float(layer.lambd.grad)
    assert abs(parts - d_full) <= 1e-5 * abs(d_full) + 1e-5


def test_native_scalar_allreduce_world1():
    """dmel_comm_* (RCCL through the C ABI) on a single-rank communicator: SUM over one rank is the identity, the
    ticket/wait ordering against the caller's stream must hold.  (Multi-rank RCCL cannot be exercised on one GPU.)"""
    from dmel_amd import capi
    try:
        uid = capi.Comm.unique_id()
    except capi.DmelError as e:
        pytest.skip(f"RCCL not loadable: {e}")
    comm = capi.Comm(uid, 0, 1)
    s = torch.cuda.current_stream().cuda_stream
    bufs = [torch.full((4,), float(i + 1), device="cuda:0") for i in range(70)]     # more than the 64-ticket ring
    tickets = []
    for i, b in enumerate(bufs):
        b.mul_(2.0)                                   # queued on the caller's stream BEFORE the collective
        tickets.append(comm.allreduce_async(b.data_ptr(), b.numel(), s))
        comm.wait(tickets[-1], s)
        b.add_(1.0)                                   # queued AFTER the wait
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert torch.equal(b.cpu(), torch.full((4,), 2.0 * (i + 1) + 1.0))
    assert all(0 <= t < 64 for t in tickets)
    comm.close()


# ---- gradient w.r.t. the filterbank ("mel params", adjoint of models.py:53) ------------------------------------
def _gfb_err(got, exp):
    return float(np.abs(got.astype(np.float64) - exp).max() / (np.abs(exp).max() + 1e-30))


def _assert_gfb_elementwise(tag, got, case, x_np, g_np, out, optimized=True, lengths=None):
    """beside _gfb_err (one maximum over the largest element of the tensor: blind to up to 98 % of it, tests/fbgrad_cases.py): the gradient
    against oracle/torch_restatement.py: fbgrad_fp64 given the saved log output `out` (None: linear), |got - ref| over the cancellation-free
    magnitude of the element, TOL on every element.  tests/test_fbgrad_restatement_cpu.py holds the references to TOL / 4 on the inputs of
    every site that calls this."""
    from fbgrad_cases import assert_fbgrad
    from oracle import torch_restatement as R
    ref, sc = R.fbgrad_fp64(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], g_np, out, case["f_min"], case["f_max"],
                            case["normalize_window"], optimized=optimized, lengths=lengths)
    return assert_fbgrad(tag, got, ref, sc, shape=ref.shape)


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g5_n128", "g6_n256_ragged"])
def test_fbgrad_matches_reference_golden(name):
    """dmel_backward_fb against torch autograd through the reference with mel_fb made a leaf (g8_fbgrad_*.npz)
    and against the fp64 oracle."""
    import os
    from dmel_amd import capi
    case = C.BY_NAME[name]
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g8_fbgrad_{name}.npz"))
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    g = torch.from_numpy(g_np).to("cuda:0")
    plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
    st = torch.cuda.current_stream().cuda_stream
    n = capi.n_fft(case["lambd"])
    y = torch.empty(C.out_shape(case), dtype=torch.float32, device="cuda:0")
    plan.forward(x.data_ptr(), case["B"], case["lambd"], y.data_ptr(), None, True, 1e-10, st)
    for log, key in ((False, "gfb_lin"), (True, "gfb_log")):
        gfb = torch.full((n // 2 + 1, case["n_mels"]), float("nan"), dtype=torch.float32, device="cuda:0")
        plan.backward_fb(x.data_ptr(), case["B"], case["lambd"], g.data_ptr(), y.data_ptr() if log else None, gfb.data_ptr(), log, st)
        torch.cuda.synchronize()
        got = gfb.cpu().numpy()
        assert np.isfinite(got).all()
        assert _gfb_err(got, gold[key].astype(np.float64)) <= TOL
        ref = O.backward_fb(x_np, case["lambd"], case["hop"], g_np, y.cpu().numpy() if log else None, case["normalize_window"])
        assert _gfb_err(got, ref) <= TOL
        _assert_gfb_elementwise(f"fbgrad_golden/{name}/{'log' if log else 'lin'}", got, case, x_np, g_np, y.cpu().numpy() if log else None)
        # deterministic: same bits on a second call
        gfb2 = torch.empty_like(gfb)
        plan.backward_fb(x.data_ptr(), case["B"], case["lambd"], g.data_ptr(), y.data_ptr() if log else None, gfb2.data_ptr(), log, st)
        assert torch.equal(gfb, gfb2)


def test_learnable_filterbank_layer():
    from dmel_amd import MelSpectrogramLayer, capi
    case = C.BY_NAME["g1_c1"]
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    g = torch.from_numpy(g_np).to("cuda:0")
    base = _layer(case, log=True)
    lay = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                              hop_length=case["hop"], device="cuda:0", optimized=True, log=True, learnable_fb=True).to("cuda:0")
    assert sorted(k for k, _ in lay.named_parameters()) == ["lambd", "mel_fb"]
    assert sorted(base.state_dict().keys()) == ["lambd"]                      # default layer keeps the reference's checkpoint keys
    n = capi.n_fft(case["lambd"])
    assert tuple(lay.mel_fb.shape) == (n // 2 + 1, case["n_mels"])
    y0, y1 = base(x), lay(x)
    assert float((y0 - y1).detach().abs().max()) <= 1e-5                       # same bank, dense tables instead of banded ones
    (y1 * g).sum().backward()
    (y0 * g).sum().backward()
    assert abs(float(lay.lambd.grad) - float(base.lambd.grad)) <= 1e-4 * abs(float(base.lambd.grad)) + 1e-6
    ref = O.backward_fb(x_np, case["lambd"], case["hop"], g_np, y1.detach().cpu().numpy())
    assert _gfb_err(lay.mel_fb.grad.cpu().numpy(), ref) <= TOL
    # an optimizer step on the bank is picked up by the next forward: compare with spec^T @ fb done by torch
    with torch.no_grad():
        lay.mel_fb.add_(0.01 * torch.rand_like(lay.mel_fb))
    y2 = lay(x).detach()
    spec = torch.empty((case["B"], n // 2 + 1, lay.n_time), dtype=torch.float32, device="cuda:0")
    lay._plan_for(x.device).spectrogram(x.data_ptr(), case["B"], case["lambd"], spec.data_ptr(), torch.cuda.current_stream().cuda_stream, remove_dc=True)
    ref2 = torch.log(torch.einsum("bft,fm->bmt", spec.double(), lay.mel_fb.detach().double()) + 1e-10).unsqueeze(1)
    assert float((y2.double() - ref2).abs().max()) <= TOL
    # ... and so is a write through .data (no version bump): the tables are refreshed from the storage at every forward
    lay.mel_fb.data.mul_(1.25)
    y3 = lay(x).detach()
    ref3 = torch.log(torch.einsum("bft,fm->bmt", spec.double(), lay.mel_fb.detach().double()) + 1e-10).unsqueeze(1)
    assert float((y3.double() - ref3).abs().max()) <= TOL and not torch.equal(y3, y2)
    # the bank is tied to its n_fft.  Sync-free layer: the kernel finds the mismatch (NaN, never a result from the wrong
    # matrix) and the next forward raises; lambd_sync=True raises at once, like the shape error of models.py:53
    with torch.no_grad():
        lay.lambd.fill_(3.0 * float(case["lambd"]))
    y4 = lay(x)
    torch.cuda.synchronize()
    assert torch.isnan(y4).all()
    with pytest.raises(RuntimeError, match="tied to one n_fft"):
        lay(x)
    with torch.no_grad():
        lay.lambd.fill_(float(case["lambd"]))
    assert torch.equal(lay(x).detach(), y3)                                      # back inside its n_fft: works again
    strict = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                 hop_length=case["hop"], device="cuda:0", optimized=True, log=True, learnable_fb=True,
                                 lambd_sync=True).to("cuda:0")
    y5 = strict(x)
    assert float((y5 - y0).detach().abs().max()) <= 1e-5
    with torch.no_grad():
        strict.lambd.fill_(3.0 * float(case["lambd"]))
    with pytest.raises(RuntimeError, match="tied to one n_fft"):
        strict(x)


@pytest.mark.parametrize("name", ["g1_c1", "g5_n128", "g6_n2048_short"])
def test_xgrad_through_a_trained_dense_filterbank(name):
    """x.requires_grad with learnable_fb=True after the bank has moved: every row of the matrix is dense, so the waveform
    gradient takes the first two columns from the packed rows (refreshed on the device with the other tables) and the rest
    from the matrix itself; against the oracle with the same matrix."""
    from dmel_amd import MelSpectrogramLayer
    case = C.BY_NAME[name]
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to("cuda:0")
    for log in (False, True):
        lay = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                  f_min=case["f_min"], f_max=case["f_max"], hop_length=case["hop"], device="cuda:0", optimized=True,
                                  normalize_window=case["normalize_window"], log=log, learnable_fb=True).to("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(7)
        with torch.no_grad():
            lay.mel_fb.add_((0.02 * torch.rand(lay.mel_fb.shape, generator=gen)).to("cuda:0"))
        fb_np = lay.mel_fb.detach().cpu().numpy()
        for _ in range(2):                                                       # second pass: the bank moves again, same tables
            x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
            y = lay(x)
            (y * g).sum().backward()
            ref = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y.detach().cpu().numpy() if log else None,
                               case["f_min"], case["f_max"], case["normalize_window"], fb=fb_np)
            assert _gx_err(x.grad.cpu().numpy(), ref) <= TOL
            with torch.no_grad():
                lay.mel_fb.mul_(1.1)
            fb_np = lay.mel_fb.detach().cpu().numpy()
            lay.mel_fb.grad = None


def test_trainable_filterbank_step_is_sync_free_and_graph_capturable():
    """lambd AND the filterbank trained together: the step (forward with the dense bank refreshed on the device, d lambd,
    d filterbank, Adam on both) queues without a host read and replays from a HIP graph; the replayed parameters equal the
    eagerly stepped ones of a layer that reads lambd on the host at every forward."""
    from dmel_amd import MelSpectrogramLayer
    case = C.BY_NAME["g1_c1"]
    x = torch.from_numpy(C.make_input(case).astype(np.float32)).to("cuda:0")
    g = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")

    def mk(sync):
        return MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                   hop_length=case["hop"], device="cuda:0", optimized=True, log=False, learnable_fb=True,
                                   lambd_sync=sync).to("cuda:0")

    def run(layer, steps, graphed):
        opt = torch.optim.Adam([{"params": [layer.lambd], "lr": 0.05}, {"params": [layer.mel_fb], "lr": 1e-4}], capturable=True)

        def step():
            opt.zero_grad(set_to_none=False)
            layer(x).backward(g)
            opt.step()
        if not graphed:
            for _ in range(steps):
                step()
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            for _ in range(steps - 2):                      # (capturing does not execute)
                graph.replay()
        torch.cuda.synchronize()
        return layer.lambd.detach().cpu().numpy().copy(), layer.mel_fb.detach().cpu().numpy().copy()

    lam_e, fb_e = run(mk(True), 8, False)
    lay = mk(False)
    lam_g, fb_g = run(lay, 8, True)
    assert lay.lambd_status()["error"] == 0
    assert abs(float(lam_e) - float(case["lambd"])) > 0.1                        # the parameters did move
    np.testing.assert_allclose(lam_g, lam_e, rtol=1e-5)
    np.testing.assert_allclose(fb_g, fb_e, rtol=1e-4, atol=1e-6)


_FB_EXTRA = {"n8192": dict(C.BY_NAME["g1_c1"], name="n8192", B=2, L=20000, lambd=900.0, hop=1000, n_mels=40),
             "n2048": dict(C.BY_NAME["g1_c1"], name="n2048", B=2, L=9000, lambd=-250.0, hop=300, n_mels=96)}


@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g5_n128", "g6_n32", "g5_n4096", "n2048", "n8192"])
def test_filterbank_from_device_equals_filterbank_from_host(name):
    """dmel_plan_set_filterbank_dev (one small kernel on the stream, no host copy, no synchronisation) fills the same tables as
    dmel_plan_set_filterbank builds on the host: identical outputs, bit for bit, for a dense random matrix."""
    from dmel_amd import capi
    case = C.BY_NAME[name] if name in C.BY_NAME else _FB_EXTRA[name]
    x = torch.from_numpy(C.make_input(case).astype(np.float32)).to("cuda:0")
    n = capi.n_fft(case["lambd"])
    fb = torch.rand((n // 2 + 1, case["n_mels"]), device="cuda:0") + 0.01
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for dev in (False, True):
        plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"])
        if dev:
            plan.set_filterbank_dev(n, fb.data_ptr(), st)
        else:
            plan.set_filterbank(n, fb.cpu().numpy())
        out = torch.empty(C.out_shape(case), device="cuda:0"); tan = torch.empty_like(out)
        plan.forward(x.data_ptr(), case["B"], case["lambd"], out.data_ptr(), tan.data_ptr(), True, 1e-10, st)
        if dev:                                   # a second matrix through the same plan: only the repack kernel runs
            fb2 = fb * 0.5
            plan.set_filterbank_dev(n, fb2.data_ptr(), st)
            out2 = torch.empty_like(out)
            plan.forward(x.data_ptr(), case["B"], case["lambd"], out2.data_ptr(), None, False, 1e-10, st)
            out1 = torch.empty_like(out)
            plan.set_filterbank_dev(n, fb.data_ptr(), st)
            plan.forward(x.data_ptr(), case["B"], case["lambd"], out1.data_ptr(), None, False, 1e-10, st)
            torch.cuda.synchronize()
            assert torch.equal(out2, 0.5 * out1)  # the contraction is linear in the matrix, and halving is exact
        torch.cuda.synchronize()
        outs.append((out, tan))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_backward_fb_rejects_bad_arguments():
    from dmel_amd import capi
    plan = capi.Plan(4000, 40, 20, 8000)
    x = torch.zeros((2, 4000), device="cuda:0")
    g = torch.zeros((2, 1, 20, 101), device="cuda:0")
    gfb = torch.zeros((33, 20), device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(capi.DmelError):
        plan.backward_fb(x.data_ptr(), 2, 9.0, g.data_ptr(), None, gfb.data_ptr(), True, st)        # log without the saved output
    with pytest.raises(capi.DmelError):
        plan.backward_fb(x.data_ptr(), 2, 200000.0, g.data_ptr(), None, gfb.data_ptr(), False, st)   # n_fft 2097152: beyond the HIP path
    plan.backward_fb(x.data_ptr(), 0, 9.0, g.data_ptr(), None, gfb.fill_(1.0).data_ptr(), False, st)   # empty batch: zeros
    torch.cuda.synchronize()
    assert float(gfb.abs().max()) == 0.0


# ---- long transforms: n_fft 8192 / 16384 (one frame per workgroup, radix-2 FFT in LDS) ---------------------------
LONG_CASES = [
    dict(C.BY_NAME["g6_fminmax"], name="long_8192", L=12000, lambd=700.0, hop=600, n_mels=40),
    dict(C.BY_NAME["g1_c1"], name="long_16384", B=2, L=20001, lambd=-1500.0, hop=997, n_mels=64, normalize_window=True),
    # the reference's ESC-50 clip (search_spaces.py:31) after lambd has drifted from 400 past 682: partial sums from the prep kernel
    dict(C.BY_NAME["g1_c1"], name="long_8192_esc", B=2, L=40000, lambd=800.0, hop=1600, n_mels=64, sr=8000),
]


@pytest.mark.parametrize("case", LONG_CASES, ids=[c["name"] for c in LONG_CASES])
def test_long_transform_matches_oracle(case):
    from dmel_amd import capi
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    n = capi.n_fft(case["lambd"])
    assert n in (8192, 16384)
    for log in (False, True):
        layer = _layer(case, log=log)
        y = layer(x)
        assert layer.plan_info()["kernel_path"] == 0 and layer.plan_info()["n_fft"] == n     # fused kernel, several waves per frame
        (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
        o_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                 case["normalize_window"], apply_log=log)
        o = y.detach().cpu().numpy()
        assert (_log_err(o, o_ref) if log else _rel_err(o, o_ref)) <= TOL
        exp_d = O.backward(g_np, t_ref)
        assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, t_ref)
        # inference path: two frames per transform
        with torch.no_grad():
            yi = _layer(case, log=log, trainable=False)(x)
        oi = yi.cpu().numpy()
        assert (_log_err(oi, o_ref) if log else _rel_err(oi, o_ref)) <= TOL
    # spectrogram stage and filterbank gradient run on the same kernel
    plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
    st = torch.cuda.current_stream().cuda_stream
    spec = torch.empty((case["B"], n // 2 + 1, case["L"] // case["hop"] + 1), dtype=torch.float32, device="cuda:0")
    plan.spectrogram(x.data_ptr(), case["B"], case["lambd"], spec.data_ptr(), st, remove_dc=True)
    torch.cuda.synchronize()
    ref = O.spectrogram(x_np, case["lambd"], case["hop"], normalize_window=case["normalize_window"], remove_dc=True)
    assert _rel_err(spec.cpu().numpy(), ref, floor=1e-5) <= TOL
    g = torch.from_numpy(g_np).to("cuda:0")
    gfb = torch.empty((n // 2 + 1, case["n_mels"]), dtype=torch.float32, device="cuda:0")
    plan.backward_fb(x.data_ptr(), case["B"], case["lambd"], g.data_ptr(), None, gfb.data_ptr(), False, st)
    torch.cuda.synchronize()
    assert _gfb_err(gfb.cpu().numpy(), O.backward_fb(x_np, case["lambd"], case["hop"], g_np, None, case["normalize_window"])) <= TOL


def test_full_window_branch_up_to_8192_points():
    """optimized=False (window = whole clip, n_fft = 2 * n_points) at n_points 4096: n_fft 8192, two waves per frame in the fused kernel."""
    case = dict(C.BY_NAME["g7_mel_nonopt_1024n"], name="nonopt_4096", L=4096, lambd=300.0, hop=256, normalize_window=False)
    x_np = C.make_input(case).astype(np.float32)
    layer = _layer(case, log=True)
    y = layer(torch.from_numpy(x_np).to("cuda:0"))
    assert layer.plan_info()["kernel_path"] == 0 and layer.plan_info()["n_fft"] == 8192
    y_ref, _ = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                         case["normalize_window"], apply_log=True, optimized=False)
    assert _log_err(y.detach().cpu().numpy(), y_ref) <= TOL


def test_full_window_branch_at_config5_clip_length():
    """The constructor's DEFAULT branch (models.py:15 optimized=False) on BASELINE config 5's clip: 220 500 samples @ 44.1 kHz ->
    n_fft 441 000 through Bluestein's identity with 2^20-point FFTs in global memory (missing #4).  Two clips, three
    frames (hop = half a clip) against the fp64 oracle, output and d lambd."""
    case = dict(C.BY_NAME["g7_mel_nonopt_8000"], name="nonopt_220500", B=2, L=220500, sr=44100, lambd=9000.0, hop=110250, n_mels=128)
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    layer = _layer(case, log=True)
    y = layer(torch.from_numpy(x_np).to("cuda:0"))
    assert layer.plan_info()["kernel_path"] == 3 and layer.plan_info()["n_fft"] == 441000
    (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
    y_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                             case["normalize_window"], apply_log=True, optimized=False)
    assert _log_err(y.detach().cpu().numpy(), y_ref) <= TOL
    exp_d = O.backward(g_np, t_ref)
    assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, t_ref)


@pytest.mark.parametrize("L,n_fft", [(20000, 40000), (40000, 80000)])
def test_full_window_branch_on_esc50_length_clips(L, n_fft):
    """optimized=False on clips of 20 000 / 40 000 samples (ESC-50's 5 s at 8 kHz): n_fft 40 000 / 80 000 through Bluestein with
    2^17 / 2^18-point FFTs whose first and last four stages run on the sequence in global memory and the rest on 8192 / 16384-point
    blocks in LDS.  Three frames per clip against the fp64 oracle, output and d lambd."""
    case = dict(C.BY_NAME["g7_mel_nonopt_8000"], name=f"nonopt_{L}", B=2, L=L, sr=8000, lambd=1500.0, hop=L // 2, n_mels=64)
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    layer = _layer(case, log=True)
    y = layer(torch.from_numpy(x_np).to("cuda:0"))
    assert layer.plan_info()["kernel_path"] == 3 and layer.plan_info()["n_fft"] == n_fft
    (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
    y_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                             case["normalize_window"], apply_log=True, optimized=False)
    assert _log_err(y.detach().cpu().numpy(), y_ref) <= TOL
    exp_d = O.backward(g_np, t_ref)
    assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, t_ref)


def test_full_window_branch_on_the_compact_layout():
    """optimized=False at n_points 2048: n_fft 4096 on the fused kernel's compact layout, half-length window from the prep kernel."""
    case = dict(C.BY_NAME["g7_mel_nonopt_1024n"], name="nonopt_2048", L=2048, lambd=-150.0, hop=100, normalize_window=True)
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    for log in (False, True):
        layer = _layer(case, log=log)
        y = layer(torch.from_numpy(x_np).to("cuda:0"))
        assert layer.plan_info()["kernel_path"] == 0 and layer.plan_info()["n_fft"] == 4096
        (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
        y_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                 case["normalize_window"], apply_log=log, optimized=False)
        o = y.detach().cpu().numpy()
        assert (_log_err(o, y_ref) if log else _rel_err(o, y_ref)) <= TOL
        exp_d = O.backward(g_np, t_ref)
        assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, t_ref)


# ---- bf16 activations (BASELINE config 2: "bf16 activations / fp32 grad") ----------------------------------------
@pytest.mark.parametrize("name", ["g1_c1", "g2_c2", "g6_n256_ragged", "g6_n32", "g6_n2048_short", "g5_n4096", "n8192"])
def test_bf16_output_is_the_rounded_fp32_output(name):
    from dmel_amd import MelSpectrogramLayer
    case = C.BY_NAME[name] if name in C.BY_NAME else _FB_EXTRA[name]
    x = torch.from_numpy(C.make_input(case).astype(np.float32)).to("cuda:0")
    g32 = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")
    for log in (False, True):
        for trainable in (True, False):
            ref = _layer(case, log=log, trainable=trainable)
            lay = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                      f_min=case["f_min"], f_max=case["f_max"], hop_length=case["hop"], device="cuda:0", optimized=True,
                                      normalize_window=case["normalize_window"], log=log, out_dtype=torch.bfloat16).to("cuda:0")
            lay.requires_grad_(trainable)
            y32, y16 = ref(x), lay(x)
            assert y16.dtype == torch.bfloat16 and y16.shape == y32.shape
            assert torch.equal(y16.detach(), y32.detach().to(torch.bfloat16))        # same fp32 value, one rounding
            if trainable:
                # the gradient arrives in bf16 and is widened exactly: same d lambd as an fp32 gradient of the same values
                g16 = g32.to(torch.bfloat16)
                (y16 * g16).sum().backward()
                (y32 * g16.to(torch.float32)).sum().backward()
                assert float(lay.lambd.grad) == float(ref.lambd.grad)


# ---- MelPANNsNet end to end ----------------------------------------------------------------------
def test_panns_net_matches_reference_outputs():
    """Our front end + our Cnn6 (MIOpen) against the reference's MelPANNsNet run on CPU with identical closed-form weights."""
    import os
    from dmel_amd import panns, synth
    cfg = C.PANNS_CFG
    gold = np.load(os.path.join(os.path.dirname(C.__file__), "g9_panns.npz"))
    x = torch.from_numpy(synth.waveforms(cfg["B"], cfg["L"], seed=cfg["seed"])).to("cuda:0")
    for energy_normalize, key in ((True, "clipwise_log"), (False, "clipwise_lin")):
        net = panns.MelPANNsNet(cfg["n_classes"], torch.tensor(cfg["lambd"]), "cuda:0", cfg["n_mels"], cfg["sr"], cfg["L"],
                                hop_length=cfg["hop"], optimized=True, energy_normalize=energy_normalize).to("cuda:0")
        C.fill_state(net, seed=cfg["seed"])
        net.eval()
        with torch.no_grad():
            y, s = net(x)
        assert s.shape == (cfg["B"], 1, cfg["n_mels"], cfg["L"] // cfg["hop"] + 1)
        assert float(np.abs(y.cpu().numpy() - gold[key]).max()) <= 2e-4             # sigmoid scores in (0, 1)
        if energy_normalize:
            assert _log_err(s.cpu().numpy(), gold["s_log"]) <= TOL


def test_panns_net_training_step():
    from dmel_amd import nets, panns, synth
    cfg = C.PANNS_CFG
    net = panns.MelPANNsNet(cfg["n_classes"], torch.tensor(cfg["lambd"]), "cuda:0", cfg["n_mels"], cfg["sr"], cfg["L"],
                            hop_length=cfg["hop"], optimized=True, energy_normalize=True, augment=True).to("cuda:0")
    net.spectrogram_layer.requires_grad_(True)
    opt = nets.make_optimizer(net, lr_model=1e-4, lr_tf=1.0, name="adam")
    x = torch.from_numpy(synth.waveforms(4, cfg["L"], seed=5)).to("cuda:0")
    target = torch.tensor([1, 7, 3, 49], device="cuda:0")
    lam0 = float(net.spectrogram_layer.lambd.detach())
    net.train()
    for _ in range(2):
        opt.zero_grad()
        y, _ = net(x)
        loss = torch.nn.functional.cross_entropy(y, target)
        loss.backward()
        assert torch.isfinite(net.spectrogram_layer.lambd.grad).all() and float(net.spectrogram_layer.lambd.grad.abs()) > 0
        opt.step()
    assert float(net.spectrogram_layer.lambd.detach()) != lam0 and torch.isfinite(loss)


# ---- gradient w.r.t. the waveform (adjoint of models.py:38-53) ---------------------------------------------------
def _gx_err(got, exp):
    return float(np.abs(got.astype(np.float64) - exp).max() / (np.abs(exp).max() + 1e-30))


@pytest.mark.parametrize("name", ["g1_c1", "g5_n128", "g6_n256_ragged", "g6_tone_dc", "g6_n32"])
def test_xgrad_matches_reference_golden(name):
    """x.requires_grad through the nn.Module against torch autograd through the reference (g10_xgrad_*.npz, first two
    clips) and against the fp64 oracle (all clips)."""
    import os
    case = C.BY_NAME[name]
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g10_xgrad_{name}.npz"))
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to("cuda:0")
    for log, key in ((False, "gx_lin"), (True, "gx_log")):
        x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
        layer = _layer(case, log=log)
        y = layer(x)
        (y * g).sum().backward()
        gx = x.grad.cpu().numpy()
        assert gx.shape == x_np.shape and np.isfinite(gx).all()
        k = gold[key].shape[0]
        assert _gx_err(gx[:k], gold[key].astype(np.float64)) <= TOL
        ref = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y.detach().cpu().numpy() if log else None,
                           case["f_min"], case["f_max"], case["normalize_window"])
        assert _gx_err(gx, ref) <= TOL
        assert float(np.abs(gx.sum(1)).max()) <= 1e-4 * float(np.abs(gx).sum(1).max())      # DC removal: zero-sum per clip
        assert layer.lambd.grad is not None                                                # both gradients from one backward
        # deterministic
        x2 = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
        (_layer(case, log=log)(x2) * g).sum().backward()
        assert torch.equal(x.grad, x2.grad)


def test_xgrad_long_transform_and_finite_difference():
    case = dict(C.BY_NAME["g6_fminmax"], name="xgrad_8192", B=1, L=12000, lambd=700.0, hop=600, n_mels=40)
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
    layer = _layer(case, log=True)
    y = layer(x)
    (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
    ref = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y.detach().cpu().numpy(), case["f_min"], case["f_max"])
    assert _gx_err(x.grad.cpu().numpy(), ref) <= TOL
    # directional finite difference on the oracle-free path: loss(x + h d) - loss(x - h d) ~ 2 h <grad, d>
    d = torch.from_numpy(C.synth.waveforms(1, case["L"], seed=99, scale=1.0)).to("cuda:0")
    h = 1e-3
    with torch.no_grad():
        gdev = torch.from_numpy(g_np).to("cuda:0").double()
        lp = (layer(x.detach() + h * d).double() * gdev).sum()
        lm = (layer(x.detach() - h * d).double() * gdev).sum()
    fd = float(lp - lm) / (2 * h)
    an = float((x.grad.double() * d.double()).sum())
    assert abs(fd - an) <= 2e-2 * abs(an) + 1e-3


@pytest.mark.parametrize("hop,T", [(1000, 1), (300, 3), (100, 8), (47, 15), (41, 18)])
def test_filterbank_gradient_with_short_and_ragged_rows(hop, T):
    """dL/dfb where the time axis is shorter than one 16-byte piece (T < 4: element-wise requests) or ends inside a piece / a 16-step
    block (the piece is read from the row's last four entries and shifted into place), linear and log output, against the oracle"""
    from dmel_amd import capi
    case = dict(C.BY_NAME["g1_c1"], name=f"fb_T{T}", B=3, L=700, lambd=40.0, hop=hop, n_mels=24)
    assert case["L"] // hop + 1 == T
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    g = torch.from_numpy(g_np).to("cuda:0")
    plan = capi.Plan(case["L"], hop, case["n_mels"], case["sr"])
    n = capi.n_fft(case["lambd"])
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((case["B"], 1, case["n_mels"], T), device="cuda:0")
    plan.forward(x.data_ptr(), case["B"], case["lambd"], y.data_ptr(), None, True, 1e-10, st)
    y_np = y.cpu().numpy()
    for log in (False, True):
        gfb = torch.empty((n // 2 + 1, case["n_mels"]), dtype=torch.float32, device="cuda:0")
        plan.backward_fb(x.data_ptr(), case["B"], case["lambd"], g.data_ptr(), y.data_ptr(), gfb.data_ptr(), log, st)
        torch.cuda.synchronize()
        assert _gfb_err(gfb.cpu().numpy(), O.backward_fb(x_np, case["lambd"], hop, g_np, y_np if log else None)) <= TOL
        _assert_gfb_elementwise(f"fbgrad_ragged/T{T}/{'log' if log else 'lin'}", gfb.cpu().numpy(), case, x_np, g_np, y_np if log else None)


def test_optional_gradients_at_tiny_n_fft():
    """dL/dx and dL/dfb where the forward runs on the direct-DFT kernel (n_fft 16, 2, 1)."""
    from dmel_amd import capi
    for lam, n in ((2.0, 16), (0.34, 2), (0.2, 1)):
        case = dict(C.BY_NAME["g6_n32"], lambd=lam)
        assert capi.n_fft(lam) == n
        x_np = C.make_input(case).astype(np.float32)
        g_np = C.make_cotangent(case)
        x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
        layer = _layer(case, log=True)
        y = layer(x)
        (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
        y_np = y.detach().cpu().numpy()
        ref = O.backward_x(x_np, lam, case["hop"], case["sr"], g_np, y_np, case["f_min"], case["f_max"])
        assert _gx_err(x.grad.cpu().numpy(), ref) <= TOL
        plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"])
        gfb = torch.empty((n // 2 + 1, case["n_mels"]), dtype=torch.float32, device="cuda:0")
        g = torch.from_numpy(g_np).to("cuda:0")
        plan.backward_fb(x.detach().data_ptr(), case["B"], lam, g.data_ptr(), y.detach().data_ptr(), gfb.data_ptr(), True,
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _gfb_err(gfb.cpu().numpy(), O.backward_fb(x_np, lam, case["hop"], g_np, y_np)) <= TOL


@pytest.mark.parametrize("name", ["g6_normwin", "g6_neglambd", "g6_fminmax", "g6_n2048_short", "g5_n4096"])
def test_optional_gradients_on_edge_configurations(name):
    """dL/dx and dL/dfb against the oracle where the fixtures do not reach: normalised window, negative lambd, a band-limited
    bank, n_fft 2048 on clips shorter than two windows, n_fft 4096."""
    from dmel_amd import capi
    case = C.BY_NAME[name]
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    g = torch.from_numpy(g_np).to("cuda:0")
    x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
    layer = _layer(case, log=True)
    y = layer(x)
    (y * g).sum().backward()
    y_np = y.detach().cpu().numpy()
    ref = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y_np, case["f_min"], case["f_max"], case["normalize_window"])
    assert _gx_err(x.grad.cpu().numpy(), ref) <= TOL
    plan = capi.Plan(case["L"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"], case["normalize_window"])
    n = capi.n_fft(case["lambd"])
    gfb = torch.empty((n // 2 + 1, case["n_mels"]), dtype=torch.float32, device="cuda:0")
    plan.backward_fb(x.detach().data_ptr(), case["B"], case["lambd"], g.data_ptr(), y.detach().data_ptr(), gfb.data_ptr(), True,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _gfb_err(gfb.cpu().numpy(), O.backward_fb(x_np, case["lambd"], case["hop"], g_np, y_np, case["normalize_window"])) <= TOL
    _assert_gfb_elementwise(f"fbgrad_edge/{name}/log", gfb.cpu().numpy(), case, x_np, g_np, y_np)


ODD_SHAPES = [
    dict(C.BY_NAME["g1_c1"], name="hop_gt_nfft", B=3, L=9000, lambd=20.0, hop=300, n_mels=32),            # n_fft 128 < hop
    dict(C.BY_NAME["g1_c1"], name="single_frame", B=2, L=700, lambd=40.0, hop=1000, n_mels=16),             # T = 1
    dict(C.BY_NAME["g1_c1"], name="one_mel", B=2, L=4000, lambd=30.0, hop=100, n_mels=1),
    dict(C.BY_NAME["g1_c1"], name="many_mels", B=2, L=16000, lambd=170.0, hop=400, n_mels=200),             # two mel groups, n_fft 1024
    dict(C.BY_NAME["g1_c1"], name="many_mels_2048", B=1, L=16000, lambd=300.0, hop=800, n_mels=300),
    dict(C.BY_NAME["g1_c1"], name="short_clip", B=4, L=37, lambd=10.0, hop=5, n_mels=8),                    # clip shorter than n_fft 64
    # compact LDS layout (n_fft 2048 / 4096): negative lambd, normalised window, frame count not a multiple of the tile
    dict(C.BY_NAME["g1_c1"], name="compact_2048_neg_norm", B=3, L=12345, lambd=-260.0, hop=333, n_mels=80, normalize_window=True),
    dict(C.BY_NAME["g1_c1"], name="compact_4096_norm", B=2, L=30011, lambd=500.0, hop=1001, n_mels=64, normalize_window=True),
]


@pytest.mark.parametrize("case", ODD_SHAPES, ids=[c["name"] for c in ODD_SHAPES])
def test_unusual_shapes_match_oracle(case):
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
    for log in (False, True):
        layer = _layer(case, log=log)
        y = layer(x)
        assert y.shape == C.out_shape(case)
        x.grad = None
        (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
        o_ref, t_ref = O.forward(x_np, case["lambd"], case["hop"], case["n_mels"], case["sr"], case["f_min"], case["f_max"],
                                 case["normalize_window"], apply_log=log)
        o = y.detach().cpu().numpy()
        assert (_log_err(o, o_ref) if log else _rel_err(o, o_ref)) <= TOL
        exp_d = O.backward(g_np, t_ref)
        assert abs(float(layer.lambd.grad) - exp_d) <= _dlam_tol(exp_d, g_np, t_ref)
        ref_x = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, o if log else None, case["f_min"], case["f_max"],
                             case["normalize_window"])
        assert _gx_err(x.grad.cpu().numpy(), ref_x) <= TOL
        with torch.no_grad():
            yi = _layer(case, log=log, trainable=False)(x.detach())
        oi = yi.cpu().numpy()
        assert (_log_err(oi, o_ref) if log else _rel_err(oi, o_ref)) <= TOL


# ---- f1: logits of the caller nets against the reference's own (tests/golden/g11_nets.npz) --------------------------------
@pytest.mark.parametrize("key,cls,cname,en", [("conv_g1_log", "MelConvNet", "g1_c1", True), ("conv_g1_lin", "MelConvNet", "g1_c1", False),
                                              ("linear_g1_log", "MelLinearNet", "g1_c1", True),
                                              ("linear_g4_log", "MelLinearNet", "g4_esc_hop441", True),
                                              ("mlp_g1_log", "MelMlpNet", "g1_c1", True), ("mlp_g1_lin", "MelMlpNet", "g1_c1", False)])
def test_caller_nets_match_reference_logits(key, cls, cname, en, monkeypatch):
    """`(logits, s)` of our MelConvNet / MelLinearNet / MelMlpNet on the G1 / G4 inputs against the reference's own nets (models.py:58-136) with the same closed-form weights; F.dropout is the identity on both sides (models.py:75 keeps it always on)."""
    import os
    import torch.nn.functional as F
    from dmel_amd import nets
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "g11_nets.npz"))
    monkeypatch.setattr(F, "dropout", lambda x, *a, **k: x)
    case = C.BY_NAME[cname]
    net = getattr(nets, cls)(C.NET_CLASSES, torch.tensor(float(case["lambd"])), "cuda:0", case["n_mels"], case["sr"], case["L"],
                             hop_length=case["hop"], optimized=True, energy_normalize=en)
    C.fill_state(net, seed=C.NET_SEED)
    net = net.to("cuda:0")
    x = torch.from_numpy(C.make_input(case)).to("cuda:0")
    with torch.no_grad():
        logits, s = net(x)
    s_np = s.cpu().numpy()
    idx = C.sample_index(case)
    got_s = s_np if idx is None else s_np.reshape(-1)[idx]
    if en:
        assert _log_err(got_s, gold[key + "_s"]) <= TOL
    else:
        assert _rel_err(got_s, gold[key + "_s"]) <= TOL
    ref = gold[key + "_logits"]
    assert logits.shape == ref.shape
    # logits are sums over thousands of spectrogram bins: 1e-4 on s bounds them by about 1e-4 of their scale
    assert float(np.abs(logits.cpu().numpy() - ref).max()) <= 3e-4 * float(np.abs(ref).max()) + 1e-5


def test_config5_training_step_front_end_share():
    """BASELINE config 5 at full size: ESC-50-shaped clips (32 x 220500 @ 44.1 kHz, hop 441, 128 mels, lambd 256 -> n_fft 2048)
    through MelConvNet, CrossEntropy, Adam with the two learning-rate groups of main.py:36-53.  The front end's kernels are
    isolated with the library's HIP-event profiling: three launches per step (partial sums, fused forward, dot), a few
    per cent of the step."""
    from dmel_amd import nets, synth
    B, L, sr, lam, hop, M, ncls = 32, 220500, 44100, 256.0, 441, 128, 50
    torch.manual_seed(0)
    net = nets.MelConvNet(ncls, torch.tensor(lam), "cuda:0", M, sr, L, hop_length=hop, optimized=True, energy_normalize=True).to("cuda:0")
    opt = nets.make_optimizer(net, lr_model=1e-4, lr_tf=1.0)
    loss_fn = torch.nn.CrossEntropyLoss()
    x = torch.from_numpy(synth.waveforms(B, L, seed=0)).to("cuda:0")
    y = (torch.arange(B, device="cuda:0") * 7) % ncls
    losses = []

    def step():
        opt.zero_grad(set_to_none=True)
        logits, s = net(x)
        loss = loss_fn(logits, y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        return s

    for _ in range(3):
        s = step()
    torch.cuda.synchronize()
    assert s.shape == (B, 1, M, L // hop + 1) and net.spectrogram_layer.plan_info()["n_fft"] == 2048
    plan = net.spectrogram_layer._plan_for(torch.device("cuda:0"))
    plan.set_profiling(True)
    import time
    n = 4
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    dt_ms = 1e3 * (time.perf_counter() - t0) / n
    pr = plan.get_profile()
    plan.set_profiling(False)
    assert (pr["prep_launches"], pr["fwd_launches"], pr["bwd_launches"]) == (n, n, n)       # no guard launches: lambd is far from a boundary
    front_ms = (pr["prep_ms"] + pr["fwd_ms"] + pr["bwd_ms"]) / n
    assert front_ms < 0.5, front_ms                                  # ~0.14 ms measured (profiles/)
    assert front_ms / dt_ms < 0.15, (front_ms, dt_ms)                # ~3 % measured: the CNN dominates the step
    ls = [float(v) for v in losses]
    assert all(np.isfinite(ls)) and ls[-1] < ls[1]          # the first Adam step overshoots (3.95 -> 68), then the loss falls
    assert float(net.spectrogram_layer.lambd) != lam and net.spectrogram_layer.lambd_status()["error"] == 0


# ---- the optional gradients outside optimized=True (missing #2 and #3) -------------------------------------------------
@pytest.mark.parametrize("name", ["g7_mel_nonopt_256", "g7_mel_nonopt_1024n", "g7_mel_nonopt_601", "g7_mel_nonopt_8000"])
def test_xgrad_full_window_matches_reference_golden(name):
    """x.requires_grad through the optimized=False branch (window = the clip, n_fft = 2 L; time_frequency.py:41,51) against torch
    autograd through the reference (g10_xgrad_g7_*.npz).  601 and 8000 samples: n_fft 1202 / 16000 are not powers of two, both
    transforms of the adjoint are chirp-z round trips (16000: through 32768-point FFTs in global memory)."""
    import os
    case = C.BY_NAME[name]
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g10_xgrad_{name}.npz"))
    x_np = C.make_input(case).astype(np.float32)
    g = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")
    for log, key in ((False, "gx_lin"), (True, "gx_log")):
        x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
        layer = _layer(case, log=log)
        assert not layer.optimized
        (layer(x) * g).sum().backward()
        gx = x.grad.cpu().numpy()
        k = gold[key].shape[0]
        assert np.isfinite(gx).all() and _gx_err(gx[:k], gold[key].astype(np.float64)) <= TOL
        assert layer.lambd.grad is not None


def test_xgrad_long_power_of_two_transform():
    """dL/dx at n_fft 32768 (lambd 2800: a power of two beyond the LDS kernels): DIF / DIT in global memory, against the oracle"""
    case = dict(C.BY_NAME["g5_n32768"], B=1)
    x_np = C.make_input(case).astype(np.float32)
    g_np = C.make_cotangent(case)
    x = torch.from_numpy(x_np).to("cuda:0").requires_grad_(True)
    layer = _layer(case, log=True)
    y = layer(x)
    (y * torch.from_numpy(g_np).to("cuda:0")).sum().backward()
    ref = O.backward_x(x_np, case["lambd"], case["hop"], case["sr"], g_np, y.detach().cpu().numpy(), case["f_min"], case["f_max"],
                       case["normalize_window"])
    assert _gx_err(x.grad.cpu().numpy(), ref) <= TOL


@pytest.mark.parametrize("name", ["g7_mel_nonopt_256", "g7_mel_nonopt_601"])
def test_learnable_filterbank_full_window_matches_reference_golden(name):
    """learnable_fb with optimized=False -- n_fft = 2 L, a power of two (512) and not (1202: the spectrogram pass of the gradient
    takes the chirp-z path) -- against torch autograd through the reference with mel_fb made a leaf (g8_fbgrad_g7_*.npz)"""
    import os
    from dmel_amd import MelSpectrogramLayer
    case = C.BY_NAME[name]
    gold = np.load(os.path.join(os.path.dirname(C.__file__), f"g8_fbgrad_{name}.npz"))
    fwd = C.load(case)
    x = torch.from_numpy(C.make_input(case).astype(np.float32)).to("cuda:0")
    g = torch.from_numpy(C.make_cotangent(case)).to("cuda:0")
    for log, key in ((False, "gfb_lin"), (True, "gfb_log")):
        layer = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                                    f_min=case["f_min"], f_max=case["f_max"], hop_length=case["hop"], device="cuda:0", optimized=False,
                                    normalize_window=case["normalize_window"], log=log, learnable_fb=True).to("cuda:0")
        assert tuple(layer.mel_fb.shape) == gold[key].shape
        y = layer(x)
        (y * g).sum().backward()
        got = layer.mel_fb.grad.cpu().numpy()
        assert np.isfinite(got).all() and _gfb_err(got, gold[key].astype(np.float64)) <= TOL
        _assert_gfb_elementwise(f"fbgrad_full_window/{name}/{'log' if log else 'lin'}", got, case, x.cpu().numpy(), g.cpu().numpy(),
                                y.detach().cpu().numpy() if log else None, optimized=False)
        assert layer.lambd.grad is not None and np.isfinite(float(layer.lambd.grad))
        # the forward with the parameter as its filterbank equals the forward with the built-in table
        plain = _layer(case, log=log)
        with torch.no_grad():
            assert (_log_err if log else _rel_err)(y.detach().cpu().numpy(), plain(x).cpu().numpy()) <= TOL
    del fwd


def test_dspec_xgrad_matches_reference_golden():
    """x.requires_grad through SpectrogramLayer (models.py:171-200, optimized=False, L = 128 -> n_fft 256) against torch autograd
    through the reference (g7_dspec_xgrad.npz)"""
    import os
    from dmel_amd import SpectrogramLayer, synth
    gold = np.load(os.path.join(os.path.dirname(C.__file__), "g7_dspec_xgrad.npz"))
    x = torch.from_numpy(synth.waveforms(2, 128, seed=77, scale=1.0)).to("cuda:0").requires_grad_(True)
    lay = SpectrogramLayer(torch.tensor(6.38), optimized=False, hop_length=1).to("cuda:0")
    s = lay(x)
    g = torch.from_numpy(synth.cotangent(tuple(s.shape), seed=78)).to("cuda:0")
    (s * g).sum().backward()
    assert _gx_err(x.grad.cpu().numpy(), gold["gx"].astype(np.float64)) <= TOL
    assert lay.lambd.grad is not None
    # L = 100 -> n_fft 200, not a power of two: chirp-z in both directions (g7_dspec_xgrad_100.npz)
    gold100 = np.load(os.path.join(os.path.dirname(C.__file__), "g7_dspec_xgrad_100.npz"))
    x100 = torch.from_numpy(synth.waveforms(2, 100, seed=77, scale=1.0)).to("cuda:0").requires_grad_(True)
    s100 = lay(x100)
    g100 = torch.from_numpy(synth.cotangent(tuple(s100.shape), seed=78)).to("cuda:0")
    (s100 * g100).sum().backward()
    assert _gx_err(x100.grad.cpu().numpy(), gold100["gx"].astype(np.float64)) <= TOL


@pytest.mark.parametrize("sr,L,hop,lam,M", [(44100, 44100, 441, 256.0, 128), (16000, 40000, 512, 300.0, 128), (8000, 40000, 80, 300.0, 64)])
def test_quads_split_over_blocks_give_what_whole_quads_give(sr, L, hop, lam, M, monkeypatch):
    """Wave-local contraction at n_fft 2048 (one frame per wave): wide quads of mel bands are split over 2 or 4 blocks of the 4x4x1 MFMA and the
    partial sums merged across lanes (host schedule in build_tables; DMEL_WLC_NOSPLIT=1 keeps every quad whole).  Same products, another order
    of additions: equal to 1e-5 of each row's largest entry, outputs and tangent; and both within the parity bar of the fp64 oracle."""
    import torch
    from dmel_amd import capi, synth
    B = 3
    T = L // hop + 1
    x = torch.from_numpy(synth.waveforms(B, L, seed=5)).cuda()
    res = []
    for nosplit in (False, True):
        if nosplit:
            monkeypatch.setenv("DMEL_WLC_NOSPLIT", "1")
        else:
            monkeypatch.delenv("DMEL_WLC_NOSPLIT", raising=False)
        plan = capi.Plan(L, hop, M, sr, max_batch=B)          # the tables are built by the first forward of this plan
        out = torch.zeros((B, 1, M, T), device="cuda")
        tan = torch.zeros_like(out)
        plan.forward(x.data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), False, 1e-10, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert plan.info()["n_fft"] == 2048
        res.append((out.cpu().numpy().astype(np.float64), tan.cpu().numpy().astype(np.float64)))
        plan.close()
    for a, b in zip(res[0], res[1]):
        scale = np.abs(b).max(axis=(0, 1, 3), keepdims=True) + 1e-30
        assert (np.abs(a - b) / scale).max() <= 1e-5, float((np.abs(a - b) / scale).max())
    y_ref, _ = O.forward(x.cpu().numpy(), lam, hop, M, sr, want_tangent=False)
    assert _rel_err(res[0][0].reshape(-1), y_ref.reshape(-1)) <= TOL


@pytest.mark.parametrize("n_mels,lam", [(512, 128.0), (400, 100.0), (509, 300.0)])
def test_wave_local_contraction_with_empty_quads(n_mels, lam):
    """Many mel bands on few bins: bands, whole quads and (sorted by width, 16 to a phase) whole PHASES of the wave-local contraction are empty.
    Round 6 issues every load of the B ring (a group past the end of its phase re-reads the last one): with a phase of no groups at all the index
    must still stay inside the table.  Every element and the tangent against the oracle; zero-width bands are exact zeros (log: log(eps))."""
    from dmel_amd import capi
    from oracle import torch_restatement as R
    from tangent_cases import assert_tangent
    L, hop, sr, B = 6000, 128, 16000, 3
    # (the seeds: clips on which the oracle and the reference's fp32 arithmetic are within TOL / 4 of the fp64 evaluation in the element-wise
    # tangent metric -- bands of one bin have near-nulls that no fp32 transform resolves, tests/tangent_cases.py: "single bins"; seed 91, used
    # until the tangent was compared element by element, has one at each of the three sizes)
    case = dict(name=f"emptyq_m{n_mels}", B=B, L=L, sr=sr, lambd=lam, hop=hop, n_mels=n_mels, kind="noise", normalize_window=False, dtype="float32",
                seed={512: 391, 400: 391, 509: 591}[n_mels], f_min=0.0, f_max=None, optimized=True)
    x_np = C.make_input(case)
    x = torch.from_numpy(x_np).to("cuda:0")
    plan = capi.Plan(L, hop, n_mels, sr)
    out = torch.empty(C.out_shape(case), dtype=torch.float32, device="cuda:0")
    tan = torch.empty_like(out)
    for log in (False, True):
        plan.forward(x.data_ptr(), B, lam, out.data_ptr(), tan.data_ptr(), log, 1e-10, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        info = plan.info()
        o_ref, t_ref = O.forward(x_np, lam, hop, n_mels, sr, apply_log=log)
        o, t = out.cpu().numpy(), tan.cpu().numpy()
        assert np.isfinite(o).all() and np.isfinite(t).all()
        if log:
            assert _log_err(o, o_ref) <= TOL
        else:
            assert _rel_err(o, o_ref) <= TOL
            assert (o[o_ref == 0] == 0).all() and (o_ref == 0).any(), "the case must hold empty bands, and they must be exact zeros"
        assert float(np.abs(t - t_ref).max()) / (np.abs(t_ref).max() + 1e-30) <= TOL
        _, _, sc = R.tangent_fp64(x_np, lam, hop, n_mels, sr, log=log)
        assert_tangent(f"tangent/{case['name']}/{'log' if log else 'lin'}", t, t_ref, sc, shape=t.shape)
    assert info["n_fft"] in (1024, 2048)
