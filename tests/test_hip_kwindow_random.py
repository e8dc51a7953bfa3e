"""The K-window layers (MultiWindowMelSpectrogram, BandSplitMelSpectrogram) on the seeded random geometries of tests/kwindow_cases.py:
f_min / f_max, four sample rates, normalize_window, n_mels 1 ... 130, random band edges with one-row groups, rows shorter than a channel's
n_fft, rows past 32768 samples, both parities of T -- what the hand-picked geometries of the K-window files do not reach.  Channel k (rows
e_k ... e_{k+1} - 1 of the band layer) is MelSpectrogramLayer at lambd[k] bit for bit, lambd.grad[k] is that layer's to 1e-6 (the bar of
test_hip_multi_window.py), and output, lambd.grad and x.grad meet the fp64 oracle's bars with the project's measures (test_hip_parity.py,
test_hip_random_shapes.py, test_hip_lengths_xgrad.py): (a) forward(x), (b) out and tangent through the C ABI, (c) forward(x, lengths), (d) the
waveform gradients, (e) bf16.  tests/test_kwindow_cases_cpu.py holds the cases to what they claim, lists the groups whose oracle gradient is
cancellation-dominated (kwindow_cases.EXEMPT: the only ones whose plain d lambd bar may be skipped) and plants two faults in the comparisons
of this file.  Every maximum goes to the parity report under kwindow/."""
import numpy as np
import pytest
import torch

import cases as C
import kwindow_cases as KC
from oracle import dmel_oracle as O
from test_hip_klen import _step                                   # (out, lambd.grad) of one forward (+ backward to lambd when train)
from test_hip_klen_xgrad import _same, _zero_past
from test_hip_klen_xgrad import _step as _xstep                   # (out, lambd.grad, x.grad) with a waveform that requires grad
from test_hip_lengths_parity import _check_pad, _silent
from test_hip_parity import TOL, _gx_err, _log_err, _rel_err, assert_parity, parity_stats, record_parity
from test_hip_random_shapes import _assert_dlam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WHICH = ["multi", "band"]


# ---- the comparisons (tests/test_kwindow_cases_cpu.py plants its faults in these) ---------------------------------------------------------
def compare_output(tag, which, case, y, refs, log, lens=None):
    """the layer's output ``y`` (B, K or 1, M, T; numpy) against the oracle's per channel, ``refs[k]`` (B, 1, M, T) -- with ``lens``
    ``refs[k][b]`` (1, 1, M, Tc) at the clip's own length, on the clip's frames: _log_err / _rel_err per channel (and clip), and the plain
    relative error of every element (assert_parity without the floor; the log output through exp) over all of them, recorded under ``tag``"""
    hop = case["hop"]
    gots, exps = [], []
    for k, lam, c, lo, hi in KC.channel_rows(which, case):
        pairs = ([(y[:, c:c + 1, lo:hi], refs[k][:, :, lo:hi])] if lens is None else
                 [(y[b:b + 1, c:c + 1, lo:hi, :lb // hop + 1], refs[k][b][:, :, lo:hi]) for b, lb in enumerate(lens)])
        for got, exp in pairs:
            assert got.shape == exp.shape, (tag, k, got.shape, exp.shape)
            err = _log_err(got, exp) if log else _rel_err(got, exp)
            assert err <= TOL, (tag, k, lam, err)
            gots.append(got.reshape(-1))
            exps.append(exp.reshape(-1))
    got, exp = np.concatenate(gots).astype(np.float64), np.concatenate(exps).astype(np.float64)
    if log:
        return assert_parity(tag + "/exp_logmel", np.exp(got), np.exp(exp), allow_floor=False)
    return assert_parity(tag + "/mel", got, exp, allow_floor=False)


def compare_dlam(key, got_d, exp_d, g_flat, t_flat):
    """lambd.grad[k] against the oracle's: _assert_dlam.  Its plain 1e-4 bar is skipped for a cancellation-dominated sum: only where the CPU
    test listed the group (KC.EXEMPT).  A group with sum |g t| == 0 (an empty band, a clip of one sample) has a gradient of exactly 0.
    Returns ("zero", 0.0), ("exempt", relative error) or ("plain", relative error)."""
    mag = float(np.abs(g_flat.astype(np.float64) * t_flat.astype(np.float64)).sum())
    if mag == 0.0:
        assert got_d == 0.0, (key, got_d)
        return "zero", 0.0
    exempt = abs(exp_d) <= 1e-3 * mag
    if exempt:
        assert key in KC.EXEMPT, (key, "the cancellation exemption would be taken for a group tests/test_kwindow_cases_cpu.py did not list", exp_d, mag)
    _assert_dlam(got_d, exp_d, g_flat, t_flat, key)
    return ("exempt" if exempt else "plain"), (abs(got_d - exp_d) / abs(exp_d) if exp_d != 0.0 else float("inf"))


def dlam_reference(which, case, g_np, k, t_ref, lens=None):
    """(d_ref, g flat, t flat) of channel k: the oracle's backward of the channel's cotangent on its tangent ``t_ref`` (B, 1, M, T); with
    ``lens`` ``t_ref[b]`` (1, 1, M, Tc) and the sum over clips of the clip's own frames"""
    gk = KC.channel_cotangent(which, case, g_np, k)
    if lens is None:
        return O.backward(gk, t_ref), gk.reshape(-1), t_ref.reshape(-1)
    hop = case["hop"]
    gs = [np.ascontiguousarray(gk[b:b + 1, :, :, :lb // hop + 1]) for b, lb in enumerate(lens)]
    d_ref = sum(O.backward(gs[b], t_ref[b]) for b in range(len(lens)))
    return d_ref, np.concatenate([v.reshape(-1) for v in gs]), np.concatenate([t_ref[b].reshape(-1) for b in range(len(lens))])


def dlam_key(case, which, lens, log, k):
    return f"{case['name']}/{which}/{'lengths' if lens else 'fixed'}/{'log' if log else 'lin'}/k{k}"


def clip_gx_errors(got, ref, lens):
    """_gx_err per clip over the clip's own samples (test_hip_lengths_xgrad._oracle_errors: a clip whose reference is zero must be zero)"""
    errs = []
    for b, lb in enumerate(lens):
        diff, top = float(np.abs(got[b, :lb].astype(np.float64) - ref[b, :lb]).max()), float(np.abs(ref[b, :lb]).max())
        errs.append(diff / top if top > 0 else (0.0 if diff == 0 else float("inf")))
    return errs


# ---- layers and inputs ---------------------------------------------------------------------------------------------------------------------
def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _scalar_layer(case, lam, log, bf16=False, **kw):
    from dmel_amd import MelSpectrogramLayer
    return MelSpectrogramLayer(torch.tensor(float(lam), dtype=torch.float32), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                               f_min=case["f_min"], f_max=case["f_max"], hop_length=case["hop"], device=DEV, optimized=True,
                               normalize_window=case["normalize_window"], log=log, out_dtype=_dt(bf16), **kw).to(DEV)


def _kwindow_layer(which, case, log, bf16=False, sync=False, **kw):
    from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram
    args = (case["n_mels"], case["L"], case["sr"], case["f_min"], case["f_max"], case["hop"], case["normalize_window"])
    kw = dict(kw, log=log, out_dtype=_dt(bf16), lambd_sync=sync)
    if which == "multi":
        return MultiWindowMelSpectrogram(case["lams"], *args, **kw).to(DEV)
    lay = BandSplitMelSpectrogram(KC.band_lams(case), *args, band_edges=None if case["edges_default"] else case["edges"], **kw).to(DEV)
    assert list(lay.band_edges) == case["edges"]
    return lay


class _Refs:
    """one case's inputs on the device, its scalar layers' outputs and its oracle outputs: computed once, shared by the tests of the case
    (multi and band, linear and log) and left unchanged"""

    def __init__(self, case):
        self.case = case
        self.x_np = C.make_input(case).astype(np.float32)
        self.x = torch.from_numpy(self.x_np).to(DEV)
        self.g_np = {w: KC.cotangent(w, case) for w in WHICH}
        self.g = {w: torch.from_numpy(v).to(DEV) for w, v in self.g_np.items()}
        self.lens = list(case["lens"])
        self.lengths = torch.tensor(self.lens, dtype=torch.int32, device=DEV)
        self.x_nan = self.x.masked_fill(torch.arange(case["L"], device=DEV)[None, :] >= self.lengths[:, None], float("nan"))
        self._scalar, self._grad, self._oracle = {}, {}, {}

    def scalar(self, lam, log, bf16=False, lens=False):
        """(layer, its output in grad mode, its output under no_grad)"""
        key = (float(lam), log, bf16, lens)
        if key not in self._scalar:
            lay = _scalar_layer(self.case, lam, log, bf16)
            a = (self.x, self.lengths) if lens else (self.x,)
            with torch.no_grad():
                y_inf = lay(*a)
            self._scalar[key] = (lay, lay(*a).detach(), y_inf)
        return self._scalar[key]

    def scalar_grad(self, which, k, lam, log, bf16=False, lens=False):
        """the scalar layer's lambd.grad for channel k's cotangent"""
        key = (which, k, log, bf16, lens)
        if key not in self._grad:
            gk = torch.from_numpy(KC.channel_cotangent(which, self.case, self.g_np[which], k)).to(DEV)
            self._grad[key] = float(_step(self.scalar(lam, log, bf16, lens)[0], self.x, gk, self.lengths if lens else None)[1])
        return self._grad[key]

    def oracle(self, lam, log, lens=False):
        """(out, tangent) of the oracle at lam; with lens the list over clips of (out, tangent) at the clip's own length"""
        key = (float(lam), log, lens)
        if key not in self._oracle:
            if lens:
                self._oracle[key] = [KC.oracle_forward(self.case, self.x_np[b:b + 1, :lb], lam, log) for b, lb in enumerate(self.lens)]
            else:
                self._oracle[key] = KC.oracle_forward(self.case, self.x_np, lam, log)
        return self._oracle[key]


_CURRENT = {}


def _refs(case):
    if _CURRENT.get("name") != case["name"]:
        _CURRENT.clear()
        _CURRENT.update(name=case["name"], refs=_Refs(case))
    return _CURRENT["refs"]


def _family(which, lens, log, bf16, case):
    return f"kwindow/{which}/{'lengths' if lens else 'fixed'}/{'log' if log else 'lin'}/{'bf16' if bf16 else 'fp32'}/{case['name']}"


def _check_launches(lay, lams, sync):
    want = sorted(KC.launches(lams).items())
    got = lay._plan_for(torch.device(DEV)).last_multi_launch()
    if sync:
        assert got == want, (got, want)                      # exactly the distinct n_fft, each with its channels
    else:
        for n, mask in want:                                 # (the sync-free path may add guard launches next to a boundary)
            assert any(gn == n and gm & mask == mask for gn, gm in got), (n, mask, got)


def _check_forward(case, which, log, bf16=False, lens=False, oracle=True):
    """(a), (c), (e): the K-window layer against the scalar layers (bits; lambd.grad to 1e-6) and against the oracle"""
    r = _refs(case)
    parts = KC.channel_rows(which, case)
    lams = [p[1] for p in parts]
    B, M, hop = case["B"], case["n_mels"], case["hop"]
    T = case["L"] // hop + 1
    g = r.g[which].to(_dt(bf16))
    lengths = r.lengths if lens else None
    tc = [lb // hop + 1 for lb in r.lens]
    fam = _family(which, lens, log, bf16, case)
    kw = dict(per_clip_lengths=True) if lens else {}
    worst_scalar = 0.0
    for sync in [False] + ([True] if case["index"] % 3 == 0 else []):
        lay = _kwindow_layer(which, case, log, bf16, sync, **kw)
        y, d = _step(lay, r.x, g, lengths)
        _check_launches(lay, lams, sync)
        y_inf, _ = _step(lay, r.x, g, lengths, train=False)
        _check_launches(lay, lams, sync)
        assert y.shape == (B, len(lams) if which == "multi" else 1, M, T) and y.dtype == _dt(bf16) and y_inf.dtype == _dt(bf16)
        for k, lam, c, lo, hi in parts:
            sl, yk, yk_inf = r.scalar(lam, log, bf16, lens)
            assert _same(y[:, c:c + 1, lo:hi], yk[:, :, lo:hi]), ("train", fam, sync, k, lam)
            assert _same(y_inf[:, c:c + 1, lo:hi], yk_inf[:, :, lo:hi]), ("no_grad", fam, sync, k, lam)
            dk = r.scalar_grad(which, k, lam, log, bf16, lens)
            assert abs(float(d[k]) - dk) <= 1e-6 * abs(dk) + 1e-12, (fam, sync, k, lam, float(d[k]), dk)
            if dk != 0.0:
                worst_scalar = max(worst_scalar, abs(float(d[k]) - dk) / abs(dk))
            if lens and not sync:
                for out, train in ((y, True), (y_inf, False)):
                    _check_pad(out[:, c:c + 1, lo:hi], tc, _silent(sl, train))
        if lens and not sync:                                # samples past a clip are never read: NaN there, identical bits
            y2, d2 = _step(lay, r.x_nan, g, lengths)
            y2_inf, _ = _step(lay, r.x_nan, g, lengths, train=False)
            assert _same(y, y2) and _same(d, d2) and _same(y_inf, y2_inf), ("NaN past the clips", fam)
        if sync:
            continue
        if not oracle:                                       # (e): the bits are the scalar layer's; its distance from the oracle is recorded
            got = np.concatenate([y[:, c:c + 1, lo:hi].float().cpu().numpy().reshape(-1) for k, lam, c, lo, hi in parts])
            exp = np.concatenate([r.oracle(lam, log)[0][:, :, lo:hi].reshape(-1) for k, lam, c, lo, hi in parts])
            record_parity(fam + "/logmel_vs_oracle", parity_stats(got, exp))
            continue
        refs = {k: r.oracle(lam, log, lens) for k, lam, *_ in parts}
        outs = {k: ([o for o, _ in v] if lens else v[0]) for k, v in refs.items()}
        tans = {k: ([t for _, t in v] if lens else v[1]) for k, v in refs.items()}
        st = compare_output(fam + "/train", which, case, y.cpu().numpy(), outs, log, r.lens if lens else None)
        compare_output(fam + "/no_grad", which, case, y_inf.cpu().numpy(), outs, log, r.lens if lens else None)
        worst, zero, exempt = 0.0, 0, 0
        for k, lam, c, lo, hi in parts:
            d_ref, gf, tf = dlam_reference(which, case, r.g_np[which], k, tans[k], r.lens if lens else None)
            key = dlam_key(case, which, lens, log, k)
            kind, rel = compare_dlam(key, float(d[k]), d_ref, gf, tf)
            zero += kind == "zero"
            exempt += kind == "exempt"
            if kind == "plain":
                worst = max(worst, rel)
        record_parity(fam + "/dlam", {"n": len(parts), "plain_max_rel": worst, "zero_groups": int(zero), "exempt_groups": int(exempt)})
        print(f"{fam}: out {st['plain_max_rel']:.3e} dlam {worst:.3e} zero {zero} exempt {exempt}")
    record_parity(fam + "/dlam_vs_scalar", {"n": len(parts), "max_rel": worst_scalar})


def _ids(items):
    return ["-".join([c["name"]] + [str(v) for v in rest]) for c, *rest in items]


# ---- a. forward and lambd.grad, fixed length -------------------------------------------------------------------------------------------------
FWD = [(c, w, log) for c in KC.FORWARD_CASES for w in WHICH for log in ("lin", "log")]


@pytest.mark.parametrize("case,which,log", FWD, ids=_ids(FWD))
def test_fixed_length_forward_and_lambd_grad(case, which, log):
    _check_forward(case, which, log == "log")


# ---- b. out and tangent through the C ABI ----------------------------------------------------------------------------------------------------
CAPI = [(c, log) for c in KC.FORWARD_CASES[::2] for log in ("lin", "log")]


@pytest.mark.parametrize("case,log", CAPI, ids=_ids(CAPI))
def test_out_and_tangent_through_the_c_abi(case, log):
    """dmel_forward_multi(_dev) and dmel_forward_band(_dev) into images pre-filled with 7.0, against dmel_forward per channel: out AND
    tangent bit for bit, and no cell of an image left unwritten (every row belongs to a group and that group's launch wrote it)"""
    from dmel_amd import capi
    log = log == "log"
    r = _refs(case)
    B, L, M, hop = case["B"], case["L"], case["n_mels"], case["hop"]
    T = L // hop + 1
    st = torch.cuda.current_stream().cuda_stream

    def plan():
        return capi.Plan(L, hop, M, case["sr"], case["f_min"], case["f_max"], case["normalize_window"])

    ref_plan, refs = plan(), {}
    for lam in case["lams"]:
        o_k, t_k = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
        ref_plan.forward(r.x.data_ptr(), B, lam, o_k.data_ptr(), t_k.data_ptr(), log, 1e-10, st)
        refs[lam] = (o_k, t_k)
    for which in WHICH:
        parts = KC.channel_rows(which, case)
        lams = [p[1] for p in parts]
        K = len(lams)
        lam_d = torch.tensor(lams, dtype=torch.float32, device=DEV)
        for dev in (False, True):
            p = plan()
            out = torch.full((B, K if which == "multi" else 1, M, T), 7.0, device=DEV)
            tan = torch.full_like(out, 7.0)
            scratch = torch.zeros((max(16, p.scratch_bytes_multi(B, K)),), dtype=torch.uint8, device=DEV)
            a = (out.data_ptr(), tan.data_ptr(), log, 1e-10, st, scratch.data_ptr())
            if which == "multi":
                p.forward_multi_dev(r.x.data_ptr(), B, lam_d.data_ptr(), K, *a) if dev else p.forward_multi(r.x.data_ptr(), B, lams, *a)
            else:
                p.forward_band_dev(r.x.data_ptr(), B, lam_d.data_ptr(), case["edges"], *a) if dev else p.forward_band(r.x.data_ptr(), B, lams, case["edges"], *a)
            torch.cuda.synchronize()
            for k, lam, c, lo, hi in parts:
                assert _same(out[:, c:c + 1, lo:hi], refs[lam][0][:, :, lo:hi]), ("out", case["name"], which, dev, k, lam)
                assert _same(tan[:, c:c + 1, lo:hi], refs[lam][1][:, :, lo:hi]), ("tangent", case["name"], which, dev, k, lam)
            assert not (out == 7.0).any() and not (tan == 7.0).any(), (case["name"], which, dev)


# ---- c. per-clip lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which,log", FWD, ids=_ids(FWD))
def test_per_clip_lengths_forward_and_lambd_grad(case, which, log):
    _check_forward(case, which, log == "log", lens=True)


# ---- d. waveform gradients ---------------------------------------------------------------------------------------------------------------------
XGRAD = [(c, w, v, log) for c in KC.GRAD_CASES for w in WHICH for v in ("fixed", "lengths") for log in ("lin", "log")]


@pytest.mark.parametrize("case,which,variant,log", XGRAD, ids=_ids(XGRAD))
def test_waveform_gradient(case, which, variant, log):
    """x.grad is 0 + gx_0 + ... + gx_{K-1} of the scalar layers bit for bit; every gx_k and the sum meet the oracle's bar (per clip with
    lengths); +0.0 past a clip; output and lambd.grad are the flag-off layer's; a second run gives the same bits"""
    log, lens = log == "log", variant == "lengths"
    r = _refs(case)
    parts = KC.channel_rows(which, case)
    g = r.g[which]
    lengths = r.lengths if lens else None
    on = dict(per_clip_lengths=True, lengths_waveform_grad=True) if lens else dict(waveform_grad=True)
    off = dict(per_clip_lengths=True) if lens else {}
    fam = _family(which, lens, log, False, case)
    lay = _kwindow_layer(which, case, log, **on)
    y, d, gx = _xstep(lay, r.x, g, lengths)
    y_np = y.cpu().numpy()
    ref, terms = KC.composed_xgrad(which, case, r.x_np, r.g_np[which], y_np if log else None, r.lens if lens else None)
    acc, worst_scalar = torch.zeros_like(r.x), 0.0
    for k, lam, c, lo, hi in parts:
        gk = torch.from_numpy(KC.channel_cotangent(which, case, r.g_np[which], k)).to(DEV)
        yk, dk, gxk = _xstep(_scalar_layer(case, lam, log, **(dict(lengths_waveform_grad=True) if lens else {})), r.x, gk, lengths)
        assert _same(y[:, c:c + 1, lo:hi], yk[:, :, lo:hi]), ("out", fam, k, lam)        # (so terms[k], formed with y, is the scalar layer's reference)
        assert abs(float(d[k]) - float(dk)) <= 1e-6 * abs(float(dk)) + 1e-12, (fam, k, float(d[k]), float(dk))
        err = max(clip_gx_errors(gxk.cpu().numpy(), terms[k], r.lens)) if lens else _gx_err(gxk.cpu().numpy(), terms[k])
        assert err <= TOL, ("scalar x.grad against the oracle", fam, k, lam, err)
        worst_scalar = max(worst_scalar, err)
        acc = acc + gxk
    assert torch.isfinite(gx).all() and _same(gx, acc), ("x.grad is not the scalar layers' sum", fam, float((gx - acc).abs().max()))
    err = max(clip_gx_errors(gx.cpu().numpy(), ref, r.lens)) if lens else _gx_err(gx.cpu().numpy(), ref)
    record_parity(fam + "/xgrad", {"n": int(gx.numel()), "max_rel": err, "scalar_max_rel": worst_scalar})
    print(f"{fam}: xgrad {err:.3e} scalar layers {worst_scalar:.3e}")
    assert err <= TOL, (fam, err)
    if lens:
        assert _zero_past(gx, r.lens), fam
    y0, d0 = _step(_kwindow_layer(which, case, log, **off), r.x, g, lengths)                 # without the flag
    assert _same(y, y0) and _same(d, d0), ("the flag changed the output or lambd.grad", fam)
    y2, d2, gx2 = _xstep(lay, r.x, g, lengths)
    assert _same(y, y2) and _same(d, d2) and _same(gx, gx2), ("second run", fam)


# ---- e. bf16 output --------------------------------------------------------------------------------------------------------------------------
BF16 = [(c, w) for c in KC.BF16_CASES for w in WHICH]


@pytest.mark.parametrize("case,which", BF16, ids=_ids(BF16))
def test_bf16_output(case, which):
    _check_forward(case, which, True, bf16=True, oracle=False)
