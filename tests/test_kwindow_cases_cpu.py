"""What can be said about the K-window sweep (tests/kwindow_cases.py, tests/test_hip_kwindow_random.py) without a GPU: the generator is
deterministic and its cases cover what they claim; the oracle sees every option a case sets and tells neighbouring band groups apart, by
more than ten times the bar the GPU test asserts; the cancellation exemption of _assert_dlam is rare in the oracle's own gradients, and the
groups that take it are exactly the ones listed (kwindow_cases.EXEMPT); the composed reference of the K-window x.grad is torch autograd's in
fp64; and two planted faults fail the GPU test's own comparisons."""
import numpy as np
import pytest
import torch

import cases as C
import kwindow_cases as KC
import test_hip_parity as P
from oracle import dmel_oracle as O
from oracle import torch_restatement as R
from test_hip_kwindow_random import WHICH, compare_output, dlam_key, dlam_reference
from test_hip_parity import TOL

ALL = KC.FORWARD_CASES + KC.GRAD_CASES
_X, _FWD = {}, {}


def _x(case):
    if case["name"] not in _X:
        _X[case["name"]] = C.make_input(case).astype(np.float32)
    return _X[case["name"]]


def _fwd(case, lam, log, lens=False, **drop):
    """the oracle's (out, tangent) at lam, computed once; with lens the list over clips at the clip's own length"""
    key = (case["name"], float(lam), log, lens, tuple(sorted(drop.items())))
    if key not in _FWD:
        x = _x(case)
        _FWD[key] = ([KC.oracle_forward(case, x[b:b + 1, :lb], lam, log, **drop) for b, lb in enumerate(case["lens"])] if lens else
                     KC.oracle_forward(case, x, lam, log, **drop))
    return _FWD[key]


def _image(which, case, log, swap=None, drop_k=None, **drop):
    """the oracle's K-window output: channels stacked (multi) or rows selected (band).  ``swap`` (k, lam): channel k computed at lam instead;
    ``drop_k`` and ``drop``: settings overridden for that channel alone"""
    B, _, M, T = C.out_shape(case)
    parts = KC.channel_rows(which, case)
    y = np.empty((B, len(parts) if which == "multi" else 1, M, T), np.float32)
    for k, lam, c, lo, hi in parts:
        if swap is not None and swap[0] == k:
            lam = swap[1]
        o = _fwd(case, lam, log, **(drop if k == drop_k else {}))[0]
        y[:, c:c + 1, lo:hi] = o[:, :, lo:hi]
    return y


def _row_rel(got, exp):
    """the GPU test's measure of the output (the plain relative error of every element, test_hip_parity.parity_stats) per mel row: (M,)"""
    g, e = got.astype(np.float64), exp.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(e != 0, np.abs(g - e) / np.abs(e), np.where(g != e, np.inf, 0.0))
    return rel.max(axis=(0, 1, 3))


def _lin(o, log):
    return np.exp(o.astype(np.float64)) if log else o


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    assert KC.kwindow_cases(40, KC.FORWARD_SEED) == KC.FORWARD_CASES
    assert KC.kwindow_cases(16, KC.GRAD_SEED, cost_cap=1.5e6, prefix="kg") == KC.GRAD_CASES
    assert KC.kwindow_cases(16, KC.GRAD_SEED + 1, cost_cap=1.5e6, prefix="kg") != KC.GRAD_CASES
    assert len(KC.FORWARD_CASES) == 40 and len(KC.GRAD_CASES) == 16 and KC.BF16_CASES == KC.FORWARD_CASES[::5]
    assert len({c["name"] for c in ALL}) == len(ALL)


def test_every_case_is_what_the_generator_promises():
    for cases, cap in ((KC.FORWARD_CASES, 6e6), (KC.GRAD_CASES, 1.5e6)):
        long_rows = [c for c in cases if c["L"] > 32768]
        assert len(long_rows) == 2, [c["name"] for c in long_rows]
        for c in cases:
            lams, L, hop, B, M = c["lams"], c["L"], c["hop"], c["B"], c["n_mels"]
            ns = [KC.n_fft(v) for v in lams]
            T = L // hop + 1
            assert ns == [O.n_fft(v) for v in lams] and all(32 <= n <= 16384 for n in ns), c["name"]
            assert 1 <= len(lams) <= 8 and 1 <= B <= 4 and T <= 300 and B * len(lams) * T * max(ns) <= cap, c["name"]
            assert C.out_shape(c) == (B, 1, M, T) and C.make_input(c).shape == (B, L) and C.make_cotangent(c).shape == (B, 1, M, T)
            assert KC.multi_cotangent(c).shape == (B, len(lams), M, T)
            if L > 32768:
                assert 32769 <= L <= 40000 and hop >= 400 and B <= 2, c["name"]
            else:
                assert max(8, min(ns) // 4) <= L <= 30000, c["name"]
            e = c["edges"]
            Kb = len(e) - 1
            assert Kb == min(len(lams), M) and e[0] == 0 and e[-1] == M and all(b > a for a, b in zip(e, e[1:])), c["name"]
            if c["edges_default"]:
                assert e == [(k * M) // Kb for k in range(Kb + 1)]
            elif M > Kb:
                assert any(b - a == 1 for a, b in zip(e, e[1:])), c["name"]
            lens = c["lens"]
            assert len(lens) == B and all(1 <= v <= L for v in lens), c["name"]
            held = set().union(*(KC.length_classes(c, v) for v in lens))
            if L > 32768:
                assert {"above", "below", "edge"} <= held and ("full" in held or "last_tile" in held), (c["name"], lens)
            else:
                fits = {"edge", "full"} | ({"last_tile"} if L >= 2 else set())
                assert len(held & fits) >= min(B, len(fits)), (c["name"], lens, held)


def test_the_two_lists_cover_what_the_sweep_claims():
    lams = [v for c in ALL for v in c["lams"]]
    assert {KC.n_fft(v) for v in lams} == set(KC.NFFTS)
    neg = sum(v < 0 for v in lams) / len(lams)
    assert 0.1 <= neg <= 0.3, neg
    assert {c["sr"] for c in ALL} == set(KC.SRS) and {c["n_mels"] for c in ALL} == set(KC.N_MELS)
    assert {c["f_min"] for c in ALL} == set(KC.F_MINS) and {c["B"] for c in ALL} == {1, 2, 3, 4}
    assert any(c["f_max"] is None for c in ALL) and any(c["f_max"] is not None and 0.3 * c["sr"] <= c["f_max"] <= 0.5 * c["sr"] for c in ALL)
    assert all(c["f_max"] is None or 0.3 * c["sr"] <= c["f_max"] <= 0.5 * c["sr"] for c in ALL)
    assert {c["normalize_window"] for c in ALL} == {False, True} and {c["edges_default"] for c in ALL} == {False, True}
    assert {len(c["lams"]) for c in ALL} >= {1, 8}
    assert sum(KC.shared_n_fft(c["lams"]) for c in ALL) >= 8
    assert sum(bool(KC.straddles(c["lams"])) for c in ALL) >= 4
    assert sum(c["n_mels"] > 1 and any(b - a == 1 for a, b in zip(c["edges"], c["edges"][1:])) for c in ALL) >= 8
    assert {(c["L"] // c["hop"] + 1) % 2 for c in ALL} == {0, 1}
    assert any(c["L"] < KC.n_fft(v) for c in ALL for v in c["lams"])
    held = set().union(*(KC.length_classes(c, v) for c in ALL for v in c["lens"]))
    assert held == set(KC.LENGTH_CLASSES), held
    for c in ALL:                                              # every single edge value occurs somewhere
        held |= {("edge", v - c["hop"]) for v in c["lens"] if v in (c["hop"] - 1, c["hop"], c["hop"] + 1)} | {("edge", "one") for v in c["lens"] if v == 1}
    assert {("edge", -1), ("edge", 0), ("edge", 1), ("edge", "one")} <= held, held


# ---- the cases can see the options -----------------------------------------------------------------------------------------------------------
def _seen(case, log, **drop):
    """(multi, band, k): the largest difference, in the GPU test's measure, the oracle shows between the proper output and the one with the
    setting dropped -- over all rows of all channels, and over every band group's own rows (the group k shows it)"""
    multi, band, at = 0.0, 0.0, None
    e = case["edges"]
    for k, lam in enumerate(case["lams"]):
        rows = _row_rel(_lin(_fwd(case, lam, log, **drop)[0], log), _lin(_fwd(case, lam, log)[0], log))
        multi = max(multi, float(rows.max()))
        if k < len(e) - 1 and float(rows[e[k]:e[k + 1]].max()) > band:
            band, at = float(rows[e[k]:e[k + 1]].max()), k
    return multi, band, at


def test_the_oracle_sees_every_option_a_case_sets():
    smallest = {}
    for c in ALL:
        drops = ([("f_max", dict(f_max=None))] if c["f_max"] is not None else []) + ([("f_min", dict(f_min=0.0))] if c["f_min"] > 0 else []) + \
                ([("normalize_window", dict(normalize_window=False))] if c["normalize_window"] else [])
        for name, drop in drops:
            for log in (False, True):
                multi, band, _ = _seen(c, log, **drop)
                assert multi > 10 * TOL and band > 10 * TOL, (c["name"], name, log, multi, band)
                smallest[name] = min(smallest.get(name, np.inf), multi, band)
    assert set(smallest) == {"f_max", "f_min", "normalize_window"}
    print("smallest 'option dropped' difference (plain relative, ten times the bar is 1e-3):", {k: f"{v:.3e}" for k, v in smallest.items()})


def _neighbour_differences(case, log):
    """[(k, difference on group k's rows between the oracle at lambd[k + 1] and at lambd[k])] for the band groups that do not share a value"""
    e, lams = case["edges"], KC.band_lams(case)
    out = []
    for k in range(len(lams) - 1):
        if np.float32(lams[k]) != np.float32(lams[k + 1]):
            rows = _row_rel(_lin(_fwd(case, lams[k + 1], log)[0], log), _lin(_fwd(case, lams[k], log)[0], log))
            out.append((k, float(rows[e[k]:e[k + 1]].max())))
    return out


def test_the_oracle_tells_neighbouring_band_groups_apart():
    same = sorted((c["name"], k) for c in ALL for k in range(len(KC.band_lams(c)) - 1)
                  if np.float32(KC.band_lams(c)[k]) == np.float32(KC.band_lams(c)[k + 1]))
    assert same == KC.SAME_LAMBD, same
    smallest, n = np.inf, 0
    for c in ALL:
        for log in (False, True):
            for k, diff in _neighbour_differences(c, log):
                assert diff > 10 * TOL, (c["name"], log, k, diff)
                smallest, n = min(smallest, diff), n + 1
    assert n >= 100, n
    print(f"smallest \"neighbour's lambd\" difference over {n} (case, log, group): {smallest:.3e} (groups sharing a lambd value: {same})")


# ---- the cancellation exemption stays rare ----------------------------------------------------------------------------------------------------
def _dlam_groups(lens):
    """over all (case, layer, log, channel or group): (keys that take the exemption, keys with sum |g t| == 0, how many there are)"""
    exempt, zero, n = [], [], 0
    for c in ALL:
        for which in WHICH:
            g = KC.cotangent(which, c)
            for log in (False, True):
                for k, lam, *_ in KC.channel_rows(which, c):
                    ref = _fwd(c, lam, log, lens)
                    t_ref = [t for _, t in ref] if lens else ref[1]
                    d_ref, gf, tf = dlam_reference(which, c, g, k, t_ref, c["lens"] if lens else None)
                    mag = float(np.abs(gf.astype(np.float64) * tf.astype(np.float64)).sum())
                    n += 1
                    if mag == 0.0:
                        assert d_ref == 0.0
                        zero.append(dlam_key(c, which, lens, log, k))
                    elif abs(d_ref) <= 1e-3 * mag:
                        exempt.append(dlam_key(c, which, lens, log, k))
    return exempt, zero, n


@pytest.mark.parametrize("lens", [False, True], ids=["fixed", "lengths"])
def test_the_cancellation_exemption_stays_rare(lens):
    exempt, zero, n = _dlam_groups(lens)
    share = len(exempt) / n
    print(f"{'per-clip lengths' if lens else 'fixed length'}: {len(exempt)} of {n} groups take the cancellation exemption ({100 * share:.1f} %), "
          f"{len(zero)} have sum |g t| == 0")
    assert share <= 0.10, (share, exempt)
    tag = "/lengths/" if lens else "/fixed/"
    assert sorted(exempt) == sorted(k for k in KC.EXEMPT if tag in k), sorted(exempt)      # the GPU test skips the plain bar for these alone


# ---- the composed x-gradient reference ----------------------------------------------------------------------------------------------------------
_BASE = dict(C.BY_NAME["g1_c1"], sr=8000, f_min=0.0, f_max=None, normalize_window=False, edges_default=False)
TINY = [dict(_BASE, name="tiny_32_64", B=2, L=200, hop=20, n_mels=7, lams=[5.0, 9.0], edges=[0, 1, 7], lens=[200, 57], seed=9001),
        dict(_BASE, name="tiny_32_32_64_banded", B=2, L=150, hop=15, n_mels=16, lams=[4.0, -4.5, 10.0], edges=[0, 5, 6, 16], lens=[149, 15], seed=9002,
             f_min=50.0, f_max=3000.0, normalize_window=True),
        dict(_BASE, name="tiny_64_short_rows", B=3, L=40, hop=7, n_mels=3, lams=[8.0, 3.5], edges=[0, 2, 3], lens=[40, 1, 7], seed=9003)]


def _autograd_xgrad(which, case, x_np, g_np, log, lens):
    """torch autograd in fp64 through oracle/torch_restatement.forward: channels stacked (multi) or rows selected (band), clip by clip on
    x[b, :Lc] and the first Lc // hop + 1 frames with lens"""
    x = torch.tensor(x_np, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(g_np, dtype=torch.float64)
    hop, M, sr = case["hop"], case["n_mels"], case["sr"]
    total = 0.0
    for k, lam, c, lo, hi in KC.channel_rows(which, case):
        n = KC.n_fft(lam)
        fb = torch.tensor(O.mel_fbanks(n // 2 + 1, case["f_min"], float(sr // 2) if case["f_max"] is None else case["f_max"], M, sr)).double()
        lam_t = torch.tensor(float(np.float32(lam)), dtype=torch.float64)
        clips = [(slice(None), case["L"])] if lens is None else [(slice(b, b + 1), lb) for b, lb in enumerate(lens)]
        for rows, lb in clips:
            out = R.forward(x[rows, :lb], lam_t, hop, M, sr, case["f_min"], case["f_max"], case["normalize_window"], log=log, fb=fb)
            total = total + (out[:, :, lo:hi] * g[rows, c:c + 1, lo:hi, :lb // hop + 1]).sum()
    total.backward()
    return x.grad.numpy()


@pytest.mark.parametrize("case", TINY, ids=[c["name"] for c in TINY])
def test_the_composed_x_gradient_reference_is_autograds(case):
    assert all(KC.n_fft(v) in (32, 64) for v in case["lams"]) and case["L"] // case["hop"] + 1 <= 12
    x_np = C.make_input(case).astype(np.float32)
    for which in WHICH:
        g_np = KC.cotangent(which, case)
        for log in (False, True):
            for lens in (None, case["lens"]):
                y = None
                if log:                                    # the saved log output: the oracle's image, pad frames never read
                    y = _image(which, case, True)
                    if lens is not None:
                        for k, lam, c, lo, hi in KC.channel_rows(which, case):
                            for b, lb in enumerate(lens):
                                tb = lb // case["hop"] + 1
                                y[b, c, lo:hi, :tb] = KC.oracle_forward(case, x_np[b:b + 1, :lb], lam, True)[0][0, 0, lo:hi]
                                y[b, c, lo:hi, tb:] = np.nan
                ref, _ = KC.composed_xgrad(which, case, x_np, g_np, y, lens)
                exp = _autograd_xgrad(which, case, x_np, g_np, log, lens)
                err = float(np.abs(ref - exp).max() / np.abs(exp).max())
                print(f"{case['name']} {which} log={log} lengths={lens}: composed reference against fp64 autograd {err:.3e}")
                assert np.isfinite(ref).all() and err <= TOL / 4, (which, log, lens, err)


# ---- the sweep bites ---------------------------------------------------------------------------------------------------------------------------
def _fails(which, case, y, log):
    """whether the GPU test's comparison of the output rejects ``y`` (its entries of the parity report are taken out again)"""
    refs = {k: _fwd(case, lam, log)[0] for k, lam, *_ in KC.channel_rows(which, case)}
    before = set(P._REPORT)
    try:
        compare_output("kwindow/planted", which, case, y, refs, log)
        return False
    except AssertionError:
        return True
    finally:
        for name in set(P._REPORT) - before:
            del P._REPORT[name]


def test_planted_faults_fail_the_comparisons_of_the_gpu_test():
    n_rows = n_fmax = 0
    for c in ALL:
        for log in (False, True):
            assert not _fails("band", c, _image("band", c, log), log) and not _fails("multi", c, _image("multi", c, log), log)
            # one group's rows taken from its neighbour's lambd
            lams = KC.band_lams(c)
            for k, diff in _neighbour_differences(c, log):
                assert _fails("band", c, _image("band", c, log, swap=(k, lams[k + 1])), log), (c["name"], log, k, diff)
                n_rows += 1
            # one channel computed with f_max dropped (the channel whose own band rows show it most)
            if c["f_max"] is not None:
                k = _seen(c, log, f_max=None)[2]
                for which in WHICH:
                    assert _fails(which, c, _image(which, c, log, drop_k=k, f_max=None), log), (c["name"], which, log, k)
                    n_fmax += 1
    assert n_rows >= 100 and n_fmax >= 20, (n_rows, n_fmax)
