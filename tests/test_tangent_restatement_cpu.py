"""The oracle's tangent d out / d lambd, element by element, against an independent fp64 evaluation (oracle/torch_restatement.py:
tangent_fp64 -- the window's derivative from autograd's jacobian, a second stft with it); until here it was pinned only through dot
products (dlam_lin / dlam_log of the fixtures, torch_restatement.step).  Same cases, inputs and metric as tests/test_hip_tangent.py
(tests/tangent_cases.py), and the condition that makes that test's bar fair: on every shared case the oracle AND the reference's own
fp32 arithmetic stay within TOL / 4 of the fp64 evaluation.  No GPU."""
import numpy as np
import pytest

import tangent_cases as TC
from tangent_cases import REF_BAR, TOL, assert_tangent, tangent_stats

MODES = (False, True)


def _modes(case):
    return (False,) if case["spectrogram"] else MODES


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_oracle_and_fp32_reference_sit_inside_the_bar(case):
    """both references within TOL / 4 of tangent_fp64 on every element (the metric of tangent_cases.py; the report says where its floor was needed), the outputs within the suite's 1e-4"""
    for log in _modes(case):
        tag = f"tangent_ref/{case['name']}/{'log' if log else 'lin'}"
        o64, t64, sc = TC.fp64(case, log)
        assert o64.shape == TC.out_shape(case) and np.isfinite(t64).all() and np.isfinite(sc).all()
        assert (np.abs(t64) <= sc * (1 + 1e-9) + 1e-300).all(), "scale bounds the tangent"
        o32, t32, _ = TC.fp32(case, log)
        st32 = assert_tangent(tag + "/fp32_restatement", t32, t64, sc, tol=REF_BAR, floor=TC.floor_of(case), shape=t64.shape)
        print(f"{tag}: fp32 restatement {st32['max_err']:.3g} (floored {st32['floored_max_err']:.3g})", end="")
        orc = TC.oracle(case, log)
        if orc is not None:
            o, t = orc
            st = assert_tangent(tag + "/oracle", t, t64, sc, tol=REF_BAR, floor=TC.floor_of(case), shape=t64.shape)
            print(f", oracle {st['max_err']:.3g} at {st['worst_index']}, {100 * st['frac_below_tol_of_largest']:.0f} % of the elements below "
                  f"1e-4 of the largest", end="")
            # outputs: linear relative, log absolute
            if log:
                assert float(np.abs(o - o64).max()) <= TOL
            else:
                nz = o64 != 0
                assert float((np.abs(o - o64)[nz] / np.abs(o64)[nz]).max(initial=0.0)) <= TOL and (o[~nz] == 0).all()
        print()


def _planted(case_name, pick):
    """a 1 % error on the tangent elements `pick(t64)` selects (a boolean mask) of the linear case: what both measures say"""
    case = TC.BY_NAME[case_name]
    _, t64, sc = TC.fp64(case, False)
    _, t = TC.oracle(case, False)
    bad = t.astype(np.float64).copy()
    mask = pick(sc)
    assert mask.any() and (sc[mask] > 0).all()
    bad[mask] *= 1.01
    return case, bad, t64, sc, tangent_stats(bad, t64, sc)


def test_metric_catches_an_error_in_the_quietest_mel_row():
    """1 % on every element of the mel row with the smallest tangents: the global-max measure the suite used does not see it"""
    def quietest_row(sc):
        m = np.zeros(sc.shape, dtype=bool)
        rows = sc.max(axis=(0, 1, 3))
        m[:, :, int(np.where(rows > 0, rows, np.inf).argmin()), :] = True
        return m
    case, bad, t64, sc, st = _planted("loud_tone_n1024", quietest_row)
    assert st["global_max_measure"] <= TOL, st                      # the old measure passes ...
    assert st["max_err"] > 10 * TOL, st                             # ... the new one sees most of the planted 1e-2
    with pytest.raises(AssertionError):
        assert_tangent("tangent_selfcheck/quiet_row", bad, t64, sc, shape=sc.shape)


def test_metric_catches_an_error_in_one_edge_frame():
    """1 % on the last frame of the last clip (mostly zero padding: small tangents)"""
    def edge_frame(sc):
        m = np.zeros(sc.shape, dtype=bool)
        m[-1, :, :, -1] = sc[-1, :, :, -1] > 0
        return m
    case, bad, t64, sc, st = _planted("loud_tone_n1024", edge_frame)
    assert st["global_max_measure"] <= TOL, st
    assert st["max_err"] > 10 * TOL, st
    with pytest.raises(AssertionError):
        assert_tangent("tangent_selfcheck/edge_frame", bad, t64, sc, shape=sc.shape)


def test_metric_demands_exact_zeros_where_nothing_can_contribute():
    case = TC.BY_NAME["wlc_m512_T36"]                               # 512 mel bands on 513 bins: bands of no bins
    _, t64, sc = TC.fp64(case, False)
    assert (sc == 0).any()
    bad = t64.copy()
    bad[sc == 0] = 1e-30
    with pytest.raises(AssertionError):
        assert_tangent("tangent_selfcheck/zeros", bad, t64, sc)
