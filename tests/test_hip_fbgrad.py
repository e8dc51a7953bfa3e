"""The filterbank gradient element by element on every kernel path: all 16 instantiations of dmel_fbgrad_lds_kernel (LOG x TINY x BF16X3 x
LEN: the log output, T < 4, DMEL_FLAG_MFMA_BF16X3, per-clip lengths) and dmel_fbgrad_reduce_kernel, through dmel_backward_fb, _dev, _saved,
_saved_dl, _dev_lengths, _saved_lengths and the layer, against oracle/torch_restatement.py: fbgrad_fp64 given the kernel's own saved log
output, in the metric of tests/fbgrad_cases.py: |got - ref| over sum spec |gm| of the element, TOL = 1e-4 on EVERY element, no floor, exact
zeros where nothing contributes.  The table in tests/fbgrad_cases.py maps each case to the edge of dmel_aux.hip it exercises;
tests/test_fbgrad_restatement_cpu.py holds the references to a quarter of the bar on these very inputs.

Every run writes into a NaN-filled gradient between sentinel guards (asserted untouched) and is repeated: the same bits.  Per case and
variant the worst element and its index, the measure the suite used until here (one maximum over the largest element) and the share of the
tensor that measure could not see are printed and go to the parity report.  Outputs and saved spectrograms are tested elsewhere: only what
the reference needs is read back."""
import numpy as np
import pytest
import torch

import fbgrad_cases as FC
from fbgrad_cases import EPS, TOL, assert_fbgrad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
GUARD = 64                      # floats on either side of grad_fb (256 bytes: the gradient stays aligned)


def _guarded(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    return flat, view


def _guards_untouched(flat):
    return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all())


class _Run:
    """one case on the device: the forward that saves what the backward is given (log output, and per entry point the spectrogram and the
    tangent), then `grads(log, bf16x3)` -> {entry point: grad_fb} with the guards checked"""

    def __init__(self, case):
        from dmel_amd import capi
        self.capi, self.case = capi, case
        c = case
        self.B, self.M, self.T, self.n = c["B"], c["n_mels"], FC.n_time(c), FC.n_fft_of(c)
        self.F = self.n // 2 + 1
        self.x = torch.from_numpy(np.array(FC.make_input(c))).to(DEV)
        self.g = torch.from_numpy(np.array(FC.make_cotangent(c))).to(DEV)
        self.st = torch.cuda.current_stream().cuda_stream
        self.plan = capi.Plan(c["L"], c["hop"], self.M, c["sr"], c["f_min"], c["f_max"], c["normalize_window"])
        self.full = 0 if c["optimized"] else capi.DMEL_FLAG_FULL_WINDOW
        self.y = torch.full(FC.out_shape(c), SENTINEL, device=DEV)
        self.lam = torch.tensor(float(c["lambd"]), dtype=torch.float32, device=DEV)
        self.dl = None
        e = c["entry"]
        if e in ("host", "dev"):
            self.plan.forward(self.x.data_ptr(), self.B, c["lambd"], self.y.data_ptr(), None, True, EPS, self.st, extra_flags=self.full)
        else:
            # the trainable-filterbank forwards: the bank given as a matrix (here the HTK one), the spectrogram and the tangent written out
            from oracle import dmel_oracle as O
            bank = O.mel_fbanks(self.F, c["f_min"], float(c["sr"] // 2) if c["f_max"] is None else c["f_max"], self.M, c["sr"])
            if e == "lengths":
                # from the device, as the layer uploads its parameter: dmel_forward_dev_fixed_lengths saves the spectrogram from the kernels of
                # a trained (dense) bank only, and a bank given from the host with the HTK zeros is scheduled band by band
                self.bank = torch.from_numpy(bank).to(DEV)
                self.plan.set_filterbank_dev(self.n, self.bank.data_ptr(), self.st)
            else:
                self.plan.set_filterbank(self.n, bank)
            self.tan = torch.full(FC.out_shape(c), SENTINEL, device=DEV)
            self.spec = torch.full((self.B, self.F, self.T), SENTINEL, device=DEV)
            self.scratch = torch.zeros(self.plan.scratch_bytes(self.B), dtype=torch.uint8, device=DEV)
            if e == "lengths":
                self.lengths = torch.tensor(c["lengths"], dtype=torch.int32, device=DEV)
                self.plan.forward_dev_fixed_lengths(self.x.data_ptr(), self.lengths.data_ptr(), self.B, self.lam.data_ptr(), self.n, self.y.data_ptr(),
                                                    self.tan.data_ptr(), self.spec.data_ptr(), True, EPS, self.st, self.scratch.data_ptr())
            else:
                self.plan.forward_dev_fixed_spec(self.x.data_ptr(), self.B, self.lam.data_ptr(), self.n, self.y.data_ptr(), self.tan.data_ptr(),
                                                 self.spec.data_ptr(), True, EPS, self.st, self.scratch.data_ptr())
        torch.cuda.synchronize()
        self.y_np = self.y.cpu().numpy()

    def grads(self, log, bf16x3):
        c, p, capi = self.case, self.plan, self.capi
        flags = self.full | (capi.DMEL_FLAG_MFMA_BF16X3 if bf16x3 else 0)
        xp, gp, yp, B, n, st = self.x.data_ptr(), self.g.data_ptr(), self.y.data_ptr() if log else None, self.B, self.n, self.st
        calls = {
            "host": {"backward_fb": lambda o: p.backward_fb(xp, B, c["lambd"], gp, yp, o, log, st, extra_flags=flags)},
            "dev": {"backward_fb_dev": lambda o: p.backward_fb_dev(xp, B, self.lam.data_ptr(), n, gp, yp, o, log, st, extra_flags=flags)},
            "saved": {"backward_fb_saved": lambda o: p.backward_fb_saved(self.spec.data_ptr(), B, n, gp, yp, o, log, st, extra_flags=flags)},
            "saved_dl": {"backward_fb_saved_dl": lambda o: p.backward_fb_saved_dl(self.spec.data_ptr(), B, n, gp, yp, self.tan.data_ptr(), o, self.dl.data_ptr(),
                                                                                 self.scratch.data_ptr(), log, st, extra_flags=flags)},
            "lengths": {"backward_fb_dev_lengths": lambda o: p.backward_fb_dev_lengths(xp, self.lengths.data_ptr(), B, self.lam.data_ptr(), n, gp, yp, o, log, st,
                                                                                       extra_flags=flags),
                        "backward_fb_saved_lengths": lambda o: p.backward_fb_saved_lengths(self.spec.data_ptr(), self.lengths.data_ptr(), B, n, gp, yp, None, o, None,
                                                                                           None, log, st, extra_flags=flags)},
        }[c["entry"]]
        res = {}
        for name, call in calls.items():
            if c["entry"] == "saved_dl":
                self.dl = torch.full((1,), float("nan"), device=DEV)
            flat, gfb = _guarded((self.F, self.M))
            call(gfb.data_ptr())
            torch.cuda.synchronize()
            assert _guards_untouched(flat), (c["name"], name, "a store outside grad_fb")
            flat2, gfb2 = _guarded((self.F, self.M))
            call(gfb2.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(gfb.view(torch.int32), gfb2.view(torch.int32)), (c["name"], name, "a second call gives other bits")
            res[name] = gfb.cpu().numpy()
        return res

    def close(self):
        self.plan.close()


def _check(case, tag, got, log, y_np, ref_cache):
    """`got` against fbgrad_fp64 given the saved log output `y_np` (one reference per case and output kind: the exact and the BF16X3 run share it)"""
    if log not in ref_cache:
        ref_cache[log] = FC.fp64_with_out(case, y_np) if log else FC.fp64_lin(case)
    ref, sc = ref_cache[log]
    assert got.shape == ref.shape
    st = FC.fbgrad_stats(got, ref, sc)
    print(f"{tag}: max err {st['max_err']:.3g} at {np.unravel_index(st['worst_index'], ref.shape)}, old measure {st['global_max_measure']:.3g}, "
          f"{100 * st['frac_below_tol_of_largest']:.1f} % of the elements below 1e-4 of the largest")
    return assert_fbgrad(tag, got, ref, sc, shape=ref.shape)


def _assert_slices(case):
    """the slice layout the case is named for, on the device at hand (fbgrad_splits restated in fbgrad_cases.expected_splits)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = FC.expected_splits(case, cus)
    blocks = case["B"] * -(-FC.n_time(case) // FC.KB)
    largest, spans = FC.slice_layout(case, splits)
    if case["splits"] is not None:
        assert splits == case["splits"] == blocks, (case["name"], splits, blocks, cus)
        assert splits % FC.RED_WAVES != 0 and (FC.grad_shape(case)[0] * FC.grad_shape(case)[1]) % 64 != 0
    if case["slices"] is not None:
        assert blocks > splits and spans >= 1, (case["name"], "more K-blocks than slices, a slice across a clip boundary", blocks, splits, spans, cus)
        if case["slices"] == "deep":
            assert largest > FC.DEPTH, (case["name"], "a slice of more than DEPTH blocks", largest, splits, cus)
    if case["entry"] == "lengths" and FC.n_time(case) >= 33:
        # a slice of two or more blocks that starts in a clip whose trailing blocks are all pad and ends in the next clip
        ntc = -(-FC.n_time(case) // FC.KB)
        base, rem = divmod(blocks, splits)
        lo, found = 0, False
        for s in range(splits):
            k = base + (1 if s < rem else 0)
            b0, b1 = lo // ntc, (lo + k - 1) // ntc if k else lo // ntc
            if k >= 2 and b1 > b0 and -(-FC.frames_of(case)[b0] // FC.KB) < ntc:
                found = True
            lo += k
        assert blocks > splits and found, (case["name"], "slices across a clip whose pad blocks are skipped", blocks, splits, cus)


C_ABI = [c for c in FC.CASES if c["entry"] != "layer"]


@pytest.mark.parametrize("case", C_ABI, ids=[c["name"] for c in C_ABI])
def test_fbgrad_matches_fp64_elementwise(case):
    _assert_slices(case)
    run = _Run(case)
    try:
        refs = {}
        for log in (False, True):
            for bf16x3 in (False, True):
                for entry, got in run.grads(log, bf16x3).items():
                    tag = f"fbgrad/{case['name']}/{entry}/{'log' if log else 'lin'}/{'bf16x3' if bf16x3 else 'fp32'}"
                    assert np.isfinite(got).all(), (tag, "an element of grad_fb was never written (NaN prefill) or is not finite")
                    _check(case, tag, got, log, run.y_np, refs)
                if case["entry"] == "saved_dl":
                    # d lambd of the same launch (M <= 128) or of the stand-alone kernel: the fp64 dot of what it was given; the kernels add in
                    # fp64 and round once to fp32: one fp32 rounding of the result + n 2^-53 sum |g t| (as tests/test_hip_write_through.py)
                    gt = run.g.double() * run.tan.double()
                    want, mag = float(gt.sum()), float(gt.abs().sum())
                    d = float(run.dl)
                    print(f"fbgrad/{case['name']}/dlambd: {d:.9g} against {want:.9g} (sum of magnitudes {mag:.3g})")
                    assert abs(d - want) <= 2.0 ** -24 * abs(want) + gt.numel() * 2.0 ** -53 * mag, (case["name"], d, want, mag)
    finally:
        run.close()


@pytest.mark.parametrize("mfma", ["fp32", "bf16x3"])
@pytest.mark.parametrize("log", [False, True], ids=["lin", "log"])
def test_layer_with_a_trained_bank_matches_fp64_elementwise(log, mfma):
    """MelSpectrogramLayer(learnable_fb=True) after one optimiser step on the bank: no longer the HTK bank, so the reference takes the saved
    output of the layer itself"""
    from dmel_amd import MelSpectrogramLayer
    case = FC.BY_NAME["entry_layer"]
    x = torch.from_numpy(np.array(FC.make_input(case))).to(DEV)
    g = torch.from_numpy(np.array(FC.make_cotangent(case))).to(DEV)
    lay = MelSpectrogramLayer(torch.tensor(float(case["lambd"])), n_mels=case["n_mels"], n_points=case["L"], sample_rate=case["sr"],
                              hop_length=case["hop"], device=DEV, optimized=True, log=log, eps=EPS, learnable_fb=True, mfma=mfma).to(DEV)
    # (the step: SGD on a seeded negative gradient, so that the bank moves off the HTK values, becomes dense and stays positive -- the log
    # output exists; the loss's own gradient of the log output is 1e10 in the columns of empty bands)
    opt = torch.optim.SGD([lay.mel_fb], lr=0.02)
    fb0 = lay.mel_fb.detach().clone()
    lay.mel_fb.grad = -torch.rand(fb0.shape, generator=torch.Generator().manual_seed(case["seed"])).to(DEV)
    opt.step()
    assert bool((lay.mel_fb.detach() > fb0).any()) and bool((lay.mel_fb.detach() >= 0).all())
    got = []
    for _ in range(2):
        lay.zero_grad(set_to_none=True)
        y = lay(x)
        (y * g).sum().backward()
        torch.cuda.synchronize()
        got.append(lay.mel_fb.grad.detach().clone())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    assert torch.isfinite(got[0]).all()
    _check(case, f"fbgrad/entry_layer/layer/{'log' if log else 'lin'}/{mfma}", got[0].cpu().numpy(), log, y.detach().cpu().numpy(), {})
