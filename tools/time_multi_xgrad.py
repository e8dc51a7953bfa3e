#!/usr/bin/env python3
"""The waveform gradient of one K = 3 MultiWindowMelSpectrogram(waveform_grad=True) against three MelSpectrogramLayers at BASELINE config 2
(256 clips of 16000 samples, hop 512, 128 mel bands, log output): forward + backward per step with lambd on the device and both lambd and x
requiring grad (B: x.grad accumulated by autograd over the three layers), for a mixed set (40, 128, 300: n_fft 256 / 1024 / 2048) and an equal
one (128 x 3: n_fft 1024).  Event timing over trains of steps, alternated A / B, median of five; prints one JSON line (microseconds per step).
--trace: five A steps and five B steps of the mixed set only, untimed (for a kernel trace: launches per backward = count / 5)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_amd import MelSpectrogramLayer, MultiWindowMelSpectrogram  # noqa: E402

B, L, HOP, M, SR = 256, 16000, 512, 128, 16000
SETS = {"mixed": [40.0, 128.0, 300.0], "same": [128.0, 128.0, 128.0]}


def _train(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def _steps(lams, x):
    multi = MultiWindowMelSpectrogram(lams, M, L, SR, hop_length=HOP, log=True, waveform_grad=True).to("cuda:0")
    scal = [MelSpectrogramLayer(torch.tensor(v), n_mels=M, n_points=L, sample_rate=SR, hop_length=HOP, device="cuda:0", optimized=True,
                                log=True).to("cuda:0") for v in lams]
    g3 = torch.randn(B, 3, M, L // HOP + 1, device="cuda:0")
    g1 = [g3[:, k:k + 1].contiguous() for k in range(3)]
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)

    def step_multi():
        multi.lambd.grad = None
        xa.grad = None
        multi(xa).backward(g3)

    def step_scalar():
        xb.grad = None
        for lay, g in zip(scal, g1):
            lay.lambd.grad = None
            lay(xb).backward(g)

    return step_multi, step_scalar


def main():
    x = 0.1 * torch.randn(B, L, device="cuda:0")
    if "--trace" in sys.argv:
        a, b = _steps(SETS["mixed"], x)
        for fn in (a, b):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"trace": "mixed", "steps_each": 5}))
        return
    reps, rounds = 50, 5
    res = {}
    for name, lams in SETS.items():
        step_multi, step_scalar = _steps(lams, x)
        a, b = [], []
        for _ in range(rounds):
            a.append(_train(step_multi, reps))
            b.append(_train(step_scalar, reps))
        ma, mb = sorted(a)[rounds // 2], sorted(b)[rounds // 2]
        res[name] = {"lambd": lams, "multi_K3_us": [round(v, 2) for v in a], "three_scalar_us": [round(v, 2) for v in b],
                     "multi_K3_median_us": round(ma, 2), "three_scalar_median_us": round(mb, 2), "ratio_median": round(ma / mb, 3)}
    print(json.dumps({"config": "BASELINE c2 (B=256, L=16000, hop=512, M=128, log), forward + backward to lambd and x per step", **res}))


if __name__ == "__main__":
    main()
