#!/usr/bin/env python3
"""One K = 3 MultiWindowMelSpectrogram against three MelSpectrogramLayers at BASELINE config 2 (256 clips of 16000 samples, hop 512,
128 mel bands, log output): forward + backward to lambd per step, lambd on the device, for a set of three equal n_fft (128, 128, 128:
n_fft 1024 each) and a mixed one (40, 128, 300: n_fft 256 / 1024 / 2048).  Event timing over trains of steps, alternated A / B; prints
one JSON line (microseconds per step)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_amd import MelSpectrogramLayer, MultiWindowMelSpectrogram  # noqa: E402

B, L, HOP, M, SR = 256, 16000, 512, 128, 16000
SETS = {"same": [128.0, 128.0, 128.0], "mixed": [40.0, 128.0, 300.0]}


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


def main():
    reps, rounds = 100, 5
    x = 0.1 * torch.randn(B, L, device="cuda:0")
    res = {}
    for name, lams in SETS.items():
        multi = MultiWindowMelSpectrogram(lams, M, L, SR, hop_length=HOP, log=True).to("cuda:0")
        scal = [MelSpectrogramLayer(torch.tensor(v), n_mels=M, n_points=L, sample_rate=SR, hop_length=HOP, device="cuda:0", optimized=True,
                                    log=True).to("cuda:0") for v in lams]
        g3 = torch.randn(B, 3, M, L // HOP + 1, device="cuda:0")
        g1 = [g3[:, k:k + 1].contiguous() for k in range(3)]

        def step_multi():
            multi.lambd.grad = None
            multi(x).backward(g3)

        def step_scalar():
            for lay, g in zip(scal, g1):
                lay.lambd.grad = None
                lay(x).backward(g)

        a, b = [], []
        for _ in range(rounds):
            a.append(_train(step_multi, reps))
            b.append(_train(step_scalar, reps))
        res[name] = {"multi_K3_us": [round(v, 2) for v in a], "three_scalar_us": [round(v, 2) for v in b],
                     "ratio_median": round(sorted(a)[rounds // 2] / sorted(b)[rounds // 2], 3)}
    print(json.dumps({"config": "BASELINE c2 (B=256, L=16000, hop=512, M=128, log), forward+backward per step", **res}))


if __name__ == "__main__":
    main()
