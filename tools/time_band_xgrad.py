#!/usr/bin/env python3
"""BandSplitMelSpectrogram(waveform_grad=True) (A) against what a user wrote before it existed (B): MultiWindowMelSpectrogram(waveform_grad=True)
with the same widths followed by torch.cat([y[:, k, e_k:e_{k+1}] for k ...], 1).unsqueeze(1) -- autograd scatters the cotangent back into a
(B, K, M, T) tensor.  BASELINE config 2 (256 clips of 16000 samples, hop 512, 128 mel bands, log output, lambd on the device), default edges,
forward + backward to lambd.grad AND x.grad per step, for the mixed set (300, 128, 40: n_fft 2048 / 1024 / 256) and the equal one
(128, 128, 128).  Event timing over five alternated trains of 100 steps; prints one JSON line (microseconds per step, every train and the
medians).  --once: thirty steps of A, then thirty of B, untimed (for a kernel trace)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram  # noqa: E402

B, L, HOP, M, SR = 256, 16000, 512, 128, 16000
SETS = {"mixed": [300.0, 128.0, 40.0], "same": [128.0, 128.0, 128.0]}


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
    once = "--once" in sys.argv
    x = (0.1 * torch.randn(B, L, device="cuda:0")).requires_grad_(True)
    g = torch.randn(B, 1, M, L // HOP + 1, device="cuda:0")
    res = {}
    for name, lams in SETS.items():
        band = BandSplitMelSpectrogram(lams, M, L, SR, hop_length=HOP, log=True, waveform_grad=True).to("cuda:0")
        multi = MultiWindowMelSpectrogram(lams, M, L, SR, hop_length=HOP, log=True, waveform_grad=True).to("cuda:0")
        e = band.band_edges

        def step_band():
            band.lambd.grad = None
            x.grad = None
            band(x).backward(g)

        def step_multi_cat():
            multi.lambd.grad = None
            x.grad = None
            y = multi(x)
            torch.cat([y[:, k, e[k]:e[k + 1]] for k in range(len(lams))], 1).unsqueeze(1).backward(g)

        # the two routes compute the same thing: y and x.grad bit for bit (the cotangent scattered by autograd has +0.0 outside the groups)
        step_band()
        ga = x.grad.clone()
        step_multi_cat()
        torch.cuda.synchronize()
        same_bits = bool(torch.equal(ga, x.grad))
        if once:
            for _ in range(30):
                step_band()
            for _ in range(30):
                step_multi_cat()
            torch.cuda.synchronize()
            continue
        a, b = [], []
        for _ in range(rounds):
            a.append(_train(step_band, reps))
            b.append(_train(step_multi_cat, reps))
        res[name] = {"lambd": lams, "x_grad_bit_identical": same_bits, "band_split_us": [round(v, 2) for v in a],
                     "multi_window_cat_us": [round(v, 2) for v in b],
                     "band_split_median_us": round(sorted(a)[rounds // 2], 2), "multi_window_cat_median_us": round(sorted(b)[rounds // 2], 2),
                     "ratio_median": round(sorted(a)[rounds // 2] / sorted(b)[rounds // 2], 3),
                     "slower_in_pairs": sum(1 for u, v in zip(a, b) if u > v)}
    if not once:
        print(json.dumps({"config": "BASELINE c2 (B=256, L=16000, hop=512, M=128, log), forward + backward to lambd.grad and x.grad per step, "
                                    "default edges", **res}))


if __name__ == "__main__":
    main()
