#!/usr/bin/env python3
"""Per-clip lengths for the trainable filterbank (MelSpectrogramLayer(learnable_fb=True, lengths_learnable_fb=True)) at BASELINE config 2
(256 clips of 16000 samples, hop 512, 128 mel bands, lambd 128: n_fft 1024, log output, lambd on the device, spectrogram saved): forward +
backward to lambd.grad and mel_fb.grad per step of
  (a) forward(x)                                   the path the parent commit has: the yardstick
  (b) forward(x, lengths), every length 16000      the length-aware kernels with nothing to skip
  (c) lengths uniform in 4000 ... 16000 (seed 0)   a zero-padded batch
  (d) every length 8000                            half of every clip's tiles and K-blocks hold no frame
with mfma="fp32" (exact) and mfma="bf16x3".  Event timing over five alternated trains of 100 steps, twice: the eager steps, and the same
steps captured ten at a time with torch.cuda.graph and replayed.  Prints one JSON line -- microseconds per step, every train and the
medians, the ratios b/a, c/a, d/a of the medians -- and, with ``--out FILE``, writes it to FILE as well (the file committed under
profiles/).  There is no bar on these times: they are recorded."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_amd import MelSpectrogramLayer  # noqa: E402
from time_klen import _alternated, _captured  # noqa: E402

B, L, HOP, M, SR, LAM = 256, 16000, 512, 128, 16000, 128.0
DEV = "cuda:0"


def _summary(times, per_call, rounds, over):
    med = {k: sorted(v)[rounds // 2] / per_call for k, v in times.items()}
    return {**{k + "_us": [round(t / per_call, 2) for t in v] for k, v in times.items()},
            **{k + "_median_us": round(v, 2) for k, v in med.items()},
            **{k + "_over_a": round(med[k] / med["a_forward_x"], 3) for k in over}}


def main():
    reps, rounds, per_graph = 100, 5, 10
    x = 0.1 * torch.randn(B, L, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    g = torch.randn(B, 1, M, L // HOP + 1, device=DEV)
    lengths = {
        "b_full": torch.full((B,), L, dtype=torch.int32, device=DEV),
        "c_uniform_4000_16000": torch.from_numpy(np.random.default_rng(0).integers(4000, L + 1, size=B).astype(np.int32)).to(DEV),
        "d_all_8000": torch.full((B,), 8000, dtype=torch.int32, device=DEV),
    }
    res = {}
    for mfma in ("fp32", "bf16x3"):
        lay = MelSpectrogramLayer(torch.tensor(LAM), n_mels=M, n_points=L, sample_rate=SR, hop_length=HOP, device=DEV, optimized=True, log=True,
                                  learnable_fb=True, mfma=mfma, lengths_learnable_fb=True).to(DEV)
        with torch.no_grad():
            lay.mel_fb += 0.02 * torch.rand(lay.mel_fb.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))

        def step(ln=None):
            lay.lambd.grad = None
            lay.mel_fb.grad = None
            (lay(x) if ln is None else lay(x, ln)).backward(g)

        variants = {"a_forward_x": step}
        for key, ln in lengths.items():
            variants[key] = (lambda ln_: lambda: step(ln_))(ln)
        # (b) computes what (a) computes: the same bits
        step()
        ya, da, fa = lay(x).detach(), lay.lambd.grad.clone(), lay.mel_fb.grad.clone()
        step(lengths["b_full"])
        same_bits = bool(torch.equal(ya, lay(x, lengths["b_full"]).detach()) and torch.equal(da, lay.lambd.grad) and torch.equal(fa, lay.mel_fb.grad))
        eager = _alternated(variants, reps, rounds)
        replays = {k: _captured(fn, per_graph) for k, fn in variants.items()}
        graphed = _alternated(replays, reps // per_graph, rounds)
        res[mfma] = {"full_lengths_bit_identical": same_bits, "eager": _summary(eager, 1, rounds, lengths),
                     "graph": _summary(graphed, per_graph, rounds, lengths)}
    line = json.dumps({"tool": "tools/time_fb_lengths.py", "device": torch.cuda.get_device_name(0),
                       "units": "microseconds per step, event timing over trains of 100 steps, 5 alternated rounds on one box",
                       "config": "BASELINE c2 (B=256, L=16000, hop=512, M=128, lambd 128, log), trainable filterbank, spectrogram saved, "
                                 "forward + backward to lambd.grad and mel_fb.grad per step",
                       **res})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(json.loads(line), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
