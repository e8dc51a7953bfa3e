#!/usr/bin/env python3
"""Per-clip lengths on the two K-window layers (per_clip_lengths=True) at BASELINE config 2 (256 clips of 16000 samples, hop 512, 128 mel bands,
log output, lambd on the device), windows (300, 128, 40: n_fft 2048 / 1024 / 256): forward + backward to lambd.grad per step of
  (a) forward(x)                                   the path every earlier build has
  (b) forward(x, lengths), every length 16000      the length-aware kernels with nothing to skip
  (c) lengths uniform in 4000 ... 16000 (seed 0)   a zero-padded batch
  (d) every length 8000                            half of every clip's tiles are pad tiles
for MultiWindowMelSpectrogram and BandSplitMelSpectrogram (default edges).  Event timing over five alternated trains of 100 steps, twice: the
eager steps, and the same steps captured ten at a time with torch.cuda.graph and replayed (no Python between the kernels).  Prints one JSON
line -- microseconds per step, every train and the medians, the ratios b/a, c/a, d/a of the medians and whether (d) came out faster than (a),
for both -- and, with ``--out FILE``, writes it to FILE as well (the file committed under profiles/)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_amd import BandSplitMelSpectrogram, MultiWindowMelSpectrogram  # noqa: E402

B, L, HOP, M, SR = 256, 16000, 512, 128, 16000
LAMS = [300.0, 128.0, 40.0]
DEV = "cuda:0"


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


def _captured(fn, steps):
    """fn captured `steps` times into one graph (after an eager warm-up on a side stream); returns the replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(steps):
            fn()
    return graph.replay


def _alternated(variants, reps, rounds):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(_train(fn, reps))
    return times


def _summary(times, per_call, rounds, over):
    med = {k: sorted(v)[rounds // 2] / per_call for k, v in times.items()}
    return {**{k + "_us": [round(t / per_call, 2) for t in v] for k, v in times.items()},
            **{k + "_median_us": round(v, 2) for k, v in med.items()},
            **{k + "_over_a": round(med[k] / med["a_forward_x"], 3) for k in over},
            # half of every clip's tiles are pad tiles in (d): it is expected below (a)
            "d_faster_than_a": bool(med["d_all_8000"] < med["a_forward_x"]),
            "d_faster_than_a_in_trains": sum(1 for u, v in zip(times["d_all_8000"], times["a_forward_x"]) if u < v)}


def main():
    reps, rounds, per_graph = 100, 5, 10
    x = 0.1 * torch.randn(B, L, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    lengths = {
        "b_full": torch.full((B,), L, dtype=torch.int32, device=DEV),
        "c_uniform_4000_16000": torch.from_numpy(np.random.default_rng(0).integers(4000, L + 1, size=B).astype(np.int32)).to(DEV),
        "d_all_8000": torch.full((B,), 8000, dtype=torch.int32, device=DEV),
    }
    res = {}
    for name, cls, K in (("multi_window", MultiWindowMelSpectrogram, len(LAMS)), ("band_split", BandSplitMelSpectrogram, 1)):
        lay = cls(LAMS, M, L, SR, hop_length=HOP, log=True, per_clip_lengths=True).to(DEV)
        g = torch.randn(B, K, M, L // HOP + 1, device=DEV)

        def step(ln=None):
            lay.lambd.grad = None
            (lay(x) if ln is None else lay(x, ln)).backward(g)

        variants = {"a_forward_x": step}
        for key, ln in lengths.items():
            variants[key] = (lambda ln_: lambda: step(ln_))(ln)
        # (b) computes what (a) computes: the same bits
        with torch.no_grad():
            same_bits = bool(torch.equal(lay(x), lay(x, lengths["b_full"])))
        eager = _alternated(variants, reps, rounds)
        replays = {k: _captured(fn, per_graph) for k, fn in variants.items()}
        graphed = _alternated(replays, reps // per_graph, rounds)
        res[name] = {"full_lengths_bit_identical": same_bits, "eager": _summary(eager, 1, rounds, lengths),
                     "graph": _summary(graphed, per_graph, rounds, lengths)}
    line = json.dumps({"tool": "tools/time_klen.py", "device": torch.cuda.get_device_name(0),
                       "units": "microseconds per step, event timing over trains of 100 steps, 5 alternated rounds on one box",
                       "config": "BASELINE c2 (B=256, L=16000, hop=512, M=128, log), windows 300 / 128 / 40, forward + backward to lambd.grad per step",
                       **res})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(json.loads(line), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
