#!/usr/bin/env python3
"""MelSpectrogramLayer with and without per-clip lengths: the training forward alone and forward + backward to lambd.grad, lambd on the
device, device-event timing over trains of steps after warm-up, the variants alternated.  BASELINE config 2 (256 clips of 16000 samples,
hop 512, 128 mel bands, n_fft 1024, log) with lengths = n_points, all n_points / 2, and uniform in [n_points / 4, n_points]; and the
reference's audio_mnist shape (64 clips of 8000 samples at 8 kHz, hop 80, 64 mel bands, lambd 46.67: n_fft 512) with lengths uniform in
2400 ... 8000.  Writes profiles/r07_lengths.json, or the path given (microseconds per step, medians over the rounds)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import MelSpectrogramLayer  # noqa: E402

DEV = "cuda:0"
SHAPES = {"c2": dict(B=256, L=16000, hop=512, M=128, sr=16000, lam=128.0), "audio_mnist": dict(B=64, L=8000, hop=80, M=64, sr=8000, lam=46.67)}


def _train(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def _median(v):
    return round(sorted(v)[len(v) // 2], 2)


def main():
    reps, rounds = 200, 5
    gen = torch.Generator(DEV).manual_seed(0)
    out = {}
    for shape, s in SHAPES.items():
        B, L = s["B"], s["L"]
        lay = MelSpectrogramLayer(torch.tensor(s["lam"]), n_mels=s["M"], n_points=L, sample_rate=s["sr"], hop_length=s["hop"], device=DEV,
                                  optimized=True, log=True).to(DEV)
        x = 0.1 * torch.randn(B, L, device=DEV, generator=gen)
        g = torch.randn(B, 1, s["M"], L // s["hop"] + 1, device=DEV, generator=gen)
        if shape == "c2":
            sets = {"full": torch.full((B,), L, dtype=torch.int32, device=DEV),
                    "half": torch.full((B,), L // 2, dtype=torch.int32, device=DEV),
                    "uniform_quarter_to_full": torch.randint(L // 4, L + 1, (B,), device=DEV, generator=gen, dtype=torch.int32)}
        else:
            sets = {"uniform_2400_8000": torch.randint(2400, L + 1, (B,), device=DEV, generator=gen, dtype=torch.int32)}

        def fwd(ln):
            return lambda: lay(x) if ln is None else lay(x, ln)

        def step(ln):
            def f():
                lay.lambd.grad = None
                (lay(x) if ln is None else lay(x, ln)).backward(g)
            return f

        def graphed(ln, n=20):
            # n training forwards captured into one graph (no host issue in the timed region): us per forward = replay time / n
            f = fwd(ln)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(n):
                    f()
            return lambda: [gr.replay() for _ in range(reps // n)]

        res = {}
        variants = {"none": None, **sets}
        times = {k: {"forward_us": [], "forward_backward_us": [], "forward_graph_us": []} for k in variants}
        lay.set_tracking(8, 3)                  # (guards near an n_fft boundary only, as GraphedStep sets it)
        for k, ln in variants.items():          # eager calls first: the sync-free path reads lambd once before a capture
            _train(fwd(ln), 20)
        replays = {k: graphed(ln) for k, ln in variants.items()}
        for _ in range(rounds):
            for k, ln in variants.items():
                times[k]["forward_us"].append(_train(fwd(ln), reps))
                times[k]["forward_backward_us"].append(_train(step(ln), reps))
                times[k]["forward_graph_us"].append(_train(replays[k], 1) / reps)
        for k, t in times.items():
            res[k] = {m: _median(v) for m, v in t.items()}
            res[k]["trains"] = {m: [round(u, 2) for u in v] for m, v in t.items()}
            if variants[k] is not None:
                res[k]["mean_length"] = round(float(variants[k].float().mean()), 1)
        out[shape] = {"shape": s, **res}
    line = {"what": "MelSpectrogramLayer training forward / forward + backward to lambd.grad, lambd on the device, without lengths ('none') "
                    f"and with them; device events over trains of {reps} steps after 10 warm-up steps, {rounds} rounds alternated, medians; "
                    "forward_graph_us: the same forward replayed from a captured graph of 20 (no host issue)",
            **out}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_lengths.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps({k: {kk: (vv if not isinstance(vv, dict) or "trains" not in vv else {m: vv[m] for m in ("forward_us", "forward_backward_us",
                                                                                                            "forward_graph_us")})
                          for kk, vv in v.items() if kk != "shape"} for k, v in out.items()}))


if __name__ == "__main__":
    main()
