#!/usr/bin/env python3
"""One forward + backward to lambd.grad AND x.grad over a zero-padded batch, the K-window layer against the K scalar layers it replaces:
  (a) MultiWindowMelSpectrogram / BandSplitMelSpectrogram(per_clip_lengths=True, lengths_waveform_grad=True)(x, lengths);
  (b) K MelSpectrogramLayer(lengths_waveform_grad=True)(x, lengths), their outputs joined with torch.cat (channels, or each layer's own rows
      for the band layer) so that one backward reaches all of them and autograd sums the K waveform gradients.
Shape: K = 3 at n_fft 256 / 1024 / 2048 (lambd 40 / 128 / 300), 64 clips of 16000 samples, hop 160, 64 mel bands, log output, lengths drawn
uniformly from 0.25 ... 1 x n_points (seeded).  Both variants sync-free.  Each is timed eagerly (host issue included) and replayed from a
captured graph of one step; device events over trains of steps after warm-up, five rounds with the variants alternated.
Usage: time_klen_xgrad.py --layer multi|band [--out PATH].  Writes profiles/r17_klen_xgrad_<layer>.json, or the path given: microseconds
per step, the median of the trains and their spread (max - min)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram  # noqa: E402

DEV = "cuda:0"
B, L, HOP, M, SR = 64, 16000, 160, 64, 16000
LAMS = [40.0, 128.0, 300.0]
STEPS, ROUNDS = 200, 5


def _train(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / STEPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", choices=("multi", "band"), required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    band = args.layer == "band"
    K, T = len(LAMS), L // HOP + 1
    gen = torch.Generator(DEV).manual_seed(0)
    x = (0.1 * torch.randn(B, L, device=DEV, generator=gen)).requires_grad_(True)
    g = torch.randn(B, 1 if band else K, M, T, device=DEV, generator=gen)
    lengths = torch.randint(L // 4, L + 1, (B,), device=DEV, generator=gen).to(torch.int32)
    kw = dict(hop_length=HOP, log=True)
    if band:
        one = BandSplitMelSpectrogram(LAMS, M, L, SR, per_clip_lengths=True, lengths_waveform_grad=True, **kw).to(DEV)
        edges = one.band_edges
    else:
        one = MultiWindowMelSpectrogram(LAMS, M, L, SR, per_clip_lengths=True, lengths_waveform_grad=True, **kw).to(DEV)
    many = [MelSpectrogramLayer(torch.tensor(v), n_mels=M, n_points=L, sample_rate=SR, device=DEV, optimized=True, lengths_waveform_grad=True,
                                **kw).to(DEV) for v in LAMS]
    gx = {k: torch.empty_like(x) for k in ("a", "b")}
    dl = {k: torch.empty(K, device=DEV) for k in ("a", "b")}

    def step_a():
        a, d = torch.autograd.grad(one(x, lengths), (x, one.lambd), g)
        gx["a"].copy_(a)
        dl["a"].copy_(d)

    def step_b():
        ys = [lay(x, lengths) for lay in many]
        y = torch.cat([yk[:, :, edges[k]:edges[k + 1]] for k, yk in enumerate(ys)], dim=2) if band else torch.cat(ys, dim=1)
        grads = torch.autograd.grad(y, [x] + [lay.lambd for lay in many], g)
        gx["b"].copy_(grads[0])
        dl["b"].copy_(torch.stack(grads[1:]))

    steps = {"a_k_window_layer": step_a, "b_k_scalar_layers": step_b}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs = {}
    with torch.cuda.stream(side):
        for name, fn in steps.items():
            for _ in range(3):
                fn()                                                 # eager first: workspaces are sized outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the two variants compute the same thing (autograd's order of the K terms is its own: compared to rounding, not on bits)
    scale = float(gx["b"].abs().max())
    agree = float((gx["a"] - gx["b"]).abs().max()) / scale
    assert agree < 1e-5 and torch.allclose(dl["a"], dl["b"], rtol=1e-5), (agree, dl)
    for name, fn in steps.items():
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs[name] = gr
    trains = {mode: {name: [] for name in steps} for mode in ("eager", "graph")}
    for _ in range(ROUNDS):
        for name, fn in steps.items():
            trains["eager"][name].append(round(_train(fn), 2))
            trains["graph"][name].append(round(_train(graphs[name].replay), 2))
    res = {mode: {name: {"median_us": sorted(v)[len(v) // 2], "spread_us": round(max(v) - min(v), 2), "trains_us": v} for name, v in per.items()}
           for mode, per in trains.items()}
    line = {"tool": "tools/time_klen_xgrad.py", "device": "MI355X (gfx950)", "layer": args.layer,
            "what": f"one forward + backward to lambd.grad and x.grad of a zero-padded batch: B={B}, L={L}, hop={HOP}, M={M}, lambd {LAMS} "
                    f"(n_fft 256 / 1024 / 2048), log, lengths uniform in {L // 4} ... {L}; device events over trains of {STEPS} steps, {ROUNDS} "
                    "rounds alternated; microseconds per step, median of the trains and their spread (max - min)",
            "mean_length": round(float(lengths.float().mean()), 1), "max_rel_difference_of_x_grad": agree, **res}
    path = args.out or os.path.join(ROOT, "profiles", f"r17_klen_xgrad_{args.layer}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
