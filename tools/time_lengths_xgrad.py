#!/usr/bin/env python3
"""The waveform gradient's launches alone, with and without per-clip lengths, at BASELINE config 2 (256 clips of 16000 samples, hop 512, 128
mel bands, lambd 128: n_fft 1024, log output): (a) dmel_backward_x, the fixed-length path; (b) dmel_backward_x_lengths with every length at
n_points; (c) dmel_backward_x_lengths with lengths spread evenly over n_points / 4 ... n_points.  Each variant is 20 calls captured into one
graph (no host issue in the timed region); device events over trains of 4000 calls after warm-up, five rounds with the variants alternated.
Writes profiles/r09_lengths_xgrad_c2.json, or the path given: microseconds per call, the median of the trains and their spread (max - min)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import MelSpectrogramLayer  # noqa: E402

DEV = "cuda:0"
B, L, HOP, M, SR, LAM = 256, 16000, 512, 128, 16000, 128.0
PER_GRAPH, REPLAYS, ROUNDS = 20, 200, 5


def _train(graph):
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / (REPLAYS * PER_GRAPH)


def main():
    gen = torch.Generator(DEV).manual_seed(0)
    lay = MelSpectrogramLayer(torch.tensor(LAM), n_mels=M, n_points=L, sample_rate=SR, hop_length=HOP, device=DEV, optimized=True, log=True,
                              lambd_sync=True).to(DEV)
    plan = lay._plan_for(torch.device(DEV))
    x = 0.1 * torch.randn(B, L, device=DEV, generator=gen)
    g = torch.randn(B, 1, M, L // HOP + 1, device=DEV, generator=gen)
    gx = torch.empty_like(x)
    full = torch.full((B,), L, dtype=torch.int32, device=DEV)
    spread = torch.linspace(L // 4, L, B, device=DEV).round().to(torch.int32)
    with torch.no_grad():
        y_full, y_spread = lay(x, full), lay(x, spread)
    stream = lambda: int(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    calls = {
        "a_fixed_length": lambda: plan.backward_x(x.data_ptr(), B, LAM, g.data_ptr(), y_full.data_ptr(), gx.data_ptr(), True, stream()),
        "b_lengths_full": lambda: plan.backward_x_lengths(x.data_ptr(), full.data_ptr(), B, LAM, g.data_ptr(), y_full.data_ptr(), gx.data_ptr(),
                                                          True, stream()),
        "c_lengths_spread": lambda: plan.backward_x_lengths(x.data_ptr(), spread.data_ptr(), B, LAM, g.data_ptr(), y_spread.data_ptr(),
                                                            gx.data_ptr(), True, stream()),
    }
    graphs = {}
    for k, f in calls.items():
        f()                                                          # eager first: the plan's workspace is sized outside the capture
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(PER_GRAPH):
                f()
        graphs[k] = gr
    trains = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            trains[k].append(round(_train(graphs[k]), 2))
    res = {k: {"median_us": sorted(v)[len(v) // 2], "spread_us": round(max(v) - min(v), 2), "trains_us": v} for k, v in trains.items()}
    line = {"tool": "tools/time_lengths_xgrad.py", "device": "MI355X (gfx950)",
            "what": f"the x-gradient launches alone (wave kernel + combine pass) at BASELINE config 2 (B={B}, L={L}, hop={HOP}, M={M}, n_fft 1024, "
                    f"log); {PER_GRAPH} calls per captured graph, device events over trains of {REPLAYS * PER_GRAPH} calls, {ROUNDS} rounds "
                    "alternated; microseconds per call, median of the trains and their spread (max - min)",
            "mean_length_spread": round(float(spread.float().mean()), 1), **res}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_lengths_xgrad_c2.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
