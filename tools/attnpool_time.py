#!/usr/bin/env python3
"""AttentivePool behind the mel layers (dmel_amd.AttentivePool, mean + std: the forward reads the image and the logits and writes 2 values
per row; the backward reads the image once more and writes ds and da) against (a) StatsPool's forward and backward with the same two
statistics on the same image -- the same row geometry with uniform weights: what the softmax costs on top, the forward's recomputed
exponentials among it -- and (b) the masked torch restatement a user would write today (a mask, a ``where`` to -inf, ``softmax``, two
weighted reductions, a ``cat``), at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
each with one attention per clip (A = 1) and one per band (A = 128), fp32, full lengths (frame_lengths=None) and mixed lengths.  Every variant
is replayed from a graph of 20 calls on static buffers (what the device spends, without the host's share of an eager call): device events
over five alternated trains per variant, 50 replays per train, every shape warmed; medians are reported.  Prints one JSON line and, with
``--out FILE``, writes it to FILE as well (the file committed under profiles/).  Nothing about time is asserted: the figures are recorded."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import AttentivePool, capi  # noqa: E402
from _stage_timing import PER_GRAPH, ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]
LOGIT_ROWS = [1, 128]
EPS = 1e-5


def masked_torch(s, a, Tc, eps=EPS):
    """what a user writes for a zero-padded batch: a (B, 1, T) mask, the logits at -inf behind it, softmax, the weighted mean and the
    weighted squared deviations"""
    B, C, M, T = s.shape
    A = a.shape[1]
    if Tc is None:
        Tc = torch.full((B,), T, dtype=torch.int64, device=s.device)
    valid = (torch.arange(T, device=s.device).reshape(1, T) < Tc.reshape(B, 1)).reshape(B, 1, T)
    w = torch.softmax(torch.where(valid, a, torch.full((), float("-inf"), dtype=a.dtype, device=a.device)), -1)
    w = w.unsqueeze(2).expand(B, A, C * M // A, T).reshape(B, C, M, T)
    x = torch.where(valid.unsqueeze(1), s, torch.zeros((), dtype=s.dtype, device=s.device))
    mu = (w * x).sum(-1)
    d = x - mu.unsqueeze(-1)
    sd = torch.sqrt((w * d * d).sum(-1) + eps)
    return torch.cat([mu, sd], dim=1)


def main():
    assert torch.cuda.is_available(), "tools/attnpool_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "per_graph": PER_GRAPH, "stats": ["mean", "std"], "eps": EPS, "shapes": {}}
    for shape in SHAPES:
        B, C, M, T = shape
        gen = torch.Generator(DEV).manual_seed(0)
        s = torch.randn(shape, device=DEV, generator=gen)
        g = torch.randn((B, 2 * C, M), device=DEV, generator=gen)
        rows, n = B * C * M, s.numel()
        for A in LOGIT_ROWS:
            a = 2.0 * torch.randn((B, A, T), device=DEV, generator=gen)
            for lengths_name in ("full", "mixed"):
                Tc = None
                if lengths_name == "mixed":
                    Tc = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(1))
                    Tc[0], Tc[-1] = T, max(1, T // 3)
                    Tc = Tc.to(DEV)
                frames = n if Tc is None else int(Tc.sum()) * C * M          # valid elements of s: what the kernels load
                logit_frames = frames // (C * M) * A
                got, want = AttentivePool(eps=EPS)(s, a, Tc), masked_torch(s, a, Tc)
                assert torch.allclose(got, want, rtol=0, atol=1e-4)           # the two compute the same thing
                y_, ds_, da_, sp_ds_ = torch.empty_like(g), torch.empty_like(s), torch.empty_like(a), torch.empty_like(s)
                stats_, norm_ = torch.empty((rows, 2), dtype=torch.float64, device=DEV), torch.empty((B * A, 2), dtype=torch.float64, device=DEV)
                sp_stats_ = torch.empty((rows, 2), dtype=torch.float64, device=DEV)
                lens = None if Tc is None else Tc.to(torch.int32)
                ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
                stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731

                def c_fwd():
                    capi.attnpool_forward(s.data_ptr(), a.data_ptr(), rows, C * M, A, T, ptr(lens), 3, EPS, y_.data_ptr(), stats_.data_ptr(),
                                          norm_.data_ptr(), stream())

                def c_bwd():
                    capi.attnpool_backward(g.data_ptr(), s.data_ptr(), a.data_ptr(), stats_.data_ptr(), norm_.data_ptr(), rows, C * M, A, T, ptr(lens), 3,
                                           EPS, ds_.data_ptr(), da_.data_ptr(), stream())

                def c_sp_fwd():
                    capi.statspool_forward(s.data_ptr(), rows, C * M, T, ptr(lens), 3, EPS, y_.data_ptr(), sp_stats_.data_ptr(), None, stream())

                def c_sp_bwd():
                    capi.statspool_backward(g.data_ptr(), s.data_ptr(), sp_stats_.data_ptr(), None, rows, C * M, T, ptr(lens), 3, sp_ds_.data_ptr(), stream())

                def t_masked():
                    with torch.no_grad():
                        return masked_torch(s, a, Tc)

                c_fwd(), c_sp_fwd()                                    # (the backwards read what a forward wrote)
                variants = {"launch_fwd_x20": (_graphed(c_fwd), 50), "launch_bwd_x20": (_graphed(c_bwd), 50),
                            "statspool_fwd_x20": (_graphed(c_sp_fwd), 50), "statspool_bwd_x20": (_graphed(c_sp_bwd), 50),
                            "masked_torch_fwd_x20": (_graphed(t_masked), 50)}
                times = _alternated(variants)
                times = {k[:-4]: [t / PER_GRAPH for t in v] for k, v in times.items()}         # per call
                med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
                out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
                out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
                out["launch_fwd_over_statspool_fwd"] = round(med["launch_fwd"] / med["statspool_fwd"], 2)
                out["launch_bwd_over_statspool_bwd"] = round(med["launch_bwd"] / med["statspool_bwd"], 2)
                out["masked_torch_over_launch_fwd"] = round(med["masked_torch_fwd"] / med["launch_fwd"], 2)
                out["valid_elements"], out["elements"], out["valid_logits"] = frames, n, logit_frames
                out["launch_gb_per_s_fwd"] = round(4 * (frames + logit_frames) / med["launch_fwd"] * 1e-3, 1)          # s and a in, once
                out["launch_gb_per_s_bwd"] = round(4 * (frames + logit_frames + n + a.numel()) / med["launch_bwd"] * 1e-3, 1)   # s and a in, ds and da out
                res["shapes"].setdefault("x".join(str(v) for v in shape), {}).setdefault(f"A{A}", {})[lengths_name] = out
    line = json.dumps(res, sort_keys=True)
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
