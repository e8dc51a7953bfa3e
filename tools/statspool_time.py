#!/usr/bin/env python3
"""StatsPool behind the mel layers (dmel_amd.StatsPool, mean + std + max: one read of the image, 3 values per row out; the backward reads
the image once more and writes ds) against (a) ``s.sum(-1)`` on the same tensor -- the floor of one read --, (b) the masked torch restatement
a user would write today (a mask, three ``where``, three reductions, a ``cat``) and (c) BandNorm's clip-statistics forward from its own file
(the same two-pass row moments, plus an apply launch that reads the image again and writes it), at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
fp32, full lengths (frame_lengths=None) and mixed lengths.  Every variant is replayed from a graph of 20 calls on static buffers (what the
device spends, without the host's share of an eager call): device events over five alternated trains per variant, 50 replays per train,
every shape warmed; medians are reported.  Prints one JSON line and, with ``--out FILE``, writes it to FILE as well (the file committed
under profiles/).  Nothing about time is asserted: the figures are recorded."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import StatsPool, capi  # noqa: E402
from _stage_timing import PER_GRAPH, ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]
EPS = 1e-5


def masked_torch(s, Tc, eps=EPS):
    """what a user writes for a zero-padded batch: a (B, 1, 1, T) mask, the masked mean, the masked squared deviations, the masked maximum"""
    B, C, M, T = s.shape
    if Tc is None:
        Tc = torch.full((B,), T, dtype=torch.int64, device=s.device)
    valid = (torch.arange(T, device=s.device).reshape(1, T) < Tc.reshape(B, 1)).reshape(B, 1, 1, T)
    n = Tc.reshape(B, 1, 1).to(s.dtype)
    zero = torch.zeros((), dtype=s.dtype, device=s.device)
    mu = torch.where(valid, s, zero).sum(-1) / n
    d = torch.where(valid, s - mu.unsqueeze(-1), zero)
    sd = torch.sqrt((d * d).sum(-1) / n + eps)
    mx = torch.where(valid, s, torch.full((), float("-inf"), dtype=s.dtype, device=s.device)).amax(-1)
    return torch.cat([mu, sd, mx], dim=1)


def main():
    assert torch.cuda.is_available(), "tools/statspool_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "per_graph": PER_GRAPH, "stats": ["mean", "std", "max"], "eps": EPS, "shapes": {}}
    for shape in SHAPES:
        B, C, M, T = shape
        gen = torch.Generator(DEV).manual_seed(0)
        s = torch.randn(shape, device=DEV, generator=gen)
        g = torch.randn((B, 3 * C, M), device=DEV, generator=gen)
        rows, n = B * C * M, s.numel()
        for lengths_name in ("full", "mixed"):
            Tc = None
            if lengths_name == "mixed":
                Tc = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(1))
                Tc[0], Tc[-1] = T, max(1, T // 3)
                Tc = Tc.to(DEV)
            frames = n if Tc is None else int(Tc.sum()) * C * M          # valid elements: what the kernels load
            got, want = StatsPool(eps=EPS)(s, Tc), masked_torch(s, Tc)
            assert torch.allclose(got[:, :2 * C], want[:, :2 * C], rtol=0, atol=1e-4) and torch.equal(got[:, 2 * C:], want[:, 2 * C:])     # the two compute the same thing
            y_, ds_, sum_, bn_ = torch.empty_like(g), torch.empty_like(s), torch.empty((B, C, M), device=DEV), torch.empty_like(s)
            stats_, am_ = torch.empty((rows, 2), dtype=torch.float64, device=DEV), torch.empty((rows,), dtype=torch.int32, device=DEV)
            bn_stats_ = torch.empty((rows, 2), dtype=torch.float64, device=DEV)
            lens = None if Tc is None else Tc.to(torch.int32)
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731

            def c_fwd():
                capi.statspool_forward(s.data_ptr(), rows, C * M, T, ptr(lens), 7, EPS, y_.data_ptr(), stats_.data_ptr(), am_.data_ptr(), stream())

            def c_bwd():
                capi.statspool_backward(g.data_ptr(), s.data_ptr(), stats_.data_ptr(), am_.data_ptr(), rows, C * M, T, ptr(lens), 7, ds_.data_ptr(), stream())

            def c_bandnorm():
                capi.bandnorm_forward(s.data_ptr(), rows, M, C * M, T, ptr(lens), None, None, False, True, EPS, 0.1, None, None, None, bn_.data_ptr(),
                                      bn_stats_.data_ptr(), None, stream())

            def t_sum():
                return torch.sum(s, -1, out=sum_)

            def t_masked():
                with torch.no_grad():
                    return masked_torch(s, Tc)

            c_fwd()                                                # (the backward reads what a forward wrote)
            variants = {"launch_fwd_x20": (_graphed(c_fwd), 50), "launch_bwd_x20": (_graphed(c_bwd), 50), "sum_x20": (_graphed(t_sum), 50),
                        "masked_torch_fwd_x20": (_graphed(t_masked), 50), "bandnorm_clip_fwd_x20": (_graphed(c_bandnorm), 50)}
            times = _alternated(variants)
            times = {k[:-4]: [t / PER_GRAPH for t in v] for k, v in times.items()}         # per call
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
            out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
            out["launch_fwd_over_sum"] = round(med["launch_fwd"] / med["sum"], 2)
            out["launch_bwd_over_sum"] = round(med["launch_bwd"] / med["sum"], 2)
            out["masked_torch_over_launch_fwd"] = round(med["masked_torch_fwd"] / med["launch_fwd"], 2)
            out["bandnorm_clip_fwd_over_launch_fwd"] = round(med["bandnorm_clip_fwd"] / med["launch_fwd"], 2)
            out["valid_elements"], out["elements"] = frames, n
            out["launch_gb_per_s_fwd"] = round(4 * frames / med["launch_fwd"] * 1e-3, 1)             # s in, once (the second pass comes from the cache)
            out["launch_gb_per_s_bwd"] = round((4 * frames + 4 * n) / med["launch_bwd"] * 1e-3, 1)   # s in on valid frames, ds out on every frame
            out["gb_per_s_sum"] = round(4 * n / med["sum"] * 1e-3, 1)
            res["shapes"].setdefault("x".join(str(v) for v in shape), {})[lengths_name] = out
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
