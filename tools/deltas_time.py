#!/usr/bin/env python3
"""Deltas behind the mel layers (dmel_amd.Deltas, win_length 5, order 2, with the static group: one read, three writes) against (a) a
``copy_`` of the output's bytes -- the traffic yardstick: three reads and three writes of the image -- and (b) the masked torch restatement
a user would write today (a gather with clamped indices, a convolution and a ``where`` per order, a ``cat``), forward and forward + backward, at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
fp32, full lengths (frame_lengths=None) and mixed lengths (int64, narrowed by two torch launches).  Device events over five alternated trains
per variant (200 calls per train, 50 of the torch restatement with its backward), every call on warmed shapes; and the launches alone
through the C ABI, 20 per graph replay (``launch_fwd``, ``launch_bwd``, ``launch_copy``: what the device spends, without the host's share of an
eager call).  Prints one JSON line and, with ``--out FILE``, writes it to FILE as well (the file committed under profiles/).  Nothing about
time is asserted: the figures are recorded."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import Deltas, capi  # noqa: E402
from _stage_timing import ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]
WIN, ORDER = 5, 2


class MaskedTorchDeltas(torch.nn.Module):
    """what a user writes for a zero-padded batch: the row extended by n frames on either side through a gather with indices clamped to
    0 ... Tc - 1, a convolution with arange(-n, n + 1) / denom, a where for the pad frames -- once per order -- and a cat"""

    def __init__(self, win_length):
        super().__init__()
        n = (win_length - 1) // 2
        self.n = n
        self.register_buffer("kernel", (torch.arange(-n, n + 1, dtype=torch.float32) / (n * (n + 1) * (2 * n + 1) // 3)).reshape(1, 1, -1))

    def forward(self, s, Tc):
        B, C, M, T = s.shape
        n = self.n
        if Tc is None:
            Tc = torch.full((B,), T, dtype=torch.int64, device=s.device)
        last = (Tc.to(torch.int64) - 1).reshape(B, 1)
        idx = torch.minimum(torch.arange(-n, T + n, device=s.device).clamp(min=0).reshape(1, -1), last)              # (B, T + 2 n)
        idx = idx.reshape(B, 1, 1, T + 2 * n).expand(B, C, M, T + 2 * n)
        valid = (torch.arange(T, device=s.device).reshape(1, T) <= last).reshape(B, 1, 1, T)
        zero = torch.zeros((), dtype=s.dtype, device=s.device)

        def once(x):
            ext = torch.gather(x, 3, idx).reshape(B * C * M, 1, T + 2 * n)
            return torch.where(valid, F.conv1d(ext, self.kernel).reshape(B, C, M, T), zero)

        d = once(s)
        return torch.cat([s, d, once(d)], dim=1)


def main():
    assert torch.cuda.is_available(), "tools/deltas_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "win_length": WIN, "order": ORDER, "include_static": True, "shapes": {}}
    for shape in SHAPES:
        B, C, M, T = shape
        gen = torch.Generator(DEV).manual_seed(0)
        s = torch.randn(shape, device=DEV, generator=gen)
        g = torch.randn((B, 3 * C, M, T), device=DEV, generator=gen)
        rows, n = B * C * M, s.numel()
        for lengths_name in ("full", "mixed"):
            Tc = None
            if lengths_name == "mixed":
                Tc = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(1))
                Tc[0], Tc[-1] = T, max(1, T // 3)
                Tc = Tc.to(DEV)
            mod = Deltas(WIN, ORDER, True)
            ref = MaskedTorchDeltas(WIN).to(DEV)
            sg = s.clone().requires_grad_(True)
            y_, ds_ = torch.empty_like(g), torch.empty_like(s)
            assert torch.allclose(mod(s, Tc), ref(s, Tc), rtol=0, atol=1e-4)                # the two compute the same thing

            def k_fwd():
                with torch.no_grad():
                    return mod(s, Tc)

            def k_fwd_bwd():
                return torch.autograd.grad(mod(sg, Tc), [sg], g)

            def t_fwd():
                with torch.no_grad():
                    return ref(s, Tc)

            def t_fwd_bwd():
                return torch.autograd.grad(ref(sg, Tc), [sg], g)

            def copy():
                return y_.copy_(g)

            # the launches alone, through the C ABI on static buffers, 20 per graph replay
            lens = None if Tc is None else Tc.to(torch.int32)
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731

            def c_fwd():
                capi.deltas_forward(s.data_ptr(), rows, C * M, T, ptr(lens), WIN, ORDER, True, y_.data_ptr(), torch.cuda.current_stream().cuda_stream)

            def c_bwd():
                capi.deltas_backward(g.data_ptr(), rows, C * M, T, ptr(lens), WIN, ORDER, True, ds_.data_ptr(), torch.cuda.current_stream().cuda_stream)

            variants = {"kernel_fwd": (k_fwd, 200), "kernel_fwd_bwd": (k_fwd_bwd, 200), "copy": (copy, 200), "masked_torch_fwd": (t_fwd, 200),
                        "masked_torch_fwd_bwd": (t_fwd_bwd, 50), "launch_fwd_x20": (_graphed(c_fwd), 50), "launch_bwd_x20": (_graphed(c_bwd), 50),
                        "launch_copy_x20": (_graphed(copy), 50)}
            times = _alternated(variants)
            for k in [k for k in times if k.endswith("_x20")]:                     # per call
                times[k[:-4]] = [t / 20 for t in times.pop(k)]
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
            out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
            out["launch_fwd_over_copy"] = round(med["launch_fwd"] / med["launch_copy"], 2)
            out["launch_bwd_over_copy"] = round(med["launch_bwd"] / med["launch_copy"], 2)
            out["masked_torch_over_kernel_fwd"] = round(med["masked_torch_fwd"] / med["kernel_fwd"], 2)
            out["masked_torch_over_kernel_fwd_bwd"] = round(med["masked_torch_fwd_bwd"] / med["kernel_fwd_bwd"], 2)
            out["bytes_moved"] = 16 * n                                            # s in, three groups out (the backward: three in, ds out)
            out["copy_bytes_moved"] = 24 * n                                       # three groups in, three out
            out["launch_gb_per_s_fwd"] = round(16 * n / med["launch_fwd"] * 1e-3, 1)
            out["launch_gb_per_s_bwd"] = round(16 * n / med["launch_bwd"] * 1e-3, 1)
            out["launch_gb_per_s_copy"] = round(24 * n / med["launch_copy"] * 1e-3, 1)
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
