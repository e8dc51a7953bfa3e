#!/usr/bin/env python3
"""SpecMask behind the mel layers (dmel_amd.SpecMask: draw, apply; the backward is the apply on the cotangent) against (a) ``y.copy_(s)`` on
the same tensor -- the traffic floor: the stage moves the same bytes -- and (b) the ``panns._IidAxisMask`` pair (time, then frequency), what a
user has without it, forward and forward + backward, at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
fp32, one time and one frequency stripe (64 / 8), full lengths (frame_lengths=None) and mixed lengths (int64, narrowed by two torch launches).
Device events over five alternated trains per variant (200 calls per train, 20 of the torch pair with its backward), every call on warmed
shapes; and the launches alone through the C ABI, 20 per graph replay (``launch_draw``, ``launch_apply``, ``launch_fwd`` = draw + apply,
``launch_bwd`` = apply on the cotangent, ``launch_copy``: what the device spends, without the host's share of an eager call).  Prints one JSON
line and, with ``--out FILE``, writes it to FILE as well (the file committed under profiles/).  Nothing about time is asserted: the figures are
recorded."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmel_amd import SpecMask, capi  # noqa: E402
from dmel_amd.panns import _IidAxisMask  # noqa: E402
from _stage_timing import ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]
TIME_PARAM, FREQ_PARAM = 64, 8


def main():
    assert torch.cuda.is_available(), "tools/specmask_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "time_param": TIME_PARAM, "freq_param": FREQ_PARAM, "shapes": {}}
    for shape in SHAPES:
        B, C, M, T = shape
        gen = torch.Generator(DEV).manual_seed(0)
        s = torch.randn(shape, device=DEV, generator=gen)
        g = torch.randn(shape, device=DEV, generator=gen)
        rows, n = B * C * M, s.numel()
        for lengths_name in ("full", "mixed"):
            Tc = None
            if lengths_name == "mixed":
                Tc = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(1))
                Tc[0], Tc[-1] = T, max(1, T // 3)
                Tc = Tc.to(DEV)
            mod = SpecMask(TIME_PARAM, FREQ_PARAM, seed=1).to(DEV)
            pair = (_IidAxisMask(TIME_PARAM, axis=3), _IidAxisMask(FREQ_PARAM, axis=2))
            sg = s.clone().requires_grad_(True)
            y_ = torch.empty_like(s)

            def k_fwd():
                with torch.no_grad():
                    return mod(s, Tc)

            def k_fwd_bwd():
                return torch.autograd.grad(mod(sg, Tc), [sg], g)

            def t_fwd():
                with torch.no_grad():
                    return pair[1](pair[0](s))

            def t_fwd_bwd():
                return torch.autograd.grad(pair[1](pair[0](sg)), [sg], g)

            def copy():
                return y_.copy_(s)

            # the launches alone, through the C ABI on static buffers, 20 per graph replay
            lens = None if Tc is None else Tc.to(torch.int32)
            ds_ = torch.empty_like(s)
            tab_ = torch.zeros((B * C, 2, 2), dtype=torch.int32, device=DEV)
            state_ = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731

            def c_draw():
                capi.specmask_draw(B * C, C, M, T, ptr(lens), TIME_PARAM, 1000, 1, FREQ_PARAM, 1, state_.data_ptr(), True, tab_.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)

            def c_apply():
                capi.specmask_apply(s.data_ptr(), rows, M, C * M, T, ptr(lens), tab_.data_ptr(), 1, 1, False, 0.0, y_.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)

            def c_fwd():
                c_draw(), c_apply()

            def c_bwd():
                capi.specmask_apply(g.data_ptr(), rows, M, C * M, T, ptr(lens), tab_.data_ptr(), 1, 1, False, 0.0, ds_.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)

            variants = {"kernel_fwd": (k_fwd, 200), "kernel_fwd_bwd": (k_fwd_bwd, 200), "copy": (copy, 200), "iid_axis_mask_fwd": (t_fwd, 200),
                        "iid_axis_mask_fwd_bwd": (t_fwd_bwd, 20), "launch_draw_x20": (_graphed(c_draw), 50), "launch_apply_x20": (_graphed(c_apply), 50),
                        "launch_fwd_x20": (_graphed(c_fwd), 50), "launch_bwd_x20": (_graphed(c_bwd), 50), "launch_copy_x20": (_graphed(copy), 50)}
            times = _alternated(variants)
            for k in [k for k in times if k.endswith("_x20")]:                     # per call
                times[k[:-4]] = [t / 20 for t in times.pop(k)]
            med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
            out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
            out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
            out["launch_apply_over_copy"] = round(med["launch_apply"] / med["launch_copy"], 2)
            out["launch_fwd_over_copy"] = round(med["launch_fwd"] / med["launch_copy"], 2)
            out["iid_axis_mask_over_kernel_fwd"] = round(med["iid_axis_mask_fwd"] / med["kernel_fwd"], 2)
            out["iid_axis_mask_over_kernel_fwd_bwd"] = round(med["iid_axis_mask_fwd_bwd"] / med["kernel_fwd_bwd"], 2)
            out["bytes_moved"] = 8 * n                                             # s in, y out
            out["launch_gb_per_s_apply"] = round(8 * n / med["launch_apply"] * 1e-3, 1)
            out["launch_gb_per_s_copy"] = round(8 * n / med["launch_copy"] * 1e-3, 1)
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
