#!/usr/bin/env python3
"""BandNorm behind the mel layers (dmel_amd.BandNorm: row statistics, band combine, apply, forward and backward) against what a user has
without it -- the masked restatement of tests/bandnorm_cases.py as torch launches on the device, and at full lengths nn.BatchNorm2d on
s.transpose(1, 2) -- at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
with full lengths (frame_lengths=None) and mixed lengths (clip 0 full, the last a third, the rest random), both statistics.
Forward (no gradient) and forward + backward to ds, dweight and dbias.  Device events over five alternated trains per variant (200 calls of
the module, 20 of the torch formulations per train), every call on warmed shapes; and the launches alone through the C ABI, 20 per graph
replay (``launch_fwd``, ``launch_bwd``: what the device spends, without the host's share of an eager call).  Also the bytes a call must move at
full lengths (forward: s twice -- statistics, apply -- and y; backward: g and s twice and ds; the row partials) over its time.  Prints one
JSON line and, with ``--out FILE``, writes it to FILE as well (the file committed under profiles/).  Nothing about time is asserted: the
figures are recorded."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # the torch restatement is the tests' (tests/bandnorm_cases.py): one copy
import bandnorm_cases as N  # noqa: E402
from dmel_amd import BandNorm, capi  # noqa: E402
from _stage_timing import ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]


def _masked_torch(s, w, b, mask, n, dims):
    """bandnorm_cases.forward's arithmetic on device tensors (the mask and the counts prepared once, outside the timed call)"""
    zero = torch.zeros((), device=s.device)
    pivot = (s[..., :1] if dims == (3,) else s[:1, :1, :, :1]).detach()
    d = s - pivot
    c = d - torch.where(mask, d, zero).sum(dim=dims, keepdim=True) / n
    var = (torch.where(mask, c, zero) ** 2).sum(dim=dims, keepdim=True) / n
    return torch.where(mask, c / torch.sqrt(var + N.EPS) * w.reshape(1, 1, -1, 1) + b.reshape(1, 1, -1, 1), zero)


def main():
    assert torch.cuda.is_available(), "tools/bandnorm_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shapes": {}}
    for shape in SHAPES:
        B, C, M, T = shape
        gen = torch.Generator(DEV).manual_seed(0)
        E = torch.rand(shape, device=DEV, generator=gen) ** 4 * 10.0 ** (-6 + 8 * torch.rand(shape[:-1] + (1,), device=DEV, generator=gen))
        s = torch.log(E + 1e-10).contiguous()
        g = torch.randn(shape, device=DEV, generator=gen)
        w, b, _, _ = (p.to(DEV) for p in N.params(M, 7))
        rows, n = B * C * M, s.numel()
        for stats in ("clip", "batch"):
            for lengths_name in ("full", "mixed"):
                Tc = None if lengths_name == "full" else N.frame_lengths(shape, 1).to(DEV)
                mod = BandNorm(M, stats=stats).to(DEV)
                with torch.no_grad():
                    mod.weight.copy_(w), mod.bias.copy_(b)
                sg = s.clone().requires_grad_(True)
                prm = list(mod.parameters())
                mask = N.valid_mask(shape, None if Tc is None else Tc.cpu()).to(DEV)
                per_clip = (torch.full((B,), T, device=DEV) if Tc is None else Tc).float().reshape(B, 1, 1, 1)
                dims, cnt = ((3,), per_clip) if stats == "clip" else ((0, 1, 3), (C * per_clip.sum()).reshape(1, 1, 1, 1))
                wt, bt = w.clone().requires_grad_(True), b.clone().requires_grad_(True)

                def k_fwd():
                    with torch.no_grad():
                        return mod(s, Tc)

                def k_fwd_bwd():
                    return torch.autograd.grad(mod(sg, Tc), [sg] + prm, g)

                def t_fwd():
                    with torch.no_grad():
                        return _masked_torch(s, w, b, mask, cnt, dims)

                def t_fwd_bwd():
                    return torch.autograd.grad(_masked_torch(sg, wt, bt, mask, cnt, dims), [sg, wt, bt], g)

                # the launches alone, through the C ABI on static buffers, 20 per graph replay
                lens = None if Tc is None else Tc.to(torch.int32)
                y_, ds_ = torch.empty_like(s), torch.empty_like(s)
                dw_, db_ = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
                st_ = torch.empty((M if stats == "batch" else rows, 2), dtype=torch.float64, device=DEV)
                sc_ = torch.empty(capi.bandnorm_scratch_bytes(rows, M) // 8, dtype=torch.float64, device=DEV)
                rm_, rv_ = torch.zeros(M, device=DEV), torch.ones(M, device=DEV)
                nbt_ = torch.zeros((), dtype=torch.int64, device=DEV)
                batch = stats == "batch"
                ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731

                def c_fwd():
                    capi.bandnorm_forward(s.data_ptr(), rows, M, C * M, T, ptr(lens), w.data_ptr(), b.data_ptr(), batch, True, N.EPS, N.MOMENTUM,
                                          ptr(rm_) if batch else None, ptr(rv_) if batch else None, ptr(nbt_) if batch else None, y_.data_ptr(),
                                          st_.data_ptr(), sc_.data_ptr(), torch.cuda.current_stream().cuda_stream)

                def c_bwd():
                    capi.bandnorm_backward(g.data_ptr(), s.data_ptr(), st_.data_ptr(), rows, M, C * M, T, ptr(lens), w.data_ptr(), batch, True,
                                           ds_.data_ptr(), dw_.data_ptr(), db_.data_ptr(), sc_.data_ptr(), torch.cuda.current_stream().cuda_stream)

                c_fwd()
                variants = {"kernel_fwd": (k_fwd, 200), "kernel_fwd_bwd": (k_fwd_bwd, 200), "torch_masked_fwd": (t_fwd, 20),
                            "torch_masked_fwd_bwd": (t_fwd_bwd, 20), "launch_fwd_x20": (_graphed(c_fwd), 50), "launch_bwd_x20": (_graphed(c_bwd), 50)}
                # the comparison is like for like (the tests hold the kernels to fp64; this is a check of the tool)
                yk, yt = k_fwd(), t_fwd()
                gk, gt = k_fwd_bwd(), t_fwd_bwd()
                agree = {"y": float((yk - yt).abs().max() / yt.abs().max())}
                for name, a_, b_ in zip(("ds", "dweight", "dbias"), gk, gt):
                    agree[name] = float((a_ - b_).abs().max() / b_.abs().max())
                if stats == "batch" and Tc is None:
                    bn = torch.nn.BatchNorm2d(M).to(DEV)
                    with torch.no_grad():
                        bn.weight.copy_(w), bn.bias.copy_(b)
                    bprm = list(bn.parameters())

                    def b_fwd():
                        with torch.no_grad():
                            return bn(s.transpose(1, 2)).transpose(1, 2)

                    def b_fwd_bwd():
                        return torch.autograd.grad(bn(sg.transpose(1, 2)).transpose(1, 2), [sg] + bprm, g)

                    variants.update(batchnorm2d_fwd=(b_fwd, 200), batchnorm2d_fwd_bwd=(b_fwd_bwd, 200))
                    agree["y_vs_batchnorm2d"] = float((yk - b_fwd()).abs().max() / yt.abs().max())
                times = _alternated(variants)
                for k in ("launch_fwd_x20", "launch_bwd_x20"):             # per call (its two or three launches)
                    times[k[:-4]] = [t / 20 for t in times.pop(k)]
                med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
                out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
                out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
                out["torch_masked_over_kernel_fwd"] = round(med["torch_masked_fwd"] / med["kernel_fwd"], 1)
                out["torch_masked_over_kernel_fwd_bwd"] = round(med["torch_masked_fwd_bwd"] / med["kernel_fwd_bwd"], 1)
                if "batchnorm2d_fwd" in med:
                    out["batchnorm2d_over_kernel_fwd"] = round(med["batchnorm2d_fwd"] / med["kernel_fwd"], 2)
                    out["batchnorm2d_over_kernel_fwd_bwd"] = round(med["batchnorm2d_fwd_bwd"] / med["kernel_fwd_bwd"], 2)
                if Tc is None:
                    bytes_fwd = 4 * n * 3 + 16 * rows                       # s twice, y; the (mu, rstd) pairs or row partials
                    bytes_bwd = 4 * n * 5 + 16 * rows * 2                   # g and s twice, ds; row partials out and in
                    out["bytes_fwd"], out["bytes_bwd"] = bytes_fwd, bytes_bwd
                    out["launch_gb_per_s_fwd"] = round(bytes_fwd / med["launch_fwd"] * 1e-3, 1)
                    out["launch_gb_per_s_bwd"] = round(bytes_bwd / med["launch_bwd"] * 1e-3, 1)
                else:
                    out["valid_fraction"] = round(float(Tc.sum()) / (B * T), 3)
                out["max_rel_difference_kernel_vs_torch"] = {k: float(f"{v:.3e}") for k, v in agree.items()}
                res["shapes"].setdefault("x".join(str(v) for v in shape), {})[f"{stats}_{lengths_name}"] = out
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
