#!/usr/bin/env python3
"""PCEN behind the mel layers (dmel_amd.PCEN: dmel_pcen_fwd_kernel, dmel_pcen_bwd_kernel + the reduction of the parameter gradients) against
what a user has without it -- the same formulas as T sequential torch launches on the device -- at
  (256, 1, 128, 32)    BASELINE config 2's image: the headline shape
  (64, 1, 128, 501)    five-second clips at hop 160
Forward (no gradient) and forward + backward to dE and the four parameter gradients.  Device events over five alternated trains per
variant (200 calls of the module, 5 of the torch formulation per train), every call on warmed shapes; and the launches alone through the C
ABI, 20 per graph replay (``launch_fwd``, ``launch_bwd``: what the device spends, without the host's share of an eager call).  Also the bytes each kernel call
must move (computed from the shapes: forward reads E, writes y and M; backward reads g, E and M (M[t-1] from the line that brought M[t]), writes dE and the row
partials) over its time.  Prints one JSON line and, with ``--out FILE``, writes it to FILE as well (the file committed under profiles/).
There is no bar beyond the kernels being faster than the torch formulation at both shapes: the figures are recorded."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # the torch restatement of the formulas is the tests' (tests/pcen_cases.py): one copy
import pcen_cases as P  # noqa: E402
from dmel_amd import PCEN  # noqa: E402
from _stage_timing import ROUNDS, _alternated, _graphed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 1, 128, 32), (64, 1, 128, 501)]


def main():
    assert torch.cuda.is_available(), "tools/pcen_time.py measures on the GPU: there is no other way to get these figures"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shapes": {}}
    for shape in SHAPES:
        n_mels, T = shape[-2], shape[-1]
        gen = torch.Generator(DEV).manual_seed(0)
        E = (torch.rand(shape, device=DEV, generator=gen) ** 4 * 10.0 ** (-6 + 8 * torch.rand(shape[:-1] + (1,), device=DEV, generator=gen))).contiguous()
        g = torch.randn(shape, device=DEV, generator=gen)
        mod = PCEN(n_mels).to(DEV)
        with torch.no_grad():
            for p, v in zip(mod.parameters(), P.params(n_mels, 7)):
                p.copy_(v)
            mod.alpha[0], mod.delta[0], mod.r[0], mod.s[0] = 0.9, 1.0, 0.5, 0.05
        prm = list(mod.parameters())
        Eg = E.clone().requires_grad_(True)

        def k_fwd():
            with torch.no_grad():
                return mod(E)

        def k_fwd_bwd():
            return torch.autograd.grad(mod(Eg), [Eg] + prm, g)

        def t_fwd():
            with torch.no_grad():
                return P.forward(E, *prm, eps=mod.eps)[0]

        def t_fwd_bwd():
            return torch.autograd.grad(P.forward(Eg, *prm, eps=mod.eps)[0], [Eg] + prm, g)

        # the launches alone, through the C ABI on static buffers, 20 per graph replay
        from dmel_amd import capi
        rows_ = E.numel() // T
        y_, M_, dE_ = torch.empty_like(E), torch.empty_like(E), torch.empty_like(E)
        dp_ = torch.empty(4, n_mels, device=DEV)
        sc_ = torch.empty(capi.pcen_scratch_bytes(rows_) // 4, device=DEV)
        pp = [p.data_ptr() for p in prm]

        def c_fwd():
            capi.pcen_forward(E.data_ptr(), rows_, n_mels, T, *pp, mod.eps, y_.data_ptr(), M_.data_ptr(), torch.cuda.current_stream().cuda_stream)

        def c_bwd():
            capi.pcen_backward(g.data_ptr(), E.data_ptr(), M_.data_ptr(), rows_, n_mels, T, *pp, mod.eps, dE_.data_ptr(), dp_.data_ptr(), sc_.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)

        c_fwd()
        g_fwd, g_bwd = _graphed(c_fwd), _graphed(c_bwd)

        # the two compute the same thing (the tests hold the kernels to fp64; this is a check that the comparison is like for like)
        yk, yt = k_fwd(), t_fwd()
        gk, gt = k_fwd_bwd(), t_fwd_bwd()
        agree = {"y": float((yk - yt).abs().max() / yt.abs().max())}
        for name, a, b in zip(("dE", "dalpha", "ddelta", "dr", "ds"), gk, gt):
            agree[name] = float((a - b).abs().max() / b.abs().max())
        times = _alternated({"kernel_fwd": (k_fwd, 200), "kernel_fwd_bwd": (k_fwd_bwd, 200), "torch_fwd": (t_fwd, 5), "torch_fwd_bwd": (t_fwd_bwd, 5),
                             "launch_fwd_x20": (g_fwd, 50), "launch_bwd_x20": (g_bwd, 50)})
        for k in ("launch_fwd_x20", "launch_bwd_x20"):             # per launch (the backward: its two launches)
            times[k[:-4]] = [t / 20 for t in times.pop(k)]
        med = {k: sorted(v)[ROUNDS // 2] for k, v in times.items()}
        n = E.numel()
        rows = n // T
        bytes_fwd = 4 * n * 3                                   # E in, y and M out
        bytes_bwd = 4 * n * 4 + 16 * rows                       # g, E, M in (M[t-1] comes from the line M[t] brought), dE out, row partials
        out = {k + "_us": [round(t, 2) for t in v] for k, v in times.items()}
        out.update({k + "_median_us": round(v, 2) for k, v in med.items()})
        out["torch_over_kernel_fwd"] = round(med["torch_fwd"] / med["kernel_fwd"], 1)
        out["torch_over_kernel_fwd_bwd"] = round(med["torch_fwd_bwd"] / med["kernel_fwd_bwd"], 1)
        out["bytes_fwd"], out["bytes_fwd_bwd"] = bytes_fwd, bytes_fwd + bytes_bwd
        out["bytes_per_element_fwd"], out["bytes_per_element_bwd"] = round(bytes_fwd / n, 2), round(bytes_bwd / n, 2)
        # a call's time holds its launches and the module's host work, not only the kernels: a rate of the call, not of a kernel
        out["call_gb_per_s_fwd"] = round(bytes_fwd / med["kernel_fwd"] * 1e-3, 1)
        out["call_gb_per_s_fwd_bwd"] = round((bytes_fwd + bytes_bwd) / med["kernel_fwd_bwd"] * 1e-3, 1)
        out["launch_gb_per_s_fwd"] = round(bytes_fwd / med["launch_fwd"] * 1e-3, 1)
        out["launch_gb_per_s_bwd"] = round(bytes_bwd / med["launch_bwd"] * 1e-3, 1)
        out["max_rel_difference_kernel_vs_torch"] = {k: float(f"{v:.3e}") for k, v in agree.items()}
        res["shapes"]["x".join(str(v) for v in shape)] = out
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
