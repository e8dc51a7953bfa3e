"""Host time of the eager layer for two versions of the Python host code (layer.py, capi.py) on the same shared objects.

    python tools/layer_host_time.py --package OLD_PKG_DIR --package differentiable-mel-spectrogram_amd [--rounds 5] [--calls 2000]
    python tools/layer_host_time.py --package PKG --lib-dir OLD_LIB_DIR --package PKG --lib-dir NEW_LIB_DIR

The packages are imported as ``tools/layer_digests.py`` does, alternating, each round in a fresh child process with a time limit.  A child
times three loops at the digest shapes (3 clips of 2000 samples, 16 mel bands, hop 100, lambd 40, log on, fp32): ``layer(x)`` under
``torch.no_grad()``; a training step without a graph (forward, ``out.sum().backward()``, ``lambd.grad = None``) on the hot path; the same
step with ``x.requires_grad`` (the tracked path through a Python autograd Function).  Wall time over one train of ``--calls`` calls, one
``torch.cuda.synchronize()`` before and after it.  The first package is the yardstick: the report gives both medians per loop and the
first package's own min-to-max spread over its rounds, and says whether the second median exceeds the first by more than that spread.
``--lib-dir`` may repeat, paired with ``--package`` in order, to time two builds of the shared objects under the same Python files.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from layer_digests import B, DEFAULT_PKG, HOP, M, N, SR, import_package, pair_lib_dirs  # noqa: E402

LOOPS = ("no_grad", "train_step", "train_step_xgrad")


def child(pkg_dir, lib_dir, calls):
    import torch
    dm = import_package(pkg_dir, lib_dir)
    dev = torch.device("cuda", 0)
    layer = dm.MelSpectrogramLayer(40.0, M, N, SR, hop_length=HOP, optimized=True, log=True).to(dev)
    x = torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(dev)
    xg = x.clone().requires_grad_(True)

    def infer():
        with torch.no_grad():
            layer(x)

    def step(inp):
        layer(inp).sum().backward()
        layer.lambd.grad = None
        inp.grad = None

    result = {}
    for name, fn in zip(LOOPS, (infer, lambda: step(x), lambda: step(xg))):
        for _ in range(max(calls // 10, 20)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        result[name] = (time.perf_counter() - t0) / calls * 1e6
    assert layer.lambd_status()["error"] == 0
    print("TIMES " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--package", action="append", help="package directory to import as dmel_amd (give two: yardstick, candidate)")
    ap.add_argument("--lib-dir", action="append", help="one for all packages, or one per package")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--timeout", type=float, default=120.0, help="time limit of one child, seconds")
    ap.add_argument("--out", help="also write the report (JSON) here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    packages = args.package or [DEFAULT_PKG]
    lib_dirs = pair_lib_dirs(ap, packages, args.lib_dir)
    if args.child:
        child(packages[0], lib_dirs[0], args.calls)
        return 0
    times = [{k: [] for k in LOOPS} for _ in packages]           # (by position: the same package may be given twice)
    for _ in range(args.rounds):
        for i, (pkg, lib_dir) in enumerate(zip(packages, lib_dirs)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package", pkg, "--lib-dir", lib_dir, "--calls", str(args.calls)]
            try:
                res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{pkg}: no result after {args.timeout:g} s, stopping", flush=True)
                return 2
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("TIMES ")]
            if res.returncode != 0 or not line:
                print(res.stdout[-2000:])
                print(f"{pkg}: the child ended with status {res.returncode}, stopping", flush=True)
                return 2
            for k, v in json.loads(line[0][6:]).items():
                times[i][k].append(v)
            print(pkg, lib_dir, line[0], flush=True)
    report = {"unit": "us per call", "calls": args.calls, "rounds": args.rounds, "loops": {}}
    for k in LOOPS:
        entry = {"yardstick_median": statistics.median(times[0][k]), "yardstick_spread": max(times[0][k]) - min(times[0][k]),
                 "yardstick_runs": times[0][k]}
        for cand in times[1:]:
            entry["candidate_median"] = statistics.median(cand[k])
            entry["candidate_runs"] = cand[k]
            entry["within_spread"] = entry["candidate_median"] <= entry["yardstick_median"] + entry["yardstick_spread"]
        report["loops"][k] = entry
    text = json.dumps(report, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 0 if all(e.get("within_spread", True) for e in report["loops"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
