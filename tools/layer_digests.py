"""SHA-256 digests of what the Python layer returns, for comparing two versions of the host code (layer.py, capi.py) bit for bit.

    python tools/layer_digests.py --package OLD_PKG_DIR --package differentiable-mel-spectrogram_amd [--lib-dir DIR] [--out FILE]
    python tools/layer_digests.py --package PKG --lib-dir OLD_LIB_DIR --package PKG --lib-dir NEW_LIB_DIR

Every ``--package`` is a directory holding the package's Python files; each is imported as ``dmel_amd`` in a fresh child process (with a
time limit) and runs against the SAME shared objects: ``libdmel_hip.so`` / ``libdmel_torch.so`` of ``--lib-dir`` (default: the
repository's package directory; ``DMEL_LIB`` still overrides the first).  ``--lib-dir`` may repeat, once per ``--package`` and paired with
them in order: the same Python files then run against two builds of the libraries (two versions of the C++ host code).  A child prints one digest per tensor -- ``out``,
``lambd.grad`` and, where the path has one, ``x.grad`` / ``mel_fb.grad`` -- for seeded inputs (3 clips of 2000 samples, 16 mel bands, hop
100, 16 kHz; lambd 10 and 40; log on and off; fp32 and bf16 output) over every path of the four layer classes and ``dmel_log_mel``.  An
exception is digested as its type and message, so the refusals that need a device are compared too.  NaN rows are hashed like any other
bits.  With two packages the digests are compared: the last line is ``N digests, all equal`` or the list of differences (exit status 1).
"""
import argparse
import hashlib
import importlib
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_PKG = os.path.join(ROOT, "differentiable-mel-spectrogram_amd")
B, N, M, HOP, SR = 3, 2000, 16, 100, 16000


def import_package(pkg_dir, lib_dir):
    """``pkg_dir`` as ``dmel_amd``, bound to the shared objects in ``lib_dir``"""
    pkg_dir = os.path.abspath(pkg_dir)
    spec = importlib.util.spec_from_file_location("dmel_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["dmel_amd"] = mod
    spec.loader.exec_module(mod)
    capi = importlib.import_module("dmel_amd.capi")
    capi.LIB_PATH = os.environ.get("DMEL_LIB") or os.path.join(lib_dir, "libdmel_hip.so")
    capi.TORCH_LIB_PATH = os.path.join(lib_dir, "libdmel_torch.so")
    return mod


def digest(t):
    import torch
    t = t.detach().contiguous().cpu()
    h = hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode())
    h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def child(pkg_dir, lib_dir):
    import torch
    dm = import_package(pkg_dir, lib_dir)
    dev = torch.device("cuda", 0)
    seed = [0]

    def randn(*shape, dtype=torch.float32):
        seed[0] += 1
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed[0]), dtype=dtype).to(dev)

    def emit(name, what, value):
        print(f"DIGEST {name}/{what} {value}", flush=True)

    class Holder(torch.nn.Module):
        """the parameter of the functional form"""

        def __init__(self, lam):
            super().__init__()
            self.lambd = torch.nn.Parameter(torch.tensor(lam))

    def run(name, make, x=None, lengths=None, slot=False, call=None, move=True):
        """one forward and backward of the layer ``make()`` builds; ``x``: the input (default: a seeded fp32 batch)"""
        seed[0] = int(hashlib.sha256(name.encode()).hexdigest()[:6], 16)          # the same inputs whatever ran before
        try:
            layer = make().to(dev) if move else make()
            x = randn(B, N) if x is None else x()
            arg = x
            if slot:
                cell = torch.tensor([x.data_ptr()], dtype=torch.int64, device=dev)
                arg = dm.SlotInput(cell, x.shape)
            out = call(layer, arg) if call is not None else (layer(arg) if lengths is None else layer(arg, lengths()))
            emit(name, "out", digest(out))
            if out.requires_grad:
                (out.float() * randn(*out.shape)).sum().backward()
            for what, p in (("lambd.grad", getattr(layer, "lambd", None)), ("x.grad", x), ("mel_fb.grad", getattr(layer, "mel_fb", None))):
                if p is not None and p.grad is not None:
                    emit(name, what, digest(p.grad))
            torch.cuda.synchronize()
        except Exception as e:                                                     # noqa: BLE001 -- the refusal is the result
            if getattr(e, "status", None) == dm.capi.DMEL_ERR_HIP or "HIP error" in str(e) or "illegal memory access" in str(e):
                raise                                                              # a device error: nothing more runs on this GPU
            emit(name, "error", hashlib.sha256((type(e).__name__ + str(e)).encode()).hexdigest())

    def grad_x(dtype=torch.float32):
        return lambda: randn(B, N, dtype=dtype).requires_grad_(True)

    full = lambda: torch.tensor([2000, 129, 1], dtype=torch.int64, device=dev)                     # noqa: E731
    bad = lambda: torch.tensor([2000, 0, 2001], dtype=torch.int32, device=dev)                     # noqa: E731

    for lam in (10.0, 40.0):
        for log in (False, True):
            for dt in (torch.float32, torch.bfloat16):
                tag = f"lambd{lam:g}/log{int(log)}/{str(dt).split('.')[1]}"

                def mel(**kw):
                    return lambda: dm.MelSpectrogramLayer(lam, M, N, SR, hop_length=HOP, optimized=kw.pop("optimized", True), log=log, out_dtype=dt, **kw)

                for sync in (False, True):
                    s = f"sync{int(sync)}"
                    run(f"{tag}/mel/hot/{s}", mel(lambd_sync=sync))
                    run(f"{tag}/mel/xgrad/{s}", mel(lambd_sync=sync), x=grad_x())
                    run(f"{tag}/mel/full_window/{s}", mel(optimized=False, lambd_sync=sync))
                    run(f"{tag}/mel/full_window_xgrad/{s}", mel(optimized=False, lambd_sync=sync), x=grad_x())
                    for spec in (True, False):
                        run(f"{tag}/mel/fb/save_spec{int(spec)}/{s}", mel(learnable_fb=True, save_spec=spec, lambd_sync=sync))
                    run(f"{tag}/mel/fb_xgrad/{s}", mel(learnable_fb=True, lambd_sync=sync), x=grad_x())
                    run(f"{tag}/mel/fp64/{s}", mel(lambd_sync=sync), x=lambda: randn(B, N, dtype=torch.float64) + 3.0)
                    run(f"{tag}/mel/fp64_xgrad/{s}", mel(lambd_sync=sync), x=grad_x(torch.float64))
                    run(f"{tag}/mel/strided/{s}", mel(lambd_sync=sync), x=lambda: randn(B, 2 * N)[:, ::2])
                    for lname, ln in (("valid", full), ("invalid", bad)):
                        run(f"{tag}/mel/lengths_{lname}/{s}", mel(lambd_sync=sync), lengths=ln)
                        run(f"{tag}/mel/lengths_{lname}_xgrad/{s}", mel(lambd_sync=sync, lengths_waveform_grad=True), x=grad_x(), lengths=ln)
                    run(f"{tag}/mel/lengths_fp64_xgrad/{s}", mel(lambd_sync=sync, lengths_waveform_grad=True), x=grad_x(torch.float64), lengths=full)
                    run(f"{tag}/mel/lengths_refused_xgrad/{s}", mel(lambd_sync=sync), x=grad_x(), lengths=full)
                    run(f"{tag}/mel/slot/{s}", mel(lambd_sync=sync), slot=True)
                    run(f"{tag}/mel/slot_lengths/{s}", mel(lambd_sync=sync), slot=True, lengths=full)
                run(f"{tag}/mel/fb_lengths", mel(learnable_fb=True), lengths=full)
                run(f"{tag}/mel/slot_fb", mel(learnable_fb=True), slot=True)
                run(f"{tag}/mel/lengths_elsewhere", mel(), lengths=lambda: torch.empty(B, dtype=torch.int32, device="meta"))
                run(f"{tag}/dmel_log_mel", lambda: Holder(lam), call=lambda holder, x: dm.dmel_log_mel(x, holder.lambd, M, SR, HOP, log=log))
        for optimized, n in ((False, 250), (True, N)):
            size = (dm.capi.n_fft(lam) // 2 + 1, n // HOP + 1)
            for sync in (False, True):
                make = lambda: dm.SpectrogramLayer(lam, optimized=optimized, size=size, hop_length=HOP, lambd_sync=sync)   # noqa: E731
                run(f"lambd{lam:g}/dspec/optimized{int(optimized)}/sync{int(sync)}", make, x=lambda: randn(B, n))
                run(f"lambd{lam:g}/dspec/optimized{int(optimized)}_xgrad/sync{int(sync)}", make, x=lambda: randn(B, n).requires_grad_(True))
        run(f"lambd{lam:g}/dspec/wrong_size", lambda: dm.SpectrogramLayer(lam, optimized=True, size=(5, 5), hop_length=HOP))
    for log in (False, True):
        for dt in (torch.float32, torch.bfloat16):
            tag = f"K2/log{int(log)}/{str(dt).split('.')[1]}"
            for sync in (False, True):
                kw = dict(hop_length=HOP, log=log, out_dtype=dt, lambd_sync=sync)
                for wg in (False, True):
                    make = lambda: dm.MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, waveform_grad=wg, **kw)             # noqa: E731
                    run(f"{tag}/multi/waveform_grad{int(wg)}/sync{int(sync)}", make)
                    run(f"{tag}/multi/waveform_grad{int(wg)}_xgrad/sync{int(sync)}", make, x=grad_x())
                band = lambda: dm.BandSplitMelSpectrogram([40.0, 10.0], M, N, SR, **kw)                                     # noqa: E731
                run(f"{tag}/band/sync{int(sync)}", band)
                run(f"{tag}/band/xgrad_refused/sync{int(sync)}", band, x=grad_x())
                run(f"{tag}/band/fp64/sync{int(sync)}", band, x=lambda: randn(B, N, dtype=torch.float64))
    # refusals that need a device and belong to no setting: a layer left on the CPU, a slot or lengths where they are not taken
    run("refusal/mel/lambd_on_cpu", lambda: dm.MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=True), move=False)
    run("refusal/multi/lambd_on_cpu", lambda: dm.MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP), move=False)
    run("refusal/band/lambd_on_cpu", lambda: dm.BandSplitMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP), move=False)
    run("refusal/dspec/lambd_on_cpu", lambda: dm.SpectrogramLayer(10.0, hop_length=HOP), move=False)
    run("refusal/multi/slot", lambda: dm.MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP), slot=True)
    run("refusal/band/slot", lambda: dm.BandSplitMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP), slot=True)
    run("refusal/multi/lengths", lambda: dm.MultiWindowMelSpectrogram([10.0, 40.0], M, N, SR, hop_length=HOP), lengths=full)
    run("refusal/mel/fb_n_fft_moved", lambda: _moved(dm.MelSpectrogramLayer(10.0, M, N, SR, hop_length=HOP, optimized=True, learnable_fb=True,
                                                                             lambd_sync=True)))
    print("CHILD DONE", flush=True)


def _moved(layer):
    layer.lambd.data.fill_(40.0)             # the filterbank was built for lambd 10 (n_fft 64); 40 asks for n_fft 256
    return layer


def pair_lib_dirs(ap, packages, lib_dirs):
    """one library directory per package: the default, the one given for all, or as many as packages, in order"""
    lib_dirs = lib_dirs or [DEFAULT_PKG]
    if len(lib_dirs) == 1:
        return lib_dirs * len(packages)
    if len(lib_dirs) != len(packages):
        ap.error(f"{len(lib_dirs)} --lib-dir for {len(packages)} --package: give one, or one per package")
    return lib_dirs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--package", action="append", help="package directory to import as dmel_amd (give two to compare)")
    ap.add_argument("--lib-dir", action="append", help="directory of libdmel_hip.so and libdmel_torch.so: one for all packages, or one per package")
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of one child, seconds")
    ap.add_argument("--out", help="also write the table here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    packages = args.package or [DEFAULT_PKG]
    lib_dirs = pair_lib_dirs(ap, packages, args.lib_dir)
    if args.child:
        child(packages[0], lib_dirs[0])
        return 0
    tables = []
    for pkg, lib_dir in zip(packages, lib_dirs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package", pkg, "--lib-dir", lib_dir]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{pkg}: no result after {args.timeout:g} s, stopping", flush=True)
            return 2
        if res.returncode != 0 or "CHILD DONE" not in res.stdout:
            print(res.stdout[-2000:])
            print(f"{pkg}: the child ended with status {res.returncode}, stopping", flush=True)
            return 2
        tables.append(dict(line.split()[1:3] for line in res.stdout.splitlines() if line.startswith("DIGEST ")))
    lines = []
    names = list(tables[0])
    for name in names:
        shas = [t.get(name, "missing") for t in tables]
        lines.append(f"{name} {shas[0][:16]} " + ("" if len(tables) == 1 else "equal" if len(set(shas)) == 1 else "DIFFERENT " + " ".join(s[:16] for s in shas[1:])))
    diff = [ln for ln in lines if "DIFFERENT" in ln] + [f"{n} only in a later package" for t in tables[1:] for n in t if n not in tables[0]]
    verdict = f"{len(names)} digests" + ("" if len(tables) == 1 else ", all equal" if not diff else f", {len(diff)} DIFFERENT:\n" + "\n".join(diff))
    text = "\n".join(lines + [verdict])
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
