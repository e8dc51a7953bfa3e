"""`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on the GPU: a plain run prints one JSON line with the headline keys and
none of the side measurements (those are `--full`'s), and DIR holds what the LAST timed step computed -- the log-mel output, lambd.grad
and lambd after the update -- checked against the fp64 oracle at the lambd that step ran at."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_timed_step_computed(tmp_path):
    from dmel_amd import synth
    from oracle import dmel_oracle as O
    import bench
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "4", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 20 and rec["warmup"] == 4 and rec["unit"] == "frames/s" and rec["dtype"] == "f32" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["module_step"]["timed_regions"]["n"] == 1
    assert not {"c_abi_kernels", "roofline", "kernel_info", "other_configs", "cpu_baseline"} & set(rec)

    B, L, sr, lam0, hop, M = bench.CONFIGS["c2"]
    T = L // hop + 1
    y, d, lam = (np.load(out / f"{n}.npy") for n in ("logmel", "lambd_grad", "lambd"))
    assert y.dtype == d.dtype == lam.dtype == np.float32
    assert y.shape == (B, 1, M, T) and d.shape == lam.shape == (1,)
    assert abs(float(lam[0]) - rec["module_step"]["lambd_end"]) <= 1e-4
    # the last step ran at the lambd before its update: Adam moves lambd by lr against the sign of a gradient that keeps its sign
    # (to ~1e-6 here); one step earlier or later the output differs by ~1.1e-3, well above the bound below
    lam_step = float(lam[0]) + bench.ADAM_LR * float(np.sign(d[0]))
    x = synth.waveforms(B, L, seed=0)
    g = synth.cotangent((B, 1, M, T), seed=1)
    y_ref, tan = O.forward(x, lam_step, hop, M, sr, apply_log=True)
    d_ref = O.backward(g, tan)
    err = np.abs(y - y_ref)
    assert (err <= 3e-4 + 1e-4 * np.abs(y_ref)).all(), float(err.max())
    assert abs(float(d[0]) - d_ref) <= 3e-4 * abs(d_ref), (float(d[0]), d_ref)
