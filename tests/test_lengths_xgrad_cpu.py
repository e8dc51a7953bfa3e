"""The waveform gradient of per-clip lengths without a GPU: the two C entry points exist and reject a NULL plan before any device work, the
opt-in flag of the constructor (default off, kept by pickle and load_state_dict, no new state_dict key, the same repr), and the code objects
of build/dmel_xgrad_len.o (what tools/kres.sh prints): every length-aware kernel exists and is free of spills and scratch."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from dmel_amd import MelSpectrogramLayer, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "differentiable-mel-spectrogram_amd", "build", "dmel_xgrad_len.o")
HEADER = os.path.join(ROOT, "include", "dmel.h")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("dmel_backward_x_lengths", "dmel_backward_x_dev_lengths")


def _layer(**kw):
    return MelSpectrogramLayer(40.0, 32, 8000, 16000, hop_length=100, optimized=True, log=True, **kw)


def test_symbols_declared_listed_and_resolved():
    with open(HEADER) as f:
        text = f.read()
    L = capi.load()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", text), f"{s} is not declared in include/dmel.h"
        assert s in capi.SYMBOLS, s
        assert hasattr(L, s), s
    for m in ("backward_x_lengths", "backward_x_dev_lengths", "forward_dev_lengths"):
        assert callable(getattr(capi.Plan, m, None)), m


def test_null_plan_is_invalid_argument():
    L = capi.load()
    assert L.dmel_backward_x_lengths(None, None, None, 2, C.c_float(40.0), 0, None, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT
    assert L.dmel_backward_x_dev_lengths(None, None, None, 2, None, 256, 0, None, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT


def test_flag_defaults_to_off_and_is_keyword_only():
    assert _layer().lengths_waveform_grad is False
    assert _layer(lengths_waveform_grad=True).lengths_waveform_grad is True
    with pytest.raises(TypeError):
        MelSpectrogramLayer(40.0, 32, 8000, 16000, 0, None, 100, "cpu", True, False, True)


def test_flag_survives_pickle_and_load_state_dict():
    on = _layer(lengths_waveform_grad=True)
    assert pickle.loads(pickle.dumps(on)).lengths_waveform_grad is True
    assert pickle.loads(pickle.dumps(_layer())).lengths_waveform_grad is False
    on.load_state_dict({"lambd": torch.tensor(50.0)})
    assert on.lengths_waveform_grad is True and float(on.lambd.detach()) == 50.0
    off = _layer()
    off.load_state_dict(on.state_dict())
    assert off.lengths_waveform_grad is False


def test_state_dict_keys_and_repr_do_not_change():
    on, off = _layer(lengths_waveform_grad=True), _layer()
    assert list(on.state_dict().keys()) == ["lambd"] == list(off.state_dict().keys())
    assert repr(on) == repr(off)
    fb = MelSpectrogramLayer(40.0, 32, 8000, 16000, hop_length=100, optimized=True, learnable_fb=True, lengths_waveform_grad=True)
    assert list(fb.state_dict().keys()) == ["lambd", "mel_fb"]


def test_cpu_tensor_still_raises_the_device_error():
    on = _layer(lengths_waveform_grad=True)
    x = torch.zeros(2, 8000, requires_grad=True)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        on(x, torch.tensor([8000, 4000], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        on(x.detach(), torch.tensor([8000, 4000], dtype=torch.int32))


def _demangle(name):
    """dmel::<identifier>[<int> | <bool>] from the mangled name (no c++filt needed), or None"""
    m = re.match(r"_ZN4dmel(\d+)", name)
    if not m:
        return None
    k = m.end()
    ident = name[k:k + int(m.group(1))]
    rest = name[k + int(m.group(1)):]
    t = re.match(r"IL(i|b)(\d+)EE", rest)
    if t:
        ident += f"<{t.group(2)}>" if t.group(1) == "i" else ("<true>" if t.group(2) == "1" else "<false>")
    return ident


def _kernel_resources():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        return None
    res = {}
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", OBJ, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
            dem = _demangle(g("name") or "")
            if dem is None or "xgrad" not in dem:
                continue
            res[dem] = (int(g("vgpr_count")), int(g("sgpr_count")), int(g("vgpr_spill_count")), int(g("private_segment_fixed_size")),
                        int(g("group_segment_fixed_size")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def test_length_aware_kernels_exist_without_spills_or_scratch():
    res = _kernel_resources()
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    want = [f"dmel_xgrad_wave_len_kernel<{n}>" for n in (32, 64, 128, 256, 512, 1024, 2048)]
    want += ["dmel_xgrad_frames_len_kernel<false>", "dmel_xgrad_frames_len_kernel<true>", "dmel_xgrad_gather_len_kernel",
             "dmel_xgrad_combine_len_kernel"]
    for name in want:
        assert name in res, (name, sorted(res))
        _, _, spill, scratch, _ = res[name]
        assert spill == 0 and scratch == 0, (name, res[name])
    # nothing else lives in this object: the kernels of dmel_xgrad.o are not compiled a second time
    assert sorted(res) == sorted(want)
