"""The multi-window layer's waveform gradient without a GPU: the three C entry points exist and reject a NULL plan before any device work,
the opt-in flag of the constructor, and the code objects of build/dmel_xgrad.o (what tools/kres.sh prints): every
dmel_xgrad_wave_multi_kernel<N> is free of spills and scratch, and the scalar x-gradient kernels keep the registers, spills, scratch and LDS
they had before the multi-window kernels were added next to them."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from dmel_amd import MultiWindowMelSpectrogram, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "differentiable-mel-spectrogram_amd", "build", "dmel_xgrad.o")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("dmel_backward_x_multi", "dmel_backward_x_multi_dev", "dmel_plan_last_multi_launch")

# the scalar x-gradient kernels as built before the multi-window kernels existed: name -> (vgpr, sgpr, spill, scratch, lds)
SCALAR = {
    "dmel_xgrad_gather_kernel": (14, 28, 0, 0, 2048),
    "dmel_xgrad_combine_kernel": (34, 52, 0, 0, 0),
    "dmel_xgrad_frames_kernel<false>": (33, 76, 0, 0, 0),
    "dmel_xgrad_frames_kernel<true>": (33, 77, 0, 0, 0),
    "dmel_xgrad_wave_kernel<32>": (66, 95, 0, 0, 0),
    "dmel_xgrad_wave_kernel<64>": (74, 93, 0, 0, 0),
    "dmel_xgrad_wave_kernel<128>": (78, 95, 0, 0, 0),
    "dmel_xgrad_wave_kernel<256>": (94, 93, 0, 0, 0),
    "dmel_xgrad_wave_kernel<512>": (92, 95, 0, 0, 0),
    "dmel_xgrad_wave_kernel<1024>": (88, 96, 0, 0, 0),
    "dmel_xgrad_wave_kernel<2048>": (136, 98, 0, 0, 0),
}


def test_symbols_listed_and_resolved():
    L = capi.load()
    for s in NEW:
        assert s in capi.SYMBOLS, s
        assert hasattr(L, s), s


def test_null_plan_is_invalid_argument():
    L = capi.load()
    lam = (C.c_float * 2)(40.0, 128.0)
    ns, masks, cnt = (C.c_int32 * 24)(256, 1024), (C.c_uint32 * 24)(1, 2), C.c_int32(0)
    assert L.dmel_backward_x_multi(None, None, 2, lam, 2, 0, None, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT
    assert L.dmel_backward_x_multi_dev(None, None, 2, None, 2, ns, masks, 2, 0, None, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT
    assert L.dmel_plan_last_multi_launch(None, ns, masks, C.byref(cnt)) == capi.DMEL_ERR_INVALID_ARGUMENT


def test_waveform_grad_flag():
    lay = MultiWindowMelSpectrogram([40.0, 128.0], 32, 8000, 16000, hop_length=128)
    assert lay.waveform_grad is False
    assert "waveform_grad=False" in repr(lay)
    on = MultiWindowMelSpectrogram([40.0, 128.0], 32, 8000, 16000, hop_length=128, log=True, waveform_grad=True)
    assert on.waveform_grad is True and "waveform_grad=True" in repr(on)
    back = pickle.loads(pickle.dumps(on))
    assert back.waveform_grad is True
    assert list(on.state_dict().keys()) == ["lambd"]
    on.load_state_dict({"lambd": torch.tensor([50.0, 60.0])})
    assert on.waveform_grad is True


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


def test_xgrad_kernel_resources():
    res = _kernel_resources()
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    for n in (32, 64, 128, 256, 512, 1024, 2048):
        name = f"dmel_xgrad_wave_multi_kernel<{n}>"
        assert name in res, sorted(res)
        _, _, spill, scratch, _ = res[name]
        assert spill == 0 and scratch == 0, (name, res[name])
    assert "dmel_xgrad_combine_multi_kernel" in res and res["dmel_xgrad_combine_multi_kernel"][2:4] == (0, 0)
    changed = {k: (res.get(k), v) for k, v in SCALAR.items() if res.get(k) != v}
    assert not changed, f"scalar x-gradient kernels changed (now, before): {changed}"
