"""Per-clip lengths without a GPU: the two C entry points are declared, exported, listed and refuse NULL arguments before any device
work; MelSpectrogramLayer.frame_lengths on CPU tensors; and the code objects of build/ (what tools/kres.sh prints): every training
instantiation of dmel_fwd_len_kernel up to n_fft 4096 is free of spills and scratch, and dmel_fwd_kernel / dmel_fwd_multi_kernel keep the
registers, spills and scratch they had before the lengths kernel was added next to them."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from dmel_amd import MelSpectrogramLayer, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "differentiable-mel-spectrogram_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("dmel_forward_lengths", "dmel_forward_dev_lengths")

# dmel_fwd_kernel and dmel_fwd_multi_kernel as built before the lengths kernel existed: (n_fft, mode, tiles) -> (vgpr, spilled, scratch bytes)
SCALAR = {
    (32, 0, 1): (104, 0, 0), (32, 1, 1): (103, 0, 0), (32, 2, 1): (66, 0, 0), (32, 3, 1): (61, 0, 0),
    (64, 0, 1): (104, 0, 0), (64, 1, 1): (103, 0, 0), (64, 2, 1): (74, 0, 0), (64, 3, 1): (64, 0, 0),
    (64, 4, 1): (68, 0, 0), (128, 0, 1): (79, 0, 0), (128, 1, 1): (78, 0, 0), (128, 2, 1): (74, 0, 0),
    (128, 3, 1): (64, 0, 0), (128, 4, 1): (68, 0, 0), (256, 0, 1): (88, 0, 0), (256, 0, 2): (107, 0, 0),
    (256, 1, 1): (90, 0, 0), (256, 1, 2): (105, 0, 0), (256, 2, 1): (90, 0, 0), (256, 2, 2): (92, 0, 0),
    (256, 3, 1): (70, 0, 0), (256, 3, 2): (76, 0, 0), (256, 4, 1): (74, 0, 0), (512, 0, 1): (103, 0, 0),
    (512, 0, 2): (128, 0, 0), (512, 1, 1): (90, 0, 0), (512, 1, 2): (128, 0, 0), (512, 2, 1): (88, 0, 0),
    (512, 2, 2): (106, 0, 0), (512, 3, 1): (90, 0, 0), (512, 3, 2): (106, 0, 0), (512, 4, 1): (92, 0, 0),
    (1024, 0, 1): (109, 0, 0), (1024, 1, 1): (102, 0, 0), (1024, 1, 2): (114, 0, 0), (1024, 2, 1): (88, 0, 0),
    (1024, 2, 2): (98, 0, 0), (1024, 3, 1): (108, 0, 0), (1024, 4, 1): (109, 0, 0), (1024, 5, 1): (109, 0, 0),
    (2048, 0, 1): (128, 0, 0), (2048, 1, 1): (128, 8, 36), (2048, 2, 1): (128, 8, 36), (2048, 3, 1): (122, 0, 0),
    (2048, 4, 1): (128, 7, 32), (2048, 5, 1): (126, 0, 0), (4096, 0, 1): (202, 0, 0), (4096, 1, 1): (256, 10, 44),
    (4096, 2, 1): (256, 8, 36), (4096, 3, 1): (202, 0, 0), (4096, 4, 1): (202, 0, 0), (8192, 0, 1): (212, 0, 0),
    (8192, 1, 1): (256, 22, 52), (8192, 2, 1): (256, 18, 44), (8192, 3, 1): (208, 0, 0), (16384, 0, 1): (256, 32, 124),
    (16384, 1, 1): (256, 53, 144), (16384, 2, 1): (256, 53, 128), (16384, 3, 1): (256, 28, 112),
}
# the multi-window kernel differs from the scalar one in these entries only
MULTI = dict(SCALAR)
MULTI.update({(256, 3, 1): (72, 0, 0), (512, 3, 1): (88, 0, 0), (512, 3, 2): (108, 0, 0), (1024, 2, 1): (86, 0, 0),
              (8192, 0, 1): (210, 0, 0), (16384, 2, 1): (256, 51, 128), (16384, 3, 1): (256, 29, 116)})


def test_symbols_listed_and_resolved():
    L = capi.load()
    for s in NEW:
        assert s in capi.SYMBOLS, s
        assert hasattr(L, s), s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{s}`" in doc for s in NEW)


def test_null_arguments_are_invalid_argument_without_a_device():
    L = capi.load()
    buf = (C.c_float * 16)()
    lens = (C.c_int32 * 4)(1, 2, 3, 4)
    p = C.cast(buf, C.c_void_p)
    q = C.cast(lens, C.c_void_p)
    for plan, x, ln, out in ((None, p, q, p), (None, None, q, p), (None, p, None, p), (None, p, q, None)):
        assert L.dmel_forward_lengths(plan, x, ln, 4, 40.0, 0, 1e-10, out, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT
        assert L.dmel_forward_dev_lengths(plan, x, ln, 4, p, 0, 1e-10, out, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT
    assert L.dmel_forward_dev_lengths(None, p, q, 4, None, 0, 1e-10, p, None, None, None) == capi.DMEL_ERR_INVALID_ARGUMENT


def test_frame_lengths_on_cpu_tensors():
    lay = MelSpectrogramLayer(torch.tensor(46.67), n_mels=64, n_points=8000, sample_rate=8000, hop_length=80, optimized=True)
    ln = torch.tensor([1, 79, 80, 81, 2400, 7999, 8000], dtype=torch.int64)
    fl = lay.frame_lengths(ln)
    assert fl.device.type == "cpu" and fl.dtype == torch.int64
    assert fl.tolist() == [v // 80 + 1 for v in ln.tolist()] == [1, 1, 2, 2, 31, 100, 101]
    assert lay.frame_lengths(ln.to(torch.int32)).tolist() == fl.tolist()
    assert int(lay.frame_lengths(torch.tensor([8000]))[0]) == lay.n_time


def _resources(pattern, kernel):
    objs = sorted(f for f in os.listdir(BUILD) if re.fullmatch(pattern, f)) if os.path.isdir(BUILD) else []
    if not objs or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        return None
    res = {}
    tmp = tempfile.mkdtemp()
    try:
        for o in objs:
            fat, co = os.path.join(tmp, o + ".fat"), os.path.join(tmp, o + ".co")
            subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", os.path.join(BUILD, o),
                                   os.path.join(tmp, "copy.o")])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={fat}", f"--output={co}"])
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
                m = re.search(r"_ZN4dmel\d+" + kernel + r"ILi(\d+)ELi(\d+)ELi(\d+)E", g("name") or "")
                if m:
                    res[tuple(int(v) for v in m.groups())] = (int(g("vgpr_count")), int(g("vgpr_spill_count")), int(g("private_segment_fixed_size")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def test_lengths_kernel_resources():
    res = _resources(r"dmel_fwd_len_part\d\.o", "dmel_fwd_len_kernel")
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    # the modes of the HTK layer, every size, one tile per workgroup
    want = {(n, m, 1) for n in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384) for m in (0, 1)} | {(1024, 5, 1), (2048, 5, 1)}
    assert want <= set(res), sorted(want - set(res))
    for (n, mode, tpw), (_, spill, scratch) in sorted(res.items()):
        if mode in (0, 5) and n <= 4096:
            assert spill == 0 and scratch == 0, (n, mode, tpw, res[(n, mode, tpw)])


def test_existing_forward_kernels_keep_their_resources():
    for kernel, table in (("dmel_fwd_kernel", SCALAR), ("dmel_fwd_multi_kernel", MULTI)):
        res = _resources(r"dmel_fwd_part\d\.o", kernel)
        if res is None:
            pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
        changed = {k: (res.get(k), v) for k, v in table.items() if res.get(k) != v}
        assert not changed and len(res) == len(table), f"{kernel} changed (now, before): {changed}"
