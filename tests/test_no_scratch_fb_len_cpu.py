"""The code objects of csrc/dmel_fwd_fb_len.hip (dmel_fwd_fb_len_kernel: the length-aware forwards of a trained filterbank): every
instantiation the host can ask for exists, and kTrainH and kSpec spill no more registers than the same (n_fft, mode) of dmel_fwd_kernel in
the same build.  The length-aware builds of the filterbank gradient's GEMM (dmel_aux.o) use no scratch memory."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_lengths_cpu import BUILD, LLVM, _resources

SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
K_TRAIN, K_SPEC, K_TRAIN_H = 0, 2, 4


def _both():
    new = _resources(r"dmel_fwd_fb_len_part\d\.o", "dmel_fwd_fb_len_kernel")
    base = _resources(r"dmel_fwd_part\d\.o", "dmel_fwd_kernel")
    if not new or not base:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    return new, base


def test_every_instantiation_exists():
    new, _ = _both()
    want = ({(n, K_TRAIN, 1) for n in SIZES} | {(n, K_SPEC, 1) for n in SIZES} | {(n, K_TRAIN_H, 1) for n in SIZES if 64 <= n <= 4096})
    assert want == set(new), (sorted(want - set(new)), sorted(set(new) - want))


def test_no_more_spills_than_the_kernel_without_lengths():
    new, base = _both()
    for key, (vgpr, spill, scratch) in sorted(new.items()):
        print(key, "vgpr, spilled, scratch bytes:", (vgpr, spill, scratch), "dmel_fwd_kernel:", base[key])
    for key, (_, spill, _) in sorted(new.items()):
        if key[1] in (K_SPEC, K_TRAIN_H):
            assert spill <= base[key][1], (key, new[key], base[key])
    # the exact contraction up to n_fft 8192: no spill and no scratch, as dmel_fwd_len_kernel's (tests/test_lengths_cpu.py)
    for n in SIZES:
        if n <= 8192:
            assert new[(n, K_TRAIN, 1)][1:] == (0, 0), (n, new[(n, K_TRAIN, 1)])


def test_length_aware_gemm_uses_no_scratch():
    obj = os.path.join(BUILD, "dmel_aux.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "aux.fat"), os.path.join(tmp, "aux.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = {}
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
        m = re.search(r"dmel_fbgrad_lds_kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)E", g("name") or "")
        if m:
            found[tuple(int(v) for v in m.groups())] = (int(g("vgpr_spill_count")), int(g("private_segment_fixed_size")))
    # LOG x TINY x BF16X3, with and without lengths
    assert set(found) == {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}, sorted(found)
    for key, res in sorted(found.items()):
        assert res == (0, 0), (key, res)
