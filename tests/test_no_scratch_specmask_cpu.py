"""The code objects of csrc/dmel_specmask.hip (build/dmel_specmask.o): the draw kernel and both builds of the apply kernel (4-byte and 2-byte
elements) exist, spill no register and use no scratch memory.  Resource usage only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_lengths_cpu import BUILD, LLVM

KERNELS = ("dmel_specmask_draw_kernel", "dmel_specmask_apply_kernel")


def test_specmask_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "dmel_specmask.o")
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    assert os.path.exists(obj), "build/dmel_specmask.o is missing: csrc/dmel_specmask.hip must be one of build.py's SOURCES"
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "specmask.fat"), os.path.join(tmp, "specmask.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = []
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
        m = re.search(r"(dmel_specmask_[a-z_]+_kernel)", g("name") or "")
        if m:
            found.append((m.group(1), g("name"), (int(g("vgpr_spill_count")), int(g("sgpr_spill_count")), int(g("private_segment_fixed_size")))))
    assert sorted(name for name, _, _ in found) == ["dmel_specmask_apply_kernel"] * 2 + ["dmel_specmask_draw_kernel"], found
    assert set(name for name, _, _ in found) == set(KERNELS)
    for name, mangled, res in sorted(found):
        print(mangled, "vgpr spills, sgpr spills, scratch bytes:", res)
        assert res == (0, 0, 0), (mangled, res)
