"""The code objects of csrc/dmel_bandnorm.hip (build/dmel_bandnorm.o): the row statistics, the band combine and the apply of the forward and of
the backward exist, spill no register and use no scratch memory."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_lengths_cpu import BUILD, LLVM

KERNELS = ("dmel_bandnorm_rowstat_kernel", "dmel_bandnorm_combine_kernel", "dmel_bandnorm_apply_kernel", "dmel_bandnorm_bwd_rowstat_kernel",
           "dmel_bandnorm_bwd_combine_kernel", "dmel_bandnorm_bwd_apply_kernel")


def test_bandnorm_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "dmel_bandnorm.o")
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    assert os.path.exists(obj), "build/dmel_bandnorm.o is missing: csrc/dmel_bandnorm.hip must be one of build.py's SOURCES"
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "bandnorm.fat"), os.path.join(tmp, "bandnorm.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = {}
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
        m = re.search(r"(dmel_bandnorm_[a-z_]+_kernel)", g("name") or "")
        if m:
            found[m.group(1)] = (int(g("vgpr_spill_count")), int(g("sgpr_spill_count")), int(g("private_segment_fixed_size")))
    assert set(found) == set(KERNELS), sorted(found)
    for name, res in sorted(found.items()):
        print(name, "vgpr spills, sgpr spills, scratch bytes:", res)
        assert res == (0, 0, 0), (name, res)
