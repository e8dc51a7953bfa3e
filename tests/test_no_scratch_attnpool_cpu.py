"""The code objects of csrc/dmel_attnpool.hip (build/dmel_attnpool.o): the forward and the two backward kernels exist, spill no register and
use no scratch memory; the forward and the one-row backward allocate no LDS, the shared-rows backward the 8 KiB in which the waves that share an owner's rows meet.  Resource usage
only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_lengths_cpu import BUILD, LLVM

KERNELS = ("dmel_attnpool_bwd_kernel", "dmel_attnpool_bwd_row_kernel", "dmel_attnpool_fwd_kernel")


def test_attnpool_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "dmel_attnpool.o")
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    assert os.path.exists(obj), "build/dmel_attnpool.o is missing: csrc/dmel_attnpool.hip must be one of build.py's SOURCES"
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "attnpool.fat"), os.path.join(tmp, "attnpool.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fat}", f"--output={co}"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    found = []
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, None])[1]      # noqa: E731
        m = re.search(r"(dmel_attnpool_[a-z_]+_kernel)", g("name") or "")
        if m:
            found.append((m.group(1), g("name"), (int(g("vgpr_spill_count")), int(g("sgpr_spill_count")), int(g("private_segment_fixed_size"))),
                          g("vgpr_count"), g("group_segment_fixed_size")))
    assert sorted(name for name, *_ in found) == sorted(KERNELS), found
    for name, mangled, res, vgprs, lds in sorted(found):
        print(mangled, "vgpr spills, sgpr spills, scratch bytes:", res, "vgprs:", vgprs, "LDS bytes:", lds)
        assert res == (0, 0, 0), (mangled, res)
        if name != "dmel_attnpool_bwd_kernel":
            assert int(lds) == 0, (mangled, lds)                   # the lanes of a row meet through __shfl_xor: no LDS allocation
        else:
            assert 0 < int(lds) <= 16 * 64 * 8, (mangled, lds)     # one fp64 partial per lane of up to sixteen waves
