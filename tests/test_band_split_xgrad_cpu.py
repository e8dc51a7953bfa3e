"""The band-split layer's waveform gradient without a GPU: the two C entry points exist, are documented and reject NULL / invalid arguments
before any device work, the opt-in flag of the constructor, and the code objects of build/dmel_xgrad_band.o: every
dmel_xgrad_wave_band_kernel<N> and the staging kernel are free of spills and scratch."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "differentiable-mel-spectrogram_amd", "build", "dmel_xgrad_band.o")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("dmel_backward_x_band", "dmel_backward_x_band_dev")


def test_symbols_listed_resolved_and_documented():
    L = capi.load()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for s in NEW:
        assert s in capi.SYMBOLS, s
        assert hasattr(L, s), s
        assert f"`{s}`" in doc, s
    assert L.dmel_abi_version() == 5


def test_null_and_invalid_arguments_need_no_device():
    """NULL plan / x / grad_out / grad_x / band_edges / launch list: DMEL_ERR_INVALID_ARGUMENT, and no device is asked for (this machine has
    none; a plan cannot exist here, so the checks behind a live plan are in the GPU suite: test_band_xgrad_argument_checks)"""
    L = capi.load()
    bad = capi.DMEL_ERR_INVALID_ARGUMENT
    lam = (C.c_float * 3)(300.0, 128.0, 40.0)
    good = (C.c_int32 * 4)(0, 21, 42, 64)
    ns, masks = (C.c_int32 * 24)(256, 1024, 2048), (C.c_uint32 * 24)(4, 2, 1)
    buf = (C.c_float * 64)()                                   # stands for every device pointer: nothing dereferences it
    p = C.addressof(buf)

    def host(x=p, lam_=lam, K=3, ed=good, g=p, gx=p):
        return L.dmel_backward_x_band(None, x, 2, lam_, K, ed, 0, g, None, gx, None)

    def dev(x=p, lam_=p, K=3, ed=good, ns_=ns, masks_=masks, count=3, g=p, gx=p):
        return L.dmel_backward_x_band_dev(None, x, 2, lam_, K, ed, ns_, masks_, count, 0, g, None, gx, None)

    for fn in (host, dev):
        assert fn() == bad                                     # the NULL plan
        for kw in ({"x": None}, {"g": None}, {"gx": None}, {"lam_": None}):
            assert fn(**kw) == bad, kw
        for name, kw in {"NULL edges": {"ed": None}, "empty group": {"ed": (C.c_int32 * 4)(0, 21, 21, 64)},
                         "not starting at 0": {"ed": (C.c_int32 * 4)(1, 21, 42, 64)}, "K = 0": {"K": 0}, "K = 9": {"K": 9}}.items():
            assert fn(**kw) == bad, name
            msg = (L.dmel_last_error() or b"").decode("utf-8", "replace")
            assert "plan is NULL" not in msg and "dmel_backward_x_band" in msg, (name, msg)      # refused for the edges themselves
    assert dev(ns_=None) == bad and dev(masks_=None) == bad and dev(count=0) == bad


def test_waveform_grad_flag():
    lay = BandSplitMelSpectrogram([300.0, 128.0, 40.0], 32, 8000, 16000, hop_length=128)
    assert lay.waveform_grad is False
    assert "waveform_grad=False" in repr(lay)
    on = BandSplitMelSpectrogram([300.0, 128.0, 40.0], 32, 8000, 16000, hop_length=128, band_edges=[0, 5, 17, 32], log=True, waveform_grad=True)
    assert on.waveform_grad is True and "waveform_grad=True" in repr(on)
    back = pickle.loads(pickle.dumps(on))
    assert back.waveform_grad is True and back.band_edges == (0, 5, 17, 32)
    assert list(on.state_dict().keys()) == ["lambd"]
    on.load_state_dict({"lambd": torch.tensor([50.0, 60.0, 70.0])})
    assert on.waveform_grad is True


def _demangle(name):
    """dmel::<identifier>[<int>] from the mangled name (no c++filt needed), or None"""
    m = re.match(r"_ZN4dmel(\d+)", name)
    if not m:
        return None
    k = m.end()
    ident = name[k:k + int(m.group(1))]
    t = re.match(r"ILi(\d+)EE", name[k + int(m.group(1)):])
    return ident + (f"<{t.group(1)}>" if t else "")


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
            res[dem] = (int(g("vgpr_count")), int(g("sgpr_count")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")),
                        int(g("private_segment_fixed_size")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def test_band_xgrad_kernel_resources():
    res = _kernel_resources()
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    names = [f"dmel_xgrad_wave_band_kernel<{n}>" for n in (32, 64, 128, 256, 512, 1024, 2048)] + ["dmel_xgrad_band_stage_kernel"]
    for name in names:
        assert name in res, sorted(res)
        assert res[name][2:] == (0, 0, 0), (name, res[name])
