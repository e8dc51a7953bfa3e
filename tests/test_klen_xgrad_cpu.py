"""The waveform gradient of per-clip lengths on MultiWindowMelSpectrogram and BandSplitMelSpectrogram without a GPU: the constructor flag
(keyword-only, needs per_clip_lengths, in extra_repr, kept by pickle), with it an x that requires grad passes the gradient refusal, the four
C entry points are declared, listed, resolved and documented and refuse NULL / invalid arguments before any device work, and the code objects
of build/dmel_xgrad_klen.o: the fifteen kernels exist, are free of spills and scratch, and nothing else lives in the object."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from dmel_amd import capi
from test_klen_cpu import LAYERS, OnMeta, _raises
from test_layer_refusals_cpu import HOP, M, N, SR, OnDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "differentiable-mel-spectrogram_amd", "build", "dmel_xgrad_klen.o")
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("dmel_backward_x_multi_lengths", "dmel_backward_x_multi_dev_lengths", "dmel_backward_x_band_lengths", "dmel_backward_x_band_dev_lengths")


@pytest.mark.parametrize("name,make", LAYERS)
def test_flag_defaults_to_off_is_keyword_only_and_needs_per_clip_lengths(name, make):
    assert make().lengths_waveform_grad is False and make(per_clip_lengths=True).lengths_waveform_grad is False
    on = make(per_clip_lengths=True, lengths_waveform_grad=True)
    assert on.lengths_waveform_grad is True and on.per_clip_lengths is True and on.waveform_grad is False
    for kw in ({}, {"per_clip_lengths": False}, {"waveform_grad": True}):
        with pytest.raises(ValueError, match="per_clip_lengths=True"):
            make(lengths_waveform_grad=True, **kw)
    with pytest.raises(TypeError):
        type(on)([10.0, 40.0], M, N, SR, 0, None, HOP, False, True)                    # keyword-only: there is no ninth positional


@pytest.mark.parametrize("name,make", LAYERS)
def test_repr_state_and_pickle(name, make):
    on, off = make(per_clip_lengths=True, lengths_waveform_grad=True), make(per_clip_lengths=True)
    assert "lengths_waveform_grad=True" in on.extra_repr() and "lengths_waveform_grad=False" in off.extra_repr()
    assert "lengths_waveform_grad=False" in make().extra_repr() and "per_clip_lengths=True" in on.extra_repr()
    assert list(on.state_dict().keys()) == ["lambd"]
    on._plans["a plan"] = object()
    back = pickle.loads(pickle.dumps(on))
    assert back.lengths_waveform_grad is True and back.per_clip_lengths is True and back._plans == {} and torch.equal(back.lambd, on.lambd)
    assert pickle.loads(pickle.dumps(off)).lengths_waveform_grad is False
    back.load_state_dict({"lambd": torch.tensor([50.0, 60.0])})
    assert back.lengths_waveform_grad is True and back.lambd.tolist() == [50.0, 60.0]


@pytest.mark.parametrize("name,make", LAYERS)
def test_with_the_flag_an_x_that_requires_grad_passes_the_refusal(name, make):
    lengths = torch.empty(3, dtype=torch.int32, device="meta")
    nxt = "lambd is on cpu but x is on meta; call layer.to(x.device)"                    # the check after the gradient refusal
    for kw in ({}, {"waveform_grad": True}):
        _raises(RuntimeError, nxt, make(per_clip_lengths=True, lengths_waveform_grad=True, **kw), OnMeta(requires_grad=True), lengths)
    # the flag off: the refusal, word for word
    message = (f"per-clip lengths have no waveform gradient on {name} yet: pass x.detach() "
               "(MelSpectrogramLayer(lengths_waveform_grad=True) has one)")
    _raises(RuntimeError, message, make(per_clip_lengths=True), OnMeta(requires_grad=True), lengths)
    # forward(x) stays waveform_grad's: the new flag alone does not open it
    with pytest.raises(RuntimeError, match="has no waveform gradient"):
        make(per_clip_lengths=True, lengths_waveform_grad=True)(OnDevice(requires_grad=True))
    _raises(RuntimeError, "lambd is on cpu but x is on cuda:0; call layer.to(x.device)",
            make(per_clip_lengths=True, lengths_waveform_grad=True, waveform_grad=True), OnDevice(requires_grad=True))


def test_other_refusals_stay():
    from dmel_amd import GraphedStep
    from test_layer_refusals_cpu import LEN, slot
    for name, make in LAYERS:
        lay = make(per_clip_lengths=True, lengths_waveform_grad=True)
        with pytest.raises(RuntimeError, match=name + " does not take a SlotInput"):
            lay(slot(), LEN)
        with pytest.raises(ValueError, match=name):
            GraphedStep(lambda: None, [lay])


def test_symbols_declared_listed_resolved_and_documented():
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert re.search(r"dmel_status\s+" + s + r"\(", header), s
        assert s in capi.SYMBOLS and hasattr(L, s), s
        assert f"`{s}`" in doc, s
    assert re.search(r"#define\s+DMEL_ABI_VERSION\s+5\b", header) and L.dmel_abi_version() == 5
    import inspect
    for m in ("backward_x_multi", "backward_x_multi_dev", "backward_x_band", "backward_x_band_dev"):
        assert inspect.signature(getattr(capi.Plan, m)).parameters["lengths_ptr"].default is None, m


def test_null_and_invalid_arguments_need_no_device():
    L = capi.load()
    bad = capi.DMEL_ERR_INVALID_ARGUMENT
    lam = (C.c_float * 3)(300.0, 128.0, 40.0)
    good = (C.c_int32 * 4)(0, 21, 42, 64)
    ns, masks = (C.c_int32 * 24)(256, 1024, 2048), (C.c_uint32 * 24)(4, 2, 1)
    buf = (C.c_float * 64)()                                   # stands for every device pointer: nothing dereferences it
    p = C.addressof(buf)
    fake = C.cast(buf, C.c_void_p)                             # a handle that is never dereferenced either

    def mh(plan=None, x=p, ln=p, lam_=lam, K=3, flags=0, g=p, gx=p, **_):
        return L.dmel_backward_x_multi_lengths(plan, x, ln, 2, lam_, K, flags, g, None, gx, None)

    def md(plan=None, x=p, ln=p, lam_=p, K=3, ns_=ns, masks_=masks, count=3, flags=0, g=p, gx=p, **_):
        return L.dmel_backward_x_multi_dev_lengths(plan, x, ln, 2, lam_, K, ns_, masks_, count, flags, g, None, gx, None)

    def bh(plan=None, x=p, ln=p, lam_=lam, K=3, ed=good, flags=0, g=p, gx=p, **_):
        return L.dmel_backward_x_band_lengths(plan, x, ln, 2, lam_, K, ed, flags, g, None, gx, None)

    def bd(plan=None, x=p, ln=p, lam_=p, K=3, ed=good, ns_=ns, masks_=masks, count=3, flags=0, g=p, gx=p, **_):
        return L.dmel_backward_x_band_dev_lengths(plan, x, ln, 2, lam_, K, ed, ns_, masks_, count, flags, g, None, gx, None)

    def last():
        return (L.dmel_last_error() or b"").decode("utf-8", "replace")

    for fn in (mh, md, bh, bd):
        assert fn() == bad and "plan is NULL" in last()
        for kw in ({"x": None}, {"ln": None}, {"g": None}, {"gx": None}):
            assert fn(plan=fake, **kw) == bad, kw
            assert "is NULL" in last() and "plan is NULL" not in last(), (kw, last())
        assert fn(lam_=None) == bad
        assert fn(plan=fake, ln=None) == bad and "lengths is NULL" in last()
        for flags in (capi.DMEL_FLAG_CHECK_NFFT, capi.DMEL_FLAG_X_INDIRECT, capi.DMEL_FLAG_FULL_WINDOW, capi.DMEL_FLAG_OUT_BF16, 1 << 30):
            assert fn(plan=fake, flags=flags | capi.DMEL_FLAG_LOG) == bad, flags
            assert "DMEL_FLAG_LOG" in last()
        assert fn(plan=fake, flags=capi.DMEL_FLAG_LOG) == bad and "saved log output" in last()      # (out is NULL in these calls)
        assert fn(plan=fake, K=0) == bad and fn(plan=fake, K=9) == bad
    for fn, who in ((bh, "dmel_backward_x_band_lengths"), (bd, "dmel_backward_x_band_dev_lengths")):
        for name, ed in {"NULL edges": None, "empty group": (C.c_int32 * 4)(0, 21, 21, 64), "not starting at 0": (C.c_int32 * 4)(1, 21, 42, 64),
                         "descending": (C.c_int32 * 4)(0, 42, 21, 64)}.items():
            assert fn(ed=ed) == bad, name
            assert "plan is NULL" not in last() and who in last(), (name, last())
    assert mh(plan=fake, lam_=None) == bad and "lambd_host is NULL" in last()
    assert md(plan=fake, lam_=None) == bad and "lambd_dev is NULL" in last()
    assert bd(ns_=None) == bad and bd(masks_=None) == bad and bd(count=0) == bad
    # the launch list (the band form looks at the plan's n_mels before it: a live plan, test_hip_klen_xgrad.py)
    for fn in (md,):
        assert fn(plan=fake, ns_=None) == bad and fn(plan=fake, masks_=None) == bad and fn(plan=fake, count=0) == bad and fn(plan=fake, count=25) == bad
        assert fn(plan=fake, ns_=(C.c_int32 * 3)(256, 1000, 2048)) == bad and "power of two" in last()
        assert fn(plan=fake, ns_=(C.c_int32 * 3)(1024, 256, 2048)) == bad and "ascending" in last()
        assert fn(plan=fake, masks_=(C.c_uint32 * 3)(4, 0, 1)) == bad
        assert fn(plan=fake, masks_=(C.c_uint32 * 3)(4, 8, 1)) == bad                   # a channel >= channels
        assert fn(plan=fake, masks_=(C.c_uint32 * 3)(4, 4, 1)) == bad and "in no launch" in last()


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
            if dem is None:
                continue
            res[dem] = (int(g("vgpr_count")), int(g("sgpr_count")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")),
                        int(g("private_segment_fixed_size")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def test_the_fifteen_kernels_exist_without_spills_or_scratch_and_nothing_else():
    res = _kernel_resources()
    if res is None:
        pytest.skip("no compiled objects (python __graft_entry__.py build) or no llvm-readelf in this image")
    sizes = (32, 64, 128, 256, 512, 1024, 2048)
    want = [f"dmel_xgrad_wave_multi_len_kernel<{n}>" for n in sizes] + [f"dmel_xgrad_wave_band_len_kernel<{n}>" for n in sizes]
    want += ["dmel_xgrad_combine_multi_len_kernel"]
    assert len(want) == 15
    for name in want:
        assert name in res, (name, sorted(res))
        assert res[name][2:] == (0, 0, 0), (name, res[name])
    assert sorted(res) == sorted(want)
