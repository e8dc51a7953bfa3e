"""PCEN without a GPU: the torch restatement the GPU tests measure against (tests/pcen_cases.py) is right -- its hand-written adjoint equals
fp64 autograd through its forward, silence stays exactly zero --, dmel_amd.PCEN constructs, projects and refuses on the CPU, the nets apply
``compression`` only when asked, and the three C entry points are exported, callable and loud without a device."""
import ctypes as C
import os

import pytest
import torch

import pcen_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_pcen_scratch_bytes", "dmel_pcen_forward", "dmel_pcen_backward")


@pytest.mark.parametrize("idx", range(len(P.SHAPES)))
def test_hand_written_adjoint_equals_fp64_autograd(idx):
    shape = P.SHAPES[idx]
    E, g = (t.double() for t in P.inputs(shape, idx))
    prm = [p.double().requires_grad_(True) for p in P.params(shape[-2], idx)]
    E.requires_grad_(True)
    y, _ = P.forward(E, *prm)
    grads = torch.autograd.grad((y * g).sum(), [E] + prm, allow_unused=True)
    grads = [torch.zeros_like(v) if d is None else d for d, v in zip(grads, [E] + prm)]      # (one frame: s is not used)
    with torch.no_grad():
        hand = P.backward(g, E, *prm)
    assert float((hand["y"] - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max() + 1)
    for name, ref in zip(("dE", "dalpha", "ddelta", "dr", "ds"), grads):
        scale = float(hand[name + "_scale"].max())
        err = float((hand[name] - ref).abs().max())
        print(shape, name, "max |hand - autograd| =", err, "of", scale)
        # (autograd adds the two powers' gradients as two sums: on an all-zero row they cancel to rounding, not to 0)
        assert err <= 1e-12 * scale + 1e-13 * float(g.abs().sum()), (name, err, scale)
        # the scales bound what they scale
        assert bool((hand[name].abs() <= hand[name + "_scale"] * (1 + 1e-12)).all()), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_silence_is_exactly_zero(dtype):
    for idx, shape in enumerate(P.SHAPES):
        E, _ = P.inputs(shape, idx)
        prm = [p.to(dtype) for p in P.params(shape[-2], idx)]
        y, M = P.forward(E.to(dtype), *prm)
        T = shape[-1]
        y2, E2 = y.reshape(-1, T), E.reshape(-1, T)
        assert bool((E2[0] == 0).all()) and bool((E2[-1, T // 3:] == 0).all())
        assert bool((y2[0] == 0).all()) and not bool(torch.signbit(y2[0]).any())
        assert bool((y2[-1, T // 3:] == 0).all()) and not bool(torch.signbit(y2[-1, T // 3:]).any())
        assert bool((y2 >= 0).all()) and (dtype == torch.float32 or bool((y2[E2 > 0] > 0).all()))
        assert M.shape == E.shape


def test_module_constructs_on_the_cpu():
    import dmel_amd
    from dmel_amd import pcen as pcen_mod
    m = dmel_amd.PCEN(7)
    assert dmel_amd.PCEN is pcen_mod.PCEN
    assert list(m.state_dict().keys()) == ["alpha", "delta", "r", "s"]
    assert [n for n, _ in m.named_parameters()] == ["alpha", "delta", "r", "s"]
    for name, value in (("alpha", 0.96), ("delta", 2.0), ("r", 0.5), ("s", 0.04)):
        p = getattr(m, name)
        assert isinstance(p, torch.nn.Parameter) and p.shape == (7,) and p.dtype == torch.float32 and p.requires_grad
        assert bool((p == torch.tensor(value, dtype=torch.float32)).all())
    assert m.eps == 1e-6
    f = dmel_amd.PCEN(3, alpha=0.5, delta=1.0, r=0.25, s=0.1, eps=1e-5, trainable=False)
    assert list(f.parameters()) == [] and list(f.state_dict().keys()) == ["alpha", "delta", "r", "s"]
    assert sorted(n for n, _ in f.named_buffers()) == ["alpha", "delta", "r", "s"] and f.eps == 1e-5
    assert float(f.r[0]) == 0.25 and not f.alpha.requires_grad
    m.load_state_dict(dmel_amd.PCEN(7, alpha=0.3).state_dict())
    assert float(m.alpha[0]) == pytest.approx(0.3)
    with pytest.raises(TypeError):
        dmel_amd.PCEN(3, 0.5)                                  # the values are keyword-only
    with pytest.raises(ValueError, match="eps"):
        dmel_amd.PCEN(3, eps=0.0)
    doc = pcen_mod.__doc__
    for phrase in ("fusing PCEN into the forward kernel", "forward-mode tangent", "bf16 input or output", "GraphedStep", "LambdAdam", "trainable ``eps``"):
        assert phrase in doc, phrase


def test_every_refusal_has_its_message():
    import dmel_amd
    m = dmel_amd.PCEN(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 5, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 5, 9))
    for dt in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match="fp32 linear mel power"):
            m(torch.zeros(2, 5, 9, dtype=dt))
    with pytest.raises(RuntimeError, match="built for n_mels=5 but dim -2 of the input has 9 bands"):
        m(torch.zeros(2, 9, 5))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m(torch.zeros(5, 9))
    with pytest.raises(RuntimeError, match=r"PCEN.alpha is on cpu but the input is on meta"):
        m(torch.zeros(2, 5, 9, device="meta"))


def test_project_clamps_in_place():
    import dmel_amd
    m = dmel_amd.PCEN(4)
    with torch.no_grad():
        m.alpha.copy_(torch.tensor([-0.5, 0.0, 0.7, 1.5]))
        m.delta.copy_(torch.tensor([-1.0, 0.0, 1e-3, 7.0]))
        m.r.copy_(torch.tensor([-1.0, 0.0, 0.5, 2.0]))
        m.s.copy_(torch.tensor([-1.0, 0.0, 0.04, 3.0]))
    ptrs = [p.data_ptr() for p in m.parameters()]
    assert m.project_() is m
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    assert torch.equal(m.alpha.data, f32([0.0, 0.0, 0.7, 1.0]))
    assert torch.equal(m.delta.data, f32([1e-3, 1e-3, 1e-3, 7.0]))
    assert torch.equal(m.r.data, f32([1e-3, 1e-3, 0.5, 1.0]))
    assert torch.equal(m.s.data, f32([1e-3, 1e-3, 0.04, 1.0]))
    assert bool((m.r > 0).all()) and all(p.requires_grad for p in m.parameters())
    frozen = dmel_amd.PCEN(2, alpha=3.0, trainable=False).project_()
    assert torch.equal(frozen.alpha, f32([1.0, 1.0]))


def test_features_apply_compression_only_when_set():
    import dmel_amd
    from dmel_amd import nets
    net = nets.MelLinearNet(3, torch.tensor(10.0), "cpu", 8, 8000, 800, hop_length=80, optimized=True)
    assert not hasattr(net, "compression")
    keys = list(net.state_dict().keys())
    s = torch.rand(2, 1, 8, 11)
    net.spectrogram_layer.forward = lambda x: s               # the front end needs the GPU
    assert net._features(torch.zeros(2, 800)) is s
    seen = []

    class Twice(torch.nn.Module):
        def forward(self, e):
            seen.append(e)
            return 2 * e

    net.compression = Twice()
    out = net._features(torch.zeros(2, 800))
    assert seen == [s] and torch.equal(out, 2 * s)
    net.compression = None
    assert net._features(torch.zeros(2, 800)) is s
    net.compression = dmel_amd.PCEN(8)
    assert list(net.state_dict().keys()) == keys + ["compression." + k for k in ("alpha", "delta", "r", "s")]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net._features(torch.zeros(2, 800))
    log_net = nets.MelMlpNet(3, torch.tensor(10.0), "cpu", 8, 8000, 800, hop_length=80, optimized=True, energy_normalize=True)
    with pytest.raises(ValueError, match="linear mel power"):
        log_net.compression = dmel_amd.PCEN(8)
    assert not hasattr(log_net, "compression")


def test_symbols_listed_exported_and_named():
    from dmel_amd import capi
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert L.dmel_abi_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NAMES)


def test_scratch_bytes_needs_no_device():
    from dmel_amd import capi
    assert capi.pcen_scratch_bytes(0) == 0
    assert capi.pcen_scratch_bytes(1) == 16
    assert capi.pcen_scratch_bytes(256 * 128) == 256 * 128 * 4 * 4
    assert capi.pcen_scratch_bytes(1 << 33) == (1 << 33) * 16
    assert capi.pcen_scratch_bytes(-5) == 0


def test_argument_checks_come_before_any_device_work():
    from dmel_amd import capi
    L = capi.load()
    buf = (C.c_float * 80)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                 # the scratch pointer must be 16-byte aligned
    INVALID = capi.DMEL_ERR_INVALID_ARGUMENT
    fwd = lambda E=p, rows=4, M=2, T=3, al=p, de=p, r=p, s=p, eps=1e-6, y=p, m=None: L.dmel_pcen_forward(E, rows, M, T, al, de, r, s, eps, y, m, None)   # noqa: E731
    bwd = lambda g=p, E=p, M_=p, rows=4, M=2, T=3, al=p, de=p, r=p, s=p, eps=1e-6, dE=p, dp=p, sc=p: L.dmel_pcen_backward(g, E, M_, rows, M, T, al, de, r, s, eps, dE, dp, sc, None)   # noqa: E731
    for bad in (dict(E=None), dict(y=None), dict(al=None), dict(de=None), dict(r=None), dict(s=None), dict(rows=5), dict(rows=-2), dict(M=0),
                dict(T=-1), dict(eps=0.0), dict(eps=float("nan"))):
        assert fwd(**bad) == INVALID, bad
        assert b"dmel_pcen_forward" in L.dmel_last_error()
    for bad in (dict(g=None), dict(E=None), dict(M_=None), dict(al=None), dict(s=None), dict(rows=3), dict(M=-1), dict(T=-4), dict(eps=-1.0),
                dict(sc=None), dict(sc=C.c_void_p(p.value + 4))):
        assert bwd(**bad) == INVALID, bad
        assert b"dmel_pcen_backward" in L.dmel_last_error()
    # no rows / no frames: a successful no-op, with or without a device
    assert fwd(rows=0) == capi.DMEL_OK and fwd(T=0) == capi.DMEL_OK
    assert bwd(rows=0) == capi.DMEL_OK and bwd(T=0) == capi.DMEL_OK
    assert bwd(dE=None, dp=None, sc=None) == capi.DMEL_OK         # nothing asked for
    assert all(v == 0.0 for v in buf)


def test_device_entry_points_fail_loudly_without_a_device():
    from dmel_amd import capi
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    buf = (C.c_float * 80)()
    p = (C.addressof(buf) + 15) & ~15
    with pytest.raises(capi.DmelError) as e:
        capi.pcen_forward(p, 4, 2, 3, p, p, p, p, 1e-6, p, None, None)
    assert e.value.status == capi.DMEL_ERR_NO_DEVICE and "dmel_pcen_forward" in str(e.value)
    with pytest.raises(capi.DmelError) as e:
        capi.pcen_backward(p, p, p, 4, 2, 3, p, p, p, p, 1e-6, p, p, p, None)
    assert e.value.status == capi.DMEL_ERR_NO_DEVICE and "dmel_pcen_backward" in str(e.value)
    with pytest.raises(capi.DmelError) as e:
        capi.pcen_forward(p, 5, 2, 3, p, p, p, p, 1e-6, p, None, None)
    assert e.value.status == capi.DMEL_ERR_INVALID_ARGUMENT and "multiple of n_mels" in str(e.value)
