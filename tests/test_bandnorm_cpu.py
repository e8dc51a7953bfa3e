"""BandNorm without a GPU: the torch restatement the GPU tests measure against (tests/bandnorm_cases.py) is right -- its hand-written adjoint
equals fp64 autograd through its forward, at full lengths it is nn.BatchNorm2d and with mixed lengths nn.BatchNorm1d on the gathered valid
frames, in fp32 it stays far below the GPU test's cap --, dmel_amd.BandNorm constructs, loads a batch norm's state and refuses on the CPU, and
the three C entry points are exported, callable and loud without a device."""
import ctypes as C
import os

import pytest
import torch

import bandnorm_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dmel_bandnorm_scratch_bytes", "dmel_bandnorm_forward", "dmel_bandnorm_backward")
IDS = [str(s) for s in N.SHAPES]
MODES = [("clip", False), ("batch", False), ("batch", True)]          # (stats, eval)
# (torch's batch norms refuse to train on one value per channel: the one-frame shape has no torch counterpart)
TRAINABLE = [i for i, (B, C, M, T) in enumerate(N.SHAPES) if B * C * T >= 2]


def _case(idx, with_lengths, dtype=torch.float64):
    shape = N.SHAPES[idx]
    s, g = (t.to(dtype) for t in N.inputs(shape, idx))
    w, b, rm, rv = N.params(shape[2], idx, dtype)
    return shape, s, g, w, b, rm, rv, (N.frame_lengths(shape, idx) if with_lengths else None)


@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "full"])
@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_hand_written_adjoint_equals_fp64_autograd(idx, with_lengths):
    shape, s, g, w, b, rm, rv, Tc = _case(idx, with_lengths)
    for stats, ev in MODES:
        running = (rm, rv) if ev else None
        leaves = [t.clone().requires_grad_(True) for t in (s, w, b)]
        y = N.forward(*leaves, Tc, stats, running=running)
        grads = torch.autograd.grad((y * g).sum(), leaves)
        with torch.no_grad():
            hand = N.backward(g, s, w, b, Tc, stats, running=running)
        assert torch.equal(hand["y"], y.detach())
        for name, ref in zip(("ds", "dweight", "dbias"), grads):
            scale = hand[name + "_scale"]
            err = (hand[name] - ref).abs()
            print(shape, stats, "eval" if ev else "train", name, "max |hand - autograd| =", float(err.max()), "of", float(scale.max()))
            assert bool((err <= 1e-12 * scale.max()).all()), (stats, ev, name, float(err.max()), float(scale.max()))
            # the scales bound what they scale, and nothing but a pad frame has none
            assert bool((hand[name].abs() <= scale * (1 + 1e-12)).all()), name
        pad = ~N.valid_mask(shape, Tc).expand(shape)
        assert bool((hand["y"][pad] == 0).all()) and bool((hand["ds"][pad] == 0).all()) and bool((hand["ds_scale"][pad] == 0).all())
        assert bool((grads[0][pad] == 0).all())


@pytest.mark.parametrize("idx", TRAINABLE, ids=[IDS[i] for i in TRAINABLE])
def test_full_lengths_are_batchnorm2d(idx):
    shape, s, g, w, b, rm, rv, _ = _case(idx, False)
    B, C, M, T = shape
    bn = torch.nn.BatchNorm2d(M, eps=N.EPS, momentum=N.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    x = s.clone().requires_grad_(True)
    y_bn = bn(x.transpose(1, 2)).transpose(1, 2)
    (ds_bn,) = torch.autograd.grad((y_bn * g).sum(), [x])
    hand = N.backward(g, s, w, b, None, "batch")
    new_mean, new_var, _, _ = N.updated_running(s, None, rm, rv)
    for name, got, ref in (("y", hand["y"], y_bn.detach()), ("ds", hand["ds"], ds_bn), ("running_mean", new_mean, bn.running_mean),
                           ("running_var", new_var, bn.running_var)):
        err = float((got - ref).abs().max())
        print(shape, name, "max |restatement - BatchNorm2d| =", err)
        assert err <= 1e-12 * float(ref.abs().max() + 1), (name, err)
    bn.eval()
    y_eval = bn(s.transpose(1, 2)).transpose(1, 2).detach()
    running = (bn.running_mean.detach(), bn.running_var.detach())
    assert float((N.forward(s, w, b, None, "batch", running=running) - y_eval).abs().max()) <= 1e-12 * float(y_eval.abs().max() + 1)


@pytest.mark.parametrize("idx", TRAINABLE, ids=[IDS[i] for i in TRAINABLE])
def test_mixed_lengths_are_batchnorm1d_on_the_gathered_valid_frames(idx):
    shape, s, g, w, b, rm, rv, Tc = _case(idx, True)
    B, C, M, T = shape
    valid = N.valid_mask(shape, Tc).expand(B, C, 1, T).reshape(-1)
    assert int(valid.sum()) >= 2
    bn = torch.nn.BatchNorm1d(M, eps=N.EPS, momentum=N.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    gathered = s.permute(0, 1, 3, 2).reshape(-1, M)[valid]                # (valid frames of every clip and channel, M)
    y_bn = bn(gathered)
    y = N.forward(s, w, b, Tc, "batch").permute(0, 1, 3, 2).reshape(-1, M)
    new_mean, new_var, _, _ = N.updated_running(s, Tc, rm, rv)
    for name, got, ref in (("y", y[valid], y_bn.detach()), ("running_mean", new_mean, bn.running_mean), ("running_var", new_var, bn.running_var)):
        err = float((got - ref).abs().max())
        print(shape, name, "max |restatement - BatchNorm1d| =", err)
        assert err <= 1e-12 * float(ref.abs().max() + 1), (name, err)
    assert bool((y[~valid] == 0).all())


@pytest.mark.parametrize("idx", range(len(N.SHAPES)), ids=IDS)
def test_fp32_restatement_stays_below_an_eighth_of_the_cap(idx):
    """8 x its error is the GPU test's bound, capped at 1e-4: the cap must never be the one that binds.  Measured on these inputs, worst over
    shapes, modes and lengths: y 2.8e-7, ds 2.2e-6 at (130, 1, 1, 3), dweight 2.0e-7, dbias 6.1e-8."""
    for with_lengths in (True, False):
        shape, s, g, w, b, rm, rv, Tc = _case(idx, with_lengths, torch.float32)
        for stats, ev in MODES:
            ref = N.backward(g.double(), s.double(), w.double(), b.double(), Tc, stats, running=(rm.double(), rv.double()) if ev else None)
            r32 = N.backward(g, s, w, b, Tc, stats, running=(rm, rv) if ev else None)
            for k in ("y", "ds", "dweight", "dbias"):
                e = N.worst(r32[k], ref[k], ref[k + "_scale"])
                print(shape, stats, "eval" if ev else "train", "lengths" if with_lengths else "full", k, f"{e:.3e}")
                assert e <= 1e-4 / 8, (stats, ev, k, e)
        m64 = N.updated_running(s.double(), Tc, rm.double(), rv.double())
        m32 = N.updated_running(s, Tc, rm, rv)
        for i, k in enumerate(("running_mean", "running_var")):
            assert N.worst(m32[i], m64[i], m64[2 + i]) <= 1e-4 / 8, k


def test_module_constructs_on_the_cpu_and_takes_a_batchnorm_state():
    import dmel_amd
    from dmel_amd import bandnorm as mod
    assert dmel_amd.BandNorm is mod.BandNorm and "BandNorm" in dmel_amd.__all__ and "bandnorm" in dmel_amd.__all__
    keys = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    m = dmel_amd.BandNorm(7, stats="batch")
    assert list(m.state_dict().keys()) == keys == list(torch.nn.BatchNorm2d(7).state_dict().keys())
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
    assert torch.equal(m.weight.data, torch.ones(7)) and torch.equal(m.bias.data, torch.zeros(7)) and m.weight.dtype == torch.float32
    assert torch.equal(m.running_mean, torch.zeros(7)) and torch.equal(m.running_var, torch.ones(7))
    assert m.num_batches_tracked.dtype == torch.int64 and int(m.num_batches_tracked) == 0 and m.eps == 1e-5 and m.momentum == 0.1
    c = dmel_amd.BandNorm(7)
    assert c.stats == "clip" and list(c.state_dict().keys()) == ["weight", "bias"] and c.running_mean is None
    assert list(dmel_amd.BandNorm(3, affine=False).state_dict().keys()) == [] and dmel_amd.BandNorm(3, affine=False).weight is None
    assert list(dmel_amd.BandNorm(3, "batch", affine=False).state_dict().keys()) == keys[2:]
    # the bn1 of a Cnn6 loads as it is
    bn = torch.nn.BatchNorm2d(7, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 2), bn.bias.normal_(), bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2)
        bn.num_batches_tracked.fill_(11)
    m.load_state_dict(bn.state_dict())
    f = dmel_amd.BandNorm.from_batchnorm(bn.eval())
    for got in (m, f):
        for k in keys:
            assert torch.equal(got.state_dict()[k], bn.state_dict()[k]), k
    assert f.eps == 1e-3 and f.momentum == 0.01 and f.stats == "batch" and not f.training and f.weight is not bn.weight
    assert "stats='batch'" in repr(f)
    with pytest.raises(ValueError, match="stats must be 'clip' or 'batch'"):
        dmel_amd.BandNorm(3, stats="layer")
    with pytest.raises(ValueError, match="eps"):
        dmel_amd.BandNorm(3, eps=0.0)
    with pytest.raises(ValueError, match="momentum=None"):
        dmel_amd.BandNorm(3, "batch", momentum=None)
    with pytest.raises(ValueError, match="n_mels must be positive"):
        dmel_amd.BandNorm(0)
    with pytest.raises(TypeError, match="from_batchnorm takes"):
        dmel_amd.BandNorm.from_batchnorm(torch.nn.LayerNorm(3))
    for phrase in ("bf16 input or output", "fusing the stage into the forward or into PCEN", "``lengths`` argument on the nets", "GraphedStep",
                   "LambdAdam", "momentum=None", "synchronised statistics"):
        assert phrase in " ".join(mod.__doc__.split()), phrase


def test_every_refusal_has_its_message():
    import dmel_amd
    m = dmel_amd.BandNorm(5, stats="batch")
    ok = torch.tensor([9, 4])
    for shape in ((2, 5, 9), (2, 3, 5, 9)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros(shape))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros(shape), ok)
    for dt in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match="takes an fp32 mel image"):
            m(torch.zeros(2, 5, 9, dtype=dt))
    with pytest.raises(RuntimeError, match="built for n_mels=5 but dim -2 of the input has 9 bands"):
        m(torch.zeros(2, 9, 5))
    with pytest.raises(ValueError, match=r"\(B, n_mels, T\) or \(B, C, n_mels, T\)"):
        m(torch.zeros(5, 9))
    with pytest.raises(ValueError, match=r"frame_lengths must have shape \(2,\), got \(3,\)"):
        m(torch.zeros(2, 5, 9), torch.tensor([9, 4, 1]))
    with pytest.raises(ValueError, match=r"frame_lengths must have shape \(2,\), got \(2, 1\)"):
        m(torch.zeros(2, 5, 9), ok[:, None])
    with pytest.raises(TypeError, match="frame_lengths must hold int32 or int64 values, got torch.float32"):
        m(torch.zeros(2, 5, 9), ok.float())
    with pytest.raises(TypeError, match="frame_lengths must be a 1-D integer tensor, got list"):
        m(torch.zeros(2, 5, 9), [9, 4])
    with pytest.raises(RuntimeError, match="frame_lengths is on cpu but the input is on meta"):
        m(torch.zeros(2, 5, 9, device="meta"), ok)
    with pytest.raises(RuntimeError, match=r"BandNorm.weight is on cpu but the input is on meta"):
        m(torch.zeros(2, 5, 9, device="meta"))
    with pytest.raises(RuntimeError, match=r"BandNorm.weight must stay torch.float32"):
        dmel_amd.BandNorm(5).double()(torch.zeros(2, 5, 9))


def test_symbols_listed_exported_and_named():
    from dmel_amd import capi
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert L.dmel_abi_version() == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in doc for name in NAMES)
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    assert "size_t dmel_bandnorm_scratch_bytes(" in header
    assert all(f"dmel_status {name}(" in header for name in NAMES[1:])


def test_scratch_bytes_needs_no_device():
    from dmel_amd import capi
    assert capi.bandnorm_scratch_bytes(0, 0) == 0
    assert capi.bandnorm_scratch_bytes(1, 1) == 32
    assert capi.bandnorm_scratch_bytes(256 * 128, 128) == (256 * 128 + 128) * 16
    assert capi.bandnorm_scratch_bytes(1 << 33, 64) == ((1 << 33) + 64) * 16
    assert capi.bandnorm_scratch_bytes(-5, -1) == 0


def _aligned(buf):
    return C.c_void_p((C.addressof(buf) + 15) & ~15)


def test_argument_checks_come_before_any_device_work():
    from dmel_amd import capi
    L = capi.load()
    buf = (C.c_double * 80)()
    p = _aligned(buf)
    odd = C.c_void_p(p.value + 8)
    INVALID = capi.DMEL_ERR_INVALID_ARGUMENT

    def fwd(s=p, rows=4, M=2, rpc=2, T=3, ln=None, w=p, b=p, batch=1, train=1, eps=1e-5, mom=0.1, rm=p, rv=p, nbt=p, y=p, st=p, sc=p):
        return L.dmel_bandnorm_forward(s, rows, M, rpc, T, ln, w, b, batch, train, eps, mom, rm, rv, nbt, y, st, sc, None)

    def bwd(g=p, s=p, st=p, rows=4, M=2, rpc=2, T=3, ln=None, w=p, batch=1, train=1, ds=p, dw=p, db=p, sc=p):
        return L.dmel_bandnorm_backward(g, s, st, rows, M, rpc, T, ln, w, batch, train, ds, dw, db, sc, None)

    for bad, word in ((dict(s=None), "s / y"), (dict(y=None), "s / y"), (dict(st=None), "stats"), (dict(st=odd), "stats"), (dict(rows=5), "rows_per_clip"),
                      (dict(rows=-2), "rows"), (dict(M=0), "n_mels"), (dict(T=-1), "T"), (dict(rpc=3), "rows_per_clip"), (dict(rpc=0), "rows_per_clip"),
                      (dict(batch=2), "batch_stats"), (dict(train=-1), "training"), (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"),
                      (dict(mom=1.5), "momentum"), (dict(mom=float("nan")), "momentum"), (dict(train=0, rm=None, rv=None), "running_mean"),
                      (dict(rm=None), "running_mean"), (dict(batch=0), "running_mean"), (dict(sc=None), "scratch"), (dict(sc=odd), "scratch")):
        assert fwd(**bad) == INVALID, bad
        msg = L.dmel_last_error().decode()
        assert "dmel_bandnorm_forward" in msg and word in msg, (bad, msg)
    for bad, word in ((dict(g=None), "g / s"), (dict(s=None), "g / s"), (dict(st=None), "stats"), (dict(rows=3), "rows_per_clip"), (dict(M=-1), "n_mels"),
                      (dict(T=-4), "T"), (dict(rpc=5), "rows_per_clip"), (dict(batch=7), "batch_stats"), (dict(sc=None), "scratch"), (dict(sc=odd), "scratch")):
        assert bwd(**bad) == INVALID, bad
        msg = L.dmel_last_error().decode()
        assert "dmel_bandnorm_backward" in msg and word in msg, (bad, msg)
    # no rows / no frames: a successful no-op, with or without a device
    assert fwd(rows=0) == capi.DMEL_OK and fwd(T=0) == capi.DMEL_OK
    assert bwd(rows=0) == capi.DMEL_OK and bwd(T=0) == capi.DMEL_OK
    assert bwd(ds=None, dw=None, db=None) == capi.DMEL_OK         # nothing asked for
    assert all(v == 0.0 for v in buf)


def test_device_entry_points_fail_loudly_without_a_device():
    from dmel_amd import capi
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    buf = (C.c_double * 80)()
    p = _aligned(buf).value
    with pytest.raises(capi.DmelError) as e:
        capi.bandnorm_forward(p, 4, 2, 2, 3, None, p, p, True, True, 1e-5, 0.1, p, p, p, p, p, p, None)
    assert e.value.status == capi.DMEL_ERR_NO_DEVICE and "dmel_bandnorm_forward" in str(e.value)
    with pytest.raises(capi.DmelError) as e:
        capi.bandnorm_forward(p, 4, 2, 2, 3, None, None, None, False, True, 1e-5, 0.1, None, None, None, p, p, None, None)
    assert e.value.status == capi.DMEL_ERR_NO_DEVICE
    with pytest.raises(capi.DmelError) as e:
        capi.bandnorm_backward(p, p, p, 4, 2, 2, 3, None, p, True, True, p, p, p, p, None)
    assert e.value.status == capi.DMEL_ERR_NO_DEVICE and "dmel_bandnorm_backward" in str(e.value)
    with pytest.raises(capi.DmelError) as e:
        capi.bandnorm_forward(p, 5, 2, 2, 3, None, p, p, True, True, 1e-5, 0.1, p, p, p, p, p, p, None)
    assert e.value.status == capi.DMEL_ERR_INVALID_ARGUMENT and "multiple of rows_per_clip" in str(e.value)
