"""Deltas as torch restates it (CPU, any float dtype), the fp32 numpy evaluation of the arithmetic include/dmel.h specifies, the
cancellation-free scales the kernel's errors are measured in, the bounds, and the cases of the GPU tests.

  n = (win_length - 1) / 2,  denom = n (n + 1) (2 n + 1) / 3,  Tc = frame_lengths[b] (None: T)
  for t <  Tc:   d[t]  = ( sum_{j = 1 .. n} j (x[min(t + j, Tc - 1)] - x[max(t - j, 0)]) ) / denom;   dd = the same on d[0 .. Tc - 1]
  for t >= Tc:   d[t] = dd[t] = 0
  y = cat([s, d, dd], dim=1) (without s: include_static=False; without dd: order=1);   ds = g_static + D^T (g_d + D^T g_dd)

The restatement goes clip by clip: slice ``[..., :Tc]``, ``F.pad(mode="replicate")``, ``F.conv1d`` with ``arange(-n, n + 1) / denom``, twice.  It
is differentiable: fp64 autograd through it is the reference of the backward.  The scales are the same two stencils with ``|j|`` on ``|s|`` and
their adjoint on ``|g|``."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# rows shorter than one and two halos (1 ... 9); the packing boundary (31, 32, 33); 64 minus four halos for each n, plus or minus one (47 ...
# 49, 56, 57, 60, 61: the chunk steps 48, 56, 60 of win_length 9, 5, 3) and the chunk boundary (63 ... 65); two, three and five chunks
# (113, 130, 300); channels; many rows; BASELINE config 2's rows
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 2), (2, 1, 3, 3), (2, 1, 2, 4), (2, 1, 2, 5), (2, 1, 3, 9), (2, 1, 7, 31), (4, 1, 4, 32), (2, 1, 3, 33),
          (2, 1, 3, 47), (2, 1, 2, 48), (2, 1, 2, 49), (2, 1, 3, 56), (2, 1, 3, 57), (2, 1, 3, 60), (2, 1, 3, 61), (2, 1, 3, 63), (1, 1, 6, 64),
          (2, 1, 3, 65), (1, 1, 2, 113), (1, 1, 2, 130), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5), (4, 1, 128, 32)]
WIN_LENGTHS = (3, 5, 9)
POOL_SIZE = 11


def half(win_length):
    return (win_length - 1) // 2


def denom(win_length):
    n = half(win_length)
    return n * (n + 1) * (2 * n + 1) // 3


def pool(T, n):
    """the lengths the cases draw from, before the clamp to 1 ... T"""
    return [T, 1, 2, n, n + 1, 2 * n, 2 * n + 1, 4 * n, 4 * n + 1, T - 1, T // 2]


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        variants = [(2, True)] + ([(1, True), (2, False)] if si % 4 == 0 else [])
        for order, static in variants:
            for win in WIN_LENGTHS:
                for given in ((False, True) if (order, static) == (2, True) else (True,)):
                    out.append(dict(shape=shape, win_length=win, order=order, include_static=static, given=given))
    for i, c in enumerate(out):
        B, T = c["shape"][0], c["shape"][3]
        p = pool(T, half(c["win_length"]))
        c["index"] = i
        c["entries"] = [(i + b) % POOL_SIZE for b in range(B)]
        c["Tc"] = [min(max(p[e], 1), T) for e in c["entries"]] if c.pop("given") else None
        c["kind"] = "log" if i % 2 == 0 else "linear"
    return out


CASES = _cases()


def case_id(c):
    return "x".join(str(v) for v in c["shape"]) + f"-w{c['win_length']}-o{c['order']}-{'s' if c['include_static'] else 'n'}-{'len' if c['Tc'] else 'full'}"


def groups(c):
    return int(c["include_static"]) + c["order"]


def lengths_of(c):
    return list(c["Tc"]) if c["Tc"] is not None else [c["shape"][3]] * c["shape"][0]


def valid_mask(shape, Tc):
    """(B, 1, 1, T) bool: t < Tc[b]"""
    B, T = shape[0], shape[-1]
    if Tc is None:
        return torch.ones(B, 1, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, :] < torch.as_tensor(Tc).reshape(B, 1)).reshape(B, 1, 1, T)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def stencil(x, win_length, absolute=False):
    """one application over the last axis of x (every frame valid): replicate padding, then the correlation with arange(-n, n + 1) / denom
    (``absolute``: with |j| / denom, the stencil of the scales)"""
    n = half(win_length)
    k = torch.arange(-n, n + 1, dtype=x.dtype) / denom(win_length)
    if absolute:
        k = k.abs()
    flat = F.pad(x.reshape(-1, 1, x.shape[-1]), (n, n), mode="replicate")
    return F.conv1d(flat, k.reshape(1, 1, -1)).reshape(x.shape)


def forward(s, Tc, win_length=5, order=2, include_static=True, absolute=False, edge_at_T=False):
    """(B, G C, M, T) from s (B, C, M, T), clip by clip at the clip's own length, zeros on pad frames; differentiable.  ``edge_at_T`` is the
    defect the stage removes: the stencil runs over all T frames of the batch (its edge at T - 1) and the pad frames are zeroed afterwards."""
    B, C, M, T = s.shape
    d, dd = torch.zeros_like(s), torch.zeros_like(s)
    for b in range(B):
        tc = T if Tc is None else int(Tc[b])
        x = s[b] if edge_at_T else s[b, :, :, :tc]
        db = stencil(x, win_length, absolute)
        ddb = stencil(db, win_length, absolute)
        d[b, :, :, :tc], dd[b, :, :, :tc] = db[..., :tc], ddb[..., :tc]
    parts = ([s] if include_static else []) + [d] + ([dd] if order == 2 else [])
    return torch.cat(parts, dim=1)


def reference(s, g, Tc, win_length, order, include_static):
    """fp64: y, ds by autograd through the restatement, and the scales of both (the static group's scale is |s|: it is moved, compared by bits)"""
    s64 = s.double().clone().requires_grad_(True)
    y = forward(s64, Tc, win_length, order, include_static)
    (ds,) = torch.autograd.grad(y, [s64], g.double())
    a64 = s.double().clone().requires_grad_(True)
    (ds_scale,) = torch.autograd.grad(forward(a64, Tc, win_length, order, include_static, absolute=True), [a64], g.double().abs())      # the stencils with |j| are linear: their adjoint on |g|
    y_scale = forward(s.double().abs(), Tc, win_length, order, include_static, absolute=True)
    return dict(y=y.detach(), ds=ds.detach(), y_scale=y_scale, ds_scale=ds_scale)


# ---- the arithmetic of the specification in fp32 numpy ---------------------------------------------------------------------------------------
def spec_rows(x, win_length):
    """x (rows, Tc) float32, every frame valid: the antisymmetric form -- a difference first, j times it second, summed in fp32 for
    j = 1 ... n, divided by denom -- every operation rounded to fp32"""
    assert x.dtype == np.float32
    n, Tc = half(win_length), x.shape[-1]
    t = np.arange(Tc)
    acc = np.zeros_like(x)
    for j in range(1, n + 1):
        acc = acc + np.float32(j) * (x[:, np.minimum(t + j, Tc - 1)] - x[:, np.maximum(t - j, 0)])
    return acc / np.float32(denom(win_length))


def spec_forward(s, Tc, win_length, order=2):
    """(d, dd) float32 arrays like s (numpy, (B, C, M, T)); dd from the stored fp32 d; +0.0 on pad frames"""
    B, C, M, T = s.shape
    d, dd = np.zeros_like(s), np.zeros_like(s)
    for b in range(B):
        tc = T if Tc is None else int(Tc[b])
        rows = spec_rows(np.ascontiguousarray(s[b, :, :, :tc]).reshape(C * M, tc), win_length)
        d[b, :, :, :tc] = rows.reshape(C, M, tc)
        if order == 2:
            dd[b, :, :, :tc] = spec_rows(rows, win_length).reshape(C, M, tc)
    return d, dd


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
def bounds(win_length):
    """in units of the scales: d (3 n + 1) u -- one rounding per difference, per product by j and per addition, one for the division --, dd
    twice that (its input carries d's error), ds (2 m + 6) u with m = 2 n + n (n + 1) / 2"""
    n = half(win_length)
    m = 2 * n + n * (n + 1) // 2
    return dict(d=(3 * n + 1) * U, dd=2 * (3 * n + 1) * U, ds=(2 * m + 6) * U)


def worst(got, ref64, scale64):
    """max |got - ref| / scale; an element whose scale is 0 must be an exact zero"""
    got = torch.as_tensor(got).double()
    err = (got - ref64).abs()
    pos = scale64 > 0
    assert bool((got[~pos] == 0).all()), "an element with zero scale is not an exact zero"
    return float((err[pos] / scale64[pos]).max()) if bool(pos.any()) else 0.0


def split(y, c):
    """(static or None, d, dd or None) of a (B, G C, M, T) tensor or array"""
    C = c["shape"][1]
    k = int(c["include_static"])
    return (y[:, :C] if k else None), y[:, k * C:(k + 1) * C], (y[:, (k + 1) * C:(k + 2) * C] if c["order"] == 2 else None)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """(s, g) fp32: s (B, C, M, T) = log(10 z^2 + 1e-10) (a large common offset) or z^2, z a seeded normal; its pad frames hold what a
    layer writes behind a short clip (log(1e-10), or 0); g (B, G C, M, T) a seeded normal"""
    gen = torch.Generator().manual_seed(5000 + c["index"])
    z = torch.randn(c["shape"], generator=gen, dtype=torch.float64)
    B, C, M, T = c["shape"]
    m = valid_mask(c["shape"], c["Tc"])
    e = torch.where(m, z * z, torch.zeros((), dtype=torch.float64))
    s = torch.log(10.0 * e + 1e-10) if c["kind"] == "log" else e
    g = torch.randn((B, groups(c) * C, M, T), generator=gen, dtype=torch.float64)
    return s.to(torch.float32), g.to(torch.float32)


@functools.lru_cache(maxsize=None)
def case_reference(index):
    """(s, g, fp64 reference) of case ``index``, computed once and shared (callers leave them unchanged)"""
    c = CASES[index]
    s, g = inputs(c)
    return s, g, reference(s, g, c["Tc"], c["win_length"], c["order"], c["include_static"])


PAD_PATTERN = (0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0x00000001)     # NaNs with payloads, -0.0, +inf, a denormal


def planted(t, Tc, pattern=PAD_PATTERN):
    """a copy of t (B, *, *, T) with the words of ``pattern`` in turn on every pad frame"""
    out = t.clone()
    if Tc is None:
        return out
    bits = out.view(torch.int32)
    words = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in pattern], dtype=torch.int32)
    for b, tc in enumerate(Tc):
        n = bits[b, :, :, tc:].numel()
        if n:
            bits[b, :, :, tc:] = words[torch.arange(n) % len(words)].reshape(bits[b, :, :, tc:].shape)
    return out
