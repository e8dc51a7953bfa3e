"""AttentivePool as torch restates it (CPU, any float dtype), the cancellation-free scales the kernel's errors are measured in, and the cases
of the GPU tests.

  s (B, C, M, T), logits a (B, A, T), A divides R = C M, row r of a clip reads logit row r / (R / A);  Tc = frame_lengths[b] (None: T)
  over the valid frames t < Tc:   w = softmax(a[:Tc])   mu = sum w s   var = sum w (s - mu)^2   sd = sqrt(var + eps)
  y = cat([mean, std], dim=1) of the selected statistics (``which``: bit 0 mean, bit 1 std), (B, S C, M)

The restatement goes clip by clip on ``s[b, ..., :Tc]`` and ``a[b, :, :Tc]`` with ``torch.softmax``; it is differentiable in both, and fp64
autograd through it is the reference of the backward.  The mean is evaluated as ``s[0] + sum w (s - s[0])`` -- the same number, and the form
in which a constant row is a constant in fp32 as well (``sum w c`` with fp32 weights that add up to 1 - 6e-8 is not ``c``, and a deviation of
one ulp(10) over sd = sqrt(eps) = 3e-3 would put the fp32 restatement's ds of the constant row at 3e-4 of its scale, above the cap of the
bounds it is there to set).  ``over_all_T=True`` is the defect the stage removes: the softmax and the statistics over all T frames.

Shapes, the pool of lengths and its rule are tests/statspool_cases.py's."""
import functools

import torch

import statspool_cases as SP
from statspool_cases import EPS, PAD_PATTERN, SHAPES, POOL_SIZE, lengths_of, pad_fraction, planted, pool, selected, split, valid_mask, worst  # noqa: F401

NAMES = ("mean", "std")
QUANTITIES = ("mean", "std", "ds", "da")


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        R = shape[1] * shape[2]
        for given in (False, True):
            out.append(dict(shape=shape, which=3, A=1, form="shared", given=given))
        if si % 4 == 0:                                            # each single statistic, and one attention per band, with and without lengths
            out += [dict(shape=shape, which=w, A=A, form=f, given=True) for w, A, f in ((1, 1, "shared"), (2, 1, "shared"), (3, R, "band"))]
            out.append(dict(shape=shape, which=3, A=R, form="band", given=False))
        if shape == (2, 3, 5, 40):                                 # one attention per channel
            out.append(dict(shape=shape, which=3, A=3, form="channel", given=True))
    for i, c in enumerate(out):
        B, C, M, T = c["shape"]
        p = pool(T)
        c["index"] = i
        c["entries"] = [(i + b) % POOL_SIZE for b in range(B)]
        c["Tc"] = [min(max(p[e], 1), T) for e in c["entries"]] if c.pop("given") else None
        c["kind"] = "log" if i % 2 == 0 else "linear"
        Tc = lengths_of(c)
        short = min(range(B), key=lambda b: (Tc[b], b))
        c["const"] = ((short + 1) % B) * C * M                      # the first row of the clip behind the shortest one: constant over its valid frames
        two = [b for b in range(B) if Tc[b] >= 2]
        c["ninf"] = (two[0], (c["A"] - 1) // 2, Tc[two[0]] // 2) if two else None      # (clip, logit row, frame) of the -inf logit
    return out


CASES = _cases()


def case_id(c):
    return "x".join(str(v) for v in c["shape"]) + f"-w{c['which']}-{c['form']}{c['A']}-{'len' if c['Tc'] else 'full'}"


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def forward(s, a, Tc, which=3, eps=EPS, over_all_T=False):
    """(y (B, S C, M), mu (B, C, M), var (B, C, M)) from s (B, C, M, T) and a (B, A, T), clip by clip at the clip's own length;
    differentiable in s and a"""
    B, C, M, T = s.shape
    A = a.shape[1]
    group = C * M // A
    mus, vars_ = [], []
    for b in range(B):
        tc = T if Tc is None or over_all_T else int(Tc[b])
        x = s[b, :, :, :tc]
        w = torch.softmax(a[b, :, :tc], -1).repeat_interleave(group, dim=0).reshape(C, M, tc)
        x0 = x[..., :1].detach()
        mu = x0[..., 0] + (w * (x - x0)).sum(-1)
        d = x - mu.unsqueeze(-1)
        mus.append(mu)
        vars_.append((w * d * d).sum(-1))
    mu, var = torch.stack(mus), torch.stack(vars_)
    groups = dict(mean=mu, std=torch.sqrt(var + eps))
    return torch.cat([groups[k] for k in selected(which)], dim=1), mu, var


def weights(a, Tc):
    """(w (B, A, T) zero on pad frames, m (B, A), Z (B, A)) of the softmax over the valid frames, in a's dtype"""
    B, A, T = a.shape
    w, m, Z = torch.zeros_like(a), [], []
    for b in range(B):
        tc = T if Tc is None else int(Tc[b])
        mb = a[b, :, :tc].amax(-1)
        pb = torch.exp(a[b, :, :tc] - mb[:, None])
        m.append(mb), Z.append(pb.sum(-1))
        w[b, :, :tc] = pb / pb.sum(-1, keepdim=True)
    return w, torch.stack(m), torch.stack(Z)


def reference(s, a, g, Tc, which, eps=EPS):
    """fp64: y, ds and da by autograd through the restatement, stats (rows, 2) = (mu, var), norm (B A, 2) = (m, Z) and the cancellation-free
    scales -- each quantity's formula with every term replaced by its absolute value: sum w |s| for the mean, sd for the std,
    w (|g_mean| + |g_std| |d| / sd) for ds and w sum_r (|g_mean| |d| + |g_std| (d^2 + var) / (2 sd)) for da (0 on pad frames)"""
    B, C, M, T = s.shape
    A = a.shape[1]
    group = C * M // A
    s64, a64 = s.double().clone().requires_grad_(True), a.double().clone().requires_grad_(True)
    y, mu, var = forward(s64, a64, Tc, which, eps)
    ds, da = torch.autograd.grad(y, [s64, a64], g.double())
    mu, var = mu.detach(), var.detach()
    sd = torch.sqrt(var + eps)
    w, m, Z = weights(a.double(), Tc)
    wr = w.repeat_interleave(group, dim=1).reshape(B, C, M, T)
    valid = valid_mask(s.shape, Tc).expand(s.shape)
    zero = torch.zeros((), dtype=torch.float64)
    sv = torch.where(valid, s.double(), zero)                       # (pad frames may hold anything: they are not part of any formula)
    d = torch.where(valid, sv - mu[..., None], zero)
    ga = split(g.double().abs(), which, C)
    gm = ga.get("mean", torch.zeros(B, C, M, dtype=torch.float64))[..., None]
    gs = ga.get("std", torch.zeros(B, C, M, dtype=torch.float64))[..., None]
    ds_scale = wr * (gm + gs * d.abs() / sd[..., None])
    bracket = torch.where(valid, gm * d.abs() + gs * (d * d + var[..., None]) / (2.0 * sd[..., None]), zero)
    da_scale = w * bracket.reshape(B, A, group, T).sum(2)
    return dict(y=y.detach(), ds=ds.detach(), da=da.detach(), stats=torch.stack([mu.reshape(-1), var.reshape(-1)], dim=1),
                norm=torch.stack([m.reshape(-1), Z.reshape(-1)], dim=1), w=w,
                scale=dict(mean=(wr * sv.abs()).sum(-1), std=sd), ds_scale=ds_scale, da_scale=da_scale)


def restatement32(s, a, g, Tc, which, eps=EPS):
    """the fp32 torch restatement: y, ds and da by autograd"""
    x, l = s.clone().requires_grad_(True), a.clone().requires_grad_(True)
    y, _, _ = forward(x, l, Tc, which, eps)
    ds, da = torch.autograd.grad(y, [x, l], g)
    return dict(y=y.detach(), ds=ds, da=da)


def errors(got_y, got_ds, got_da, ref, c, exact_zeros=True):
    """{quantity: worst error in units of its scale} of the selected mean and std, of ds and of da (None: left out); with ``exact_zeros``
    an element whose scale is 0 must compare equal to 0"""
    C = c["shape"][1]
    parts, refs = split(got_y, c["which"], C), split(ref["y"], c["which"], C)
    out = {k: worst(parts[k], refs[k], ref["scale"][k], exact_zeros) for k in NAMES if k in parts}
    if got_ds is not None:
        out["ds"] = worst(got_ds, ref["ds"], ref["ds_scale"], exact_zeros)
    if got_da is not None:
        out["da"] = worst(got_da, ref["da"], ref["da_scale"], exact_zeros)
    return out


def bounds(r32, ref, c):
    """(bounds, the fp32 restatement's worst errors) per quantity: 8 x the worst error of the fp32 torch restatement on this case, capped at
    1e-4, the project's parity bar (BandNorm's and StatsPool's rule)"""
    w = errors(r32["y"], r32["ds"], r32["da"], ref, c, exact_zeros=False)
    return {k: min(8.0 * v, 1e-4) for k, v in w.items()}, w


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """(s, a, g) fp32: s (B, C, M, T) = log(1e-4 z^2 + 1e-10) or z^2, z a seeded normal, its pad frames what a layer writes behind a short
    clip (log(1e-10), or 0), with the constant row ``c["const"]`` (a multiple of 1 / 64 over its valid frames); a (B, A, T) = 2 n, n a
    seeded normal on EVERY frame (a scorer sees the pad frames too), with -inf at ``c["ninf"]``; g (B, S C, M) a seeded normal pushed away
    from zero, sign(n) (0.25 + |n|)"""
    gen = torch.Generator().manual_seed(9000 + c["index"])
    B, C, M, T = c["shape"]
    z = torch.randn(c["shape"], generator=gen, dtype=torch.float64)
    e = torch.where(valid_mask(c["shape"], c["Tc"]), z * z, torch.zeros((), dtype=torch.float64))
    s = (torch.log(1e-4 * e + 1e-10) if c["kind"] == "log" else e).to(torch.float32)
    a = (2.0 * torch.randn((B, c["A"], T), generator=gen, dtype=torch.float64)).to(torch.float32)
    n = torch.randn((B, len(selected(c["which"])) * C, M), generator=gen, dtype=torch.float64)
    g = (torch.where(n < 0, -1.0, 1.0) * (0.25 + n.abs())).to(torch.float32)
    rows, Tc, k = s.view(B * C * M, T), lengths_of(c), c["const"]
    rows[k, :Tc[k // (C * M)]] = torch.round(rows[k, 0] * 64.0) / 64.0
    if c["ninf"] is not None:
        b, r, t = c["ninf"]
        a[b, r, t] = float("-inf")
    return s, a, g


@functools.lru_cache(maxsize=None)
def case_reference(index):
    """(s, a, g, fp64 reference, fp32 restatement) of case ``index``, computed once and shared (callers leave them unchanged)"""
    c = CASES[index]
    s, a, g = inputs(c)
    return s, a, g, reference(s, a, g, c["Tc"], c["which"]), restatement32(s, a, g, c["Tc"], c["which"])
