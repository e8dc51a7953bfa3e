"""StatsPool as torch restates it (CPU, any float dtype), the cancellation-free scales the kernel's errors are measured in, and the cases of
the GPU tests.

  Tc = frame_lengths[b] (None: T);  over the valid frames t < Tc of every row (clip, channel, band):
  mean  mu = sum s[t] / Tc            std  sd = sqrt(sum (s[t] - mu)^2 / Tc + eps)            max  s[am]
  am by the order: a NaN beats a non-NaN, then the larger value wins, then the lower t (-0.0 and +0.0 tie)
  y = cat([mean, std, max], dim=1) of the selected statistics (``which``: bit 0 mean, bit 1 std, bit 2 max), (B, S C, M)

The restatement goes clip by clip on ``s[b, ..., :Tc]``: ``mean(-1)``, ``sqrt(var(-1, unbiased=False) + eps)`` and the maximum through an
explicit index ``am`` (a gather, whose adjoint is the one-hot of ``am``).  It is differentiable: fp64 autograd through it is the reference of the backward.  ``over_all_T=True`` is the
defect the stage removes: the statistics are taken over all T frames of the batch."""
import functools

import torch

EPS = 1e-5
# the shortest rows (1, 2, 3, 5); the packing boundary (31, 32, 33); the chunk boundary (63, 64, 65); more chunks (130, 300); row counts that
# leave a wave partly filled, channels, many rows and BASELINE config 2's rows
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 2), (2, 1, 2, 3), (2, 1, 2, 5), (2, 1, 7, 31), (4, 1, 4, 32), (2, 1, 3, 33), (2, 1, 3, 63),
          (1, 1, 6, 64), (2, 1, 3, 65), (1, 1, 2, 130), (2, 1, 1, 300), (2, 3, 5, 40), (70, 1, 2, 5), (4, 1, 128, 32)]
NAMES = ("mean", "std", "max")
POOL_SIZE = 8


def pool(T):
    """the lengths the cases draw from, before the clamp to 1 ... T"""
    return [T, 1, 2, 63, 64, 65, T - 1, T // 2]


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for given in (False, True):
            out.append(dict(shape=shape, which=7, given=given))
        if si % 4 == 0:                                            # each single statistic, and mean + max
            out += [dict(shape=shape, which=w, given=True) for w in (1, 2, 4, 5)]
    for i, c in enumerate(out):
        B, C, M, T = c["shape"]
        p = pool(T)
        c["index"] = i
        c["entries"] = [(i + b) % POOL_SIZE for b in range(B)]
        c["Tc"] = [min(max(p[e], 1), T) for e in c["entries"]] if c.pop("given") else None
        c["kind"] = "log" if i % 2 == 0 else "linear"
        c["rows"] = _plant_rows(c)
    return out


def lengths_of(c):
    return list(c["Tc"]) if c["Tc"] is not None else [c["shape"][3]] * c["shape"][0]


def _plant_rows(c):
    """the rows (of the B C M of the case) that carry the plants: ``neg`` the last row of the shortest clip (its valid maximum is negative;
    +0.0 and larger values stand in its pad frames), ``const`` the first row of the clip behind it (constant over its valid frames), ``tie``
    the first other row (its maximum stands at two frames); with two rows the tie shares the negative row, with one there is ``const`` only"""
    B, C, M, T = c["shape"]
    R, cm, Tc = B * C * M, C * M, lengths_of(c)
    bneg = min(range(B), key=lambda b: (Tc[b], b))
    const = ((bneg + 1) % B) * cm
    neg = bneg * cm + cm - 1
    if neg == const:
        return dict(const=const, neg=None, tie=None)
    others = [r for r in range(R) if r not in (const, neg)]
    return dict(const=const, neg=neg, tie=others[0] if others else neg)


CASES = _cases()


def case_id(c):
    return "x".join(str(v) for v in c["shape"]) + f"-w{c['which']}-{'len' if c['Tc'] else 'full'}"


def selected(which):
    return [k for i, k in enumerate(NAMES) if which >> i & 1]


def split(y, which, C):
    """{name: (B, C, M)} of a (B, S C, M) tensor"""
    return {k: y[:, o * C:(o + 1) * C] for o, k in enumerate(selected(which))}


def valid_mask(shape, Tc):
    """(B, 1, 1, T) bool: t < Tc[b]"""
    B, T = shape[0], shape[-1]
    if Tc is None:
        return torch.ones(B, 1, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, :] < torch.as_tensor(Tc).reshape(B, 1)).reshape(B, 1, 1, T)


def pad_fraction(c):
    """the largest share of pad frames among the clips of the case"""
    T = c["shape"][3]
    return max((T - t) / T for t in lengths_of(c))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def argmax_by_the_order(x):
    """index over the last axis: the first NaN if there is one, else the first frame that holds the largest value (-0.0 == +0.0)"""
    n = x.shape[-1]
    t = torch.arange(n).expand(x.shape)
    nan = torch.isnan(x)
    first_nan = torch.where(nan, t, n).amin(-1)
    top = torch.where(nan, torch.full_like(x, float("-inf")), x).amax(-1, keepdim=True)
    first_top = torch.where(x == top, t, n).amin(-1)
    return torch.where(first_nan < n, first_nan, first_top)


def forward(s, Tc, which=7, eps=EPS, over_all_T=False):
    """(y (B, S C, M), am (B, C, M) int64) from s (B, C, M, T), clip by clip at the clip's own length; differentiable in s"""
    B, C, M, T = s.shape
    groups = {k: [] for k in NAMES}
    ams = []
    for b in range(B):
        tc = T if Tc is None or over_all_T else int(Tc[b])
        x = s[b, :, :, :tc]
        am = argmax_by_the_order(x.detach())
        groups["mean"].append(x.mean(-1))
        groups["std"].append(torch.sqrt(x.var(-1, unbiased=False) + eps))
        # s[am] picked by the index found above, as a word (-0.0 and NaN payloads survive); its adjoint is the one-hot of am: the cotangent
        # is scattered to frame am alone, whatever torch.max would do with a tie
        groups["max"].append(x.gather(-1, am.unsqueeze(-1)).squeeze(-1))
        ams.append(am)
    return torch.cat([torch.stack(groups[k]) for k in selected(which)], dim=1), torch.stack(ams)


def reference(s, g, Tc, which, eps=EPS):
    """fp64: y, am, ds by autograd through the restatement, and the cancellation-free scales: mean|s| for the mean, sd itself for the std
    (its radicand is a sum of non-negative terms), |g_mean| / Tc + |g_std| |s - mu| / (Tc sd) + [t == am] |g_max| for ds (0 on pad frames)"""
    B, C, M, T = s.shape
    s64 = s.double().clone().requires_grad_(True)
    y, am = forward(s64, Tc, which, eps)
    (ds,) = torch.autograd.grad(y, [s64], g.double())
    full, _ = forward(s.double(), Tc, 7, eps)
    mu, sd = full[:, :C], full[:, C:2 * C]
    valid = valid_mask(s.shape, Tc).expand(s.shape)
    tcs = torch.tensor([T if Tc is None else int(t) for t in Tc or [T] * B], dtype=torch.float64).reshape(B, 1, 1, 1)
    mean_abs = torch.where(valid, s.double().abs(), torch.zeros((), dtype=torch.float64)).sum(-1) / tcs[..., 0]
    ga = split(g.double().abs(), which, C)
    zero = torch.zeros(s.shape, dtype=torch.float64)
    ds_scale = zero.clone()
    if "mean" in ga:
        ds_scale = ds_scale + ga["mean"][..., None] / tcs
    if "std" in ga:
        ds_scale = ds_scale + ga["std"][..., None] * (s.double() - mu[..., None]).abs() / (tcs * sd[..., None])
    if "max" in ga:
        ds_scale = ds_scale + torch.nn.functional.one_hot(am, T).double() * ga["max"][..., None]
    ds_scale = torch.where(valid, ds_scale, zero)
    return dict(y=y.detach(), am=am, ds=ds.detach(), scale=dict(mean=mean_abs, std=sd), ds_scale=ds_scale)


def restatement32(s, g, Tc, which, eps=EPS):
    """the fp32 torch restatement: y and ds by autograd"""
    x = s.clone().requires_grad_(True)
    y, _ = forward(x, Tc, which, eps)
    (ds,) = torch.autograd.grad(y, [x], g)
    return dict(y=y.detach(), ds=ds)


def worst(got, ref64, scale64, exact_zeros=True):
    """max |got - ref| / scale; with ``exact_zeros`` an element whose scale is 0 must compare equal to 0 (the kernel's results; the fp32
    restatement's such elements are left out of the maximum)"""
    got = torch.as_tensor(got).double()
    err = (got - ref64).abs()
    pos = scale64 > 0
    if exact_zeros:
        assert bool((got[~pos] == 0).all()), "an element with zero scale does not compare equal to 0"
    return float((err[pos] / scale64[pos]).max()) if bool(pos.any()) else 0.0


def errors(got_y, got_ds, ref, c, exact_zeros=True):
    """{quantity: worst error in units of its scale} of the selected mean and std and of ds (None: left out)"""
    C = c["shape"][1]
    parts, refs = split(got_y, c["which"], C), split(ref["y"], c["which"], C)
    out = {k: worst(parts[k], refs[k], ref["scale"][k], exact_zeros) for k in ("mean", "std") if k in parts}
    if got_ds is not None:
        out["ds"] = worst(got_ds, ref["ds"], ref["ds_scale"], exact_zeros)
    return out


def bounds(r32, ref, c):
    """(bounds, the fp32 restatement's worst errors) per quantity: 8 x the worst error of the fp32 torch restatement on this case, capped at
    1e-4, the project's parity bar (BandNorm's rule: an fp64-inside kernel should sit at or below the fp32 restatement, and 8 x leaves
    room for a different summation order)"""
    w = errors(r32["y"], r32["ds"], ref, c, exact_zeros=False)
    return {k: min(8.0 * v, 1e-4) for k, v in w.items()}, w


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """(s, g) fp32: s (B, C, M, T) = log(1e-4 z^2 + 1e-10) (rows of mean about -10: the cancellation in the variance) or z^2, z a seeded
    normal; its pad frames hold what a layer writes behind a short clip (log(1e-10), or 0); then the plants of ``c["rows"]``;
    g (B, S C, M) a seeded normal n pushed away from zero, sign(n) (0.25 + |n|): the cotangents of a row's groups are of like magnitude, as
    behind a linear head.  (The scale of ds is free of cancellation for an evaluation that holds mu unrounded, as the kernel and the fp64
    restatement do; the fp32 restatement forms s - mu from an fp32 mu, an absolute error of about ulp(10) / 2 under the log, which the
    term |g_std| |s - mu| covers only with the help of |g_mean| / Tc: with g_mean a thousand times smaller than g_std it alone passes 1e-4.)"""
    gen = torch.Generator().manual_seed(7000 + c["index"])
    z = torch.randn(c["shape"], generator=gen, dtype=torch.float64)
    B, C, M, T = c["shape"]
    m = valid_mask(c["shape"], c["Tc"])
    e = torch.where(m, z * z, torch.zeros((), dtype=torch.float64))
    s = (torch.log(1e-4 * e + 1e-10) if c["kind"] == "log" else e).to(torch.float32)
    n = torch.randn((B, len(selected(c["which"])) * C, M), generator=gen, dtype=torch.float64)
    g = (torch.where(n < 0, -1.0, 1.0) * (0.25 + n.abs())).to(torch.float32)
    rows, Tc, cm = s.view(B * C * M, T), lengths_of(c), C * M
    r = c["rows"]
    # (a multiple of 1 / 64: its partial sums are exact in fp32 too, so the fp32 restatement sees a constant row as the kernel does; with an
    # fp32 mean one ulp(10) off it finds deviations of 1e-6 over sd = sqrt(eps) = 3e-3.  The GPU tests also run constants of full precision)
    rows[r["const"], :Tc[r["const"] // cm]] = torch.round(rows[r["const"], 0] * 64.0) / 64.0
    if r["neg"] is not None:
        tc = Tc[r["neg"] // cm]
        rows[r["neg"], :tc] = -rows[r["neg"], :tc].abs() - 1.0
        rows[r["neg"], tc:] = torch.tensor([0.0, 5.0])[torch.arange(T - tc) % 2]
    if r["tie"] is not None:
        tc = Tc[r["tie"] // cm]
        if tc >= 2:
            t1 = int(rows[r["tie"], :tc].argmax())
            t2 = (t1 + max(tc // 2, 1)) % tc
            rows[r["tie"], t2] = rows[r["tie"], t1]
    return s, g


@functools.lru_cache(maxsize=None)
def case_reference(index):
    """(s, g, fp64 reference, fp32 restatement) of case ``index``, computed once and shared (callers leave them unchanged)"""
    c = CASES[index]
    s, g = inputs(c)
    return s, g, reference(s, g, c["Tc"], c["which"]), restatement32(s, g, c["Tc"], c["which"])


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
