"""BandNorm as torch restates it (CPU, any float dtype): the forward of include/dmel.h's dmel_bandnorm_forward with a mask, its hand-written
adjoint (dmel_bandnorm_backward's formulas), the cancellation-free scales the kernel's errors are measured in, and the inputs of the GPU tests.

  valid frames of clip b: t < Tc[b];   population of a statistic: the valid frames of one row (stats="clip") or of every row of a band ("batch")
  mu = mean s;  var = mean (s - mu)^2;  rstd = 1 / sqrt(var + eps);  yh = (s - mu) rstd;  y = yh weight[band] + bias[band];  0 on pad frames
  ds = weight rstd (g - mean g - yh mean(g yh))   (eval mode of the batch statistics: weight rstd g);   dweight = sum g yh;  dbias = sum g
  running_mean <- (1 - momentum) running_mean + momentum mu;  running_var <- (1 - momentum) running_var + momentum var n / (n - 1)

Tensors are (B, C, n_mels, T); parameters and buffers (n_mels,); ``Tc`` a (B,) integer tensor or None (every frame valid).  In fp32 this is the
mask tensor and the dozen launches a user would write today, and its own error against fp64 is the yardstick of tests/test_hip_bandnorm.py."""
import torch

import pcen_cases

EPS, MOMENTUM = 1e-5, 0.1
# the smallest shapes that reach each code path: one frame; packed rows of 2, 32 (31 of 32 lanes) and exactly 32 frames; one chunk short of
# 64, exactly 64, one frame into a second chunk; three and five chunks; channels; more than 64 rows per band (a second round of the combine's
# lanes: 70 and 130 rows); BASELINE config 2's rows
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 2), (2, 1, 7, 31), (4, 1, 4, 32), (2, 1, 3, 63), (1, 1, 6, 64), (2, 1, 3, 65), (1, 1, 2, 130), (2, 1, 1, 300),
          (2, 3, 5, 40), (70, 1, 2, 5), (130, 1, 1, 3), (4, 1, 128, 32)]


def valid_mask(shape, Tc):
    """(B, 1, 1, T) bool: t < Tc[b]"""
    B, T = shape[0], shape[-1]
    if Tc is None:
        return torch.ones(B, 1, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, :] < Tc.reshape(B, 1)).reshape(B, 1, 1, T)


def _population(s, Tc, stats):
    """(mask as s's dtype, the dims a statistic sums over, n per population broadcastable against the sums)"""
    B, C, M, T = s.shape
    m = valid_mask(s.shape, Tc)
    per_clip = (torch.full((B,), T) if Tc is None else Tc).to(s.dtype).reshape(B, 1, 1, 1)
    if stats == "clip":
        return m, (3,), per_clip
    return m, (0, 1, 3), (C * per_clip.sum()).reshape(1, 1, 1, 1)


def _band(p, like, fill):
    return (torch.full((like.shape[2],), fill, dtype=like.dtype) if p is None else p.to(like.dtype)).reshape(1, 1, -1, 1)


def moments(s, Tc, stats, eps=EPS):
    """(mu, var, rstd, n, s - mu), broadcastable against s; differentiable.  Taken on shifted data, d = s - pivot with the pivot the
    population's first frame (always valid): mu = pivot + mean d, s - mu = d - mean d.  Without the shift fp32 leaves mu a rounding of
    |mu| = 23 away under the log, a nearly silent row (var ~ eps) gets rstd wrong by 1e-4, and a silent one (d = 0 exactly here) gets
    yh ~ 4e-4 where the answer is 0."""
    m, dims, n = _population(s, Tc, stats)
    zero = torch.zeros((), dtype=s.dtype)
    pivot = (s[..., :1] if stats == "clip" else s[:1, :1, :, :1]).detach()
    d = s - pivot
    mean_d = torch.where(m, d, zero).sum(dim=dims, keepdim=True) / n
    centered = d - mean_d
    var = (torch.where(m, centered, zero) ** 2).sum(dim=dims, keepdim=True) / n
    return pivot + mean_d, var, 1 / torch.sqrt(var + eps), n, centered


def _standardised(s, Tc, stats, eps, running):
    """(mu, rstd, s - mu): of the batch or the clip, or from the running buffers (eval mode of the batch statistics)"""
    if running is None:
        mu, _, rstd, _, centered = moments(s, Tc, stats, eps)
        return mu, rstd, centered
    mu = _band(running[0], s, 0.0)
    return mu, 1 / torch.sqrt(_band(running[1], s, 1.0) + eps), s - mu


def forward(s, weight, bias, Tc, stats, eps=EPS, running=None):
    """y; differentiable (fp64 autograd through it is the reference of the hand-written adjoint).  ``running`` = (running_mean, running_var):
    eval mode of the batch statistics"""
    m = valid_mask(s.shape, Tc)
    _, rstd, centered = _standardised(s, Tc, stats, eps, running)
    yh = torch.where(m, centered * rstd, torch.zeros((), dtype=s.dtype))
    return torch.where(m, yh * _band(weight, s, 1.0) + _band(bias, s, 0.0), torch.zeros((), dtype=s.dtype))


def updated_running(s, Tc, running_mean, running_var, momentum=MOMENTUM, eps=EPS):
    """(running_mean, running_var, their scales) after one training forward of the batch statistics; the scales: every term of the mean by
    its magnitude, every squared deviation by (|s| + |mu|)^2"""
    m, dims, n = _population(s, Tc, "batch")
    mu, var, _, _, _ = moments(s, Tc, "batch", eps)
    zero = torch.zeros((), dtype=s.dtype)
    flat = lambda v: v.reshape(-1)      # noqa: E731
    rm, rv = running_mean.to(s.dtype), running_var.to(s.dtype)
    n1 = torch.clamp(n - 1, min=1)
    mean_abs = torch.where(m, s.abs(), zero).sum(dim=dims, keepdim=True) / n
    sq_abs = (torch.where(m, s.abs() + mu.abs(), zero) ** 2).sum(dim=dims, keepdim=True) / n1
    new_mean = (1 - momentum) * rm + momentum * flat(mu)
    new_var = (1 - momentum) * rv + momentum * flat(var * n / n1)
    if float(n) < 2:
        new_var = rv.clone()
    return new_mean, new_var, (1 - momentum) * rm.abs() + momentum * flat(mean_abs), (1 - momentum) * rv.abs() + momentum * flat(sq_abs)


def backward(g, s, weight, bias, Tc, stats, eps=EPS, running=None):
    """the adjoint as the issue writes it: a dict with y, ds (like s), dweight, dbias ((n_mels,) each) and the scales ``*_scale``:
    y ((|s| + |mu|) rstd |weight| + |bias|), ds (|weight| rstd (|g| + mean|g| + |yh| mean|g yh|)), dweight (sum |g yh|), dbias (sum |g|);
    every scale is 0 on a pad frame"""
    m, dims, n = _population(s, Tc, stats)
    zero = torch.zeros((), dtype=s.dtype)
    w, b = _band(weight, s, 1.0), _band(bias, s, 0.0)
    mu, rstd, centered = _standardised(s, Tc, stats, eps, running)
    yh = torch.where(m, centered * rstd, zero)
    gm = torch.where(m, g, zero)
    mean = lambda v: v.sum(dim=dims, keepdim=True) / n      # noqa: E731
    if running is None:
        ds = w * rstd * (gm - mean(gm) - yh * mean(gm * yh))
        ds_scale = w.abs() * rstd * (gm.abs() + mean(gm.abs()) + yh.abs() * mean((gm * yh).abs()))
    else:
        ds = w * rstd * gm
        ds_scale = w.abs() * rstd * gm.abs()
    band = (0, 1, 3)
    return {"y": torch.where(m, yh * w + b, zero), "y_scale": torch.where(m, (s.abs() + mu.abs()) * rstd * w.abs() + b.abs(), zero),
            "ds": torch.where(m, ds, zero), "ds_scale": torch.where(m, ds_scale, zero),
            "dweight": (gm * yh).sum(dim=band), "dweight_scale": (gm * yh).abs().sum(dim=band),
            "dbias": gm.sum(dim=band), "dbias_scale": gm.abs().sum(dim=band)}


worst = pcen_cases.worst      # max |got - ref| / scale; an element whose scale is 0 must be exact


def params(n_mels, seed, dtype=torch.float32):
    """weight (both signs, away from 0), bias, and the running buffers an eval-mode test starts from, per band"""
    gen = torch.Generator().manual_seed(2000 + seed)
    u = lambda: torch.rand(n_mels, generator=gen, dtype=torch.float64)      # noqa: E731
    weight = (0.25 + 1.5 * u()) * torch.where(u() < 0.3, -1.0, 1.0)
    bias = torch.randn(n_mels, generator=gen, dtype=torch.float64)
    running_mean = -8.0 + 3.0 * torch.randn(n_mels, generator=gen, dtype=torch.float64)
    running_var = 0.5 + 20.0 * u()
    return tuple(p.to(torch.float32).to(dtype) for p in (weight, bias, running_mean, running_var))


def inputs(shape, seed):
    """(s, g) fp32 of ``shape``: s = log(E + 1e-10) with E drawn as pcen_cases.inputs draws it (row 0 is silence: the constant log(1e-10);
    the last row falls silent at frame T // 3)"""
    E, g = pcen_cases.inputs(shape, seed)
    return torch.log(E.double() + 1e-10).to(torch.float32), g


def frame_lengths(shape, seed):
    """(B,) int64: Tc[0] = T, Tc[-1] = max(1, T // 3) (in that order: a single clip gets the short length), the rest random in 1 ... T"""
    B, T = shape[0], shape[-1]
    gen = torch.Generator().manual_seed(3000 + seed)
    Tc = torch.randint(1, T + 1, (B,), generator=gen)
    Tc[0] = T
    Tc[-1] = max(1, T // 3)
    return Tc
