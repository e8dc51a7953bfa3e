"""PCEN as torch restates it (CPU, any float dtype): the forward of include/dmel.h's dmel_pcen_forward, its hand-written adjoint
(dmel_pcen_backward's formulas), the cancellation-free scales the kernel's errors are measured in, and the inputs of the GPU tests.

  M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t];   D = eps + M;  a = E D^(-alpha);  u = a + delta;  y = u^r - delta^r
  q = r u^(r-1);  mu[T] = 0;  mu[t] = g[t] (-alpha q a / D)[t] + (1 - s) mu[t+1]
  dE[t] = g q D^(-alpha) + s mu[t] (t >= 1), dE[0] = g q D^(-alpha) + mu[0]
  dalpha = sum g q a (-ln D);  ddelta = sum g (q - r delta^(r-1));  dr = sum g (u^r ln u - delta^r ln delta);  ds = sum_{t>=1} mu[t] (E[t] - M[t-1])

Tensors are (..., n_mels, T); the parameters (n_mels,).  The scan is sequential and the powers are torch.pow: in fp32 this is what a user
would write today, and its own error against fp64 is the yardstick of tests/test_hip_pcen.py."""
import torch

EPS = 1e-6
SHAPES = [(3, 5, 1), (3, 5, 2), (2, 7, 31), (4, 4, 32), (2, 3, 33), (2, 3, 63), (1, 6, 64), (2, 3, 65), (1, 2, 130), (1, 1, 300), (2, 3, 5, 40)]


def _col(p, like):
    return p.to(like.dtype)[:, None]


def smoother(E, s):
    """M of (..., n_mels, T), sequentially along T"""
    sc = _col(s, E)
    ms = [E[..., 0]]
    for t in range(1, E.shape[-1]):
        ms.append((1 - sc[:, 0]) * ms[-1] + sc[:, 0] * E[..., t])
    return torch.stack(ms, dim=-1)


def forward(E, alpha, delta, r, s, eps=EPS):
    """(y, M); differentiable (fp64 autograd through it is the reference of the hand-written adjoint)"""
    M = smoother(E, s)
    D = eps + M
    a = E * torch.pow(D, -_col(alpha, E))
    u = a + _col(delta, E)
    y = torch.pow(u, _col(r, E)) - torch.pow(_col(delta, E), _col(r, E))
    return y, M


def backward(g, E, alpha, delta, r, s, eps=EPS):
    """the adjoint as the issue writes it: a dict with dE (like E), dalpha, ddelta, dr, ds ((n_mels,) each), the forward's y, and the
    scales ``*_scale``: for y the value u; for dE[t] the sum of |direct term| and of |every term of s mu[t]|; for each parameter gradient the
    sum of |summand|"""
    al, de, rr, ss = (_col(p, E) for p in (alpha, delta, r, s))
    M = smoother(E, s)
    D = eps + M
    Dp = torch.pow(D, -al)
    a = E * Dp
    u = a + de
    ur = torch.pow(u, rr)
    dpr = torch.pow(de, rr)
    q = rr * torch.pow(u, rr - 1)
    h = g * (-al * q * a / D)
    T = E.shape[-1]
    mu = [None] * T
    mu_abs = [None] * T
    nxt = torch.zeros_like(E[..., 0])
    nxt_abs = torch.zeros_like(E[..., 0])
    for t in range(T - 1, -1, -1):
        nxt = h[..., t] + (1 - ss[:, 0]) * nxt
        nxt_abs = h[..., t].abs() + (1 - ss[:, 0]) * nxt_abs
        mu[t], mu_abs[t] = nxt, nxt_abs
    mu = torch.stack(mu, dim=-1)
    mu_abs = torch.stack(mu_abs, dim=-1)
    first = torch.zeros(T, dtype=E.dtype)
    first[0] = 1
    w = first + (1 - first) * ss                       # (n_mels, T): 1 at t = 0, s after
    direct = g * q * Dp
    Mprev = torch.cat([torch.zeros_like(M[..., :1]), M[..., :-1]], dim=-1)
    terms = {"dalpha": g * q * a * (-torch.log(D)),
             "ddelta": g * (q - rr * torch.pow(de, rr - 1)),
             "dr": g * (ur * torch.log(u) - dpr * torch.log(de)),
             "ds": (1 - first) * mu * (E - Mprev)}
    lead = tuple(range(E.dim() - 2)) + (E.dim() - 1,)
    out = {"y": ur - dpr, "M": M, "y_scale": u, "dE": direct + w * mu, "dE_scale": direct.abs() + w * mu_abs}
    for k, v in terms.items():
        out[k] = v.sum(dim=lead)
        out[k + "_scale"] = v.abs().sum(dim=lead)
    return out


def worst(got, ref64, scale64):
    """max |got - ref| / scale; an element whose scale is 0 must be exact"""
    err = (got.double() - ref64).abs()
    pos = scale64 > 0
    assert bool((err[~pos] == 0).all()), "an element with zero scale is not exact"
    return float((err[pos] / scale64[pos]).max()) if bool(pos.any()) else 0.0


def params(n_mels, seed, dtype=torch.float32):
    """alpha, delta, r, s per band inside PCEN.project_()'s ranges; with three bands or more band 0 sits on the closed ends
    (alpha = 0, r = 1, s = 1: the smoother is E itself and its coefficient 1 - s is 0) and band 1 on alpha = 1"""
    gen = torch.Generator().manual_seed(1000 + seed)
    u = lambda: torch.rand(n_mels, generator=gen, dtype=torch.float64)      # noqa: E731
    alpha = 0.2 + 0.8 * u()
    delta = 10.0 ** (-1.3 + 2.0 * u())                   # 0.05 ... 5
    r = 0.2 + 0.8 * u()
    s = 10.0 ** (-2.7 + 2.7 * u())                       # 0.002 ... 1
    if n_mels >= 3:
        alpha[0], r[0], s[0], delta[0] = 0.0, 1.0, 1.0, 1e-3
        alpha[1] = 1.0
    return tuple(p.to(torch.float32).to(dtype) for p in (alpha, delta, r, s))


def inputs(shape, seed):
    """(E, g) fp32 of ``shape`` = (..., n_mels, T): E = rand^4 * 10^U(-6, 2) per row, row 0 all zero, the last row zero from frame T // 3 on"""
    gen = torch.Generator().manual_seed(seed)
    T = shape[-1]
    rows = 1
    for v in shape[:-1]:
        rows *= v
    E = torch.rand(rows, T, generator=gen, dtype=torch.float64) ** 4 * 10.0 ** (-6 + 8 * torch.rand(rows, 1, generator=gen, dtype=torch.float64))
    E[0] = 0.0
    E[rows - 1, T // 3:] = 0.0
    g = torch.randn(rows, T, generator=gen, dtype=torch.float64)
    return E.to(torch.float32).reshape(shape), g.to(torch.float32).reshape(shape)
