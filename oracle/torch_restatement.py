"""Batched torch-CPU restatement of the reference's DMEL path.  TEST INFRASTRUCTURE ONLY.

Same library calls as the reference (torch.stft with the Gaussian window, |.|^2, matmul with the HTK
filterbank, log, torch autograd for d/dlambd) but for the whole batch at once instead of the
per-sample Python loop of models.py:37-54.  It exists for two reasons:
  * an independent check of oracle/dmel_oracle.c (different FFT, reverse-mode autograd instead of
    the closed-form tangent);
  * bench.py's cpu_baseline: it is the fastest CPU form of the reference's algorithm measured in
    BASELINE.md section 2 (the reference's own loop spends 70 % of its time in a CopySlices artefact).
Only tests/ and bench.py's cpu_baseline leg may import this module.

tangent_fp64 / tangent_fp32 evaluate the forward-mode tangent d out / d lambd element by element by a third route (the window's
derivative from torch.autograd.functional.jacobian, then a second stft with it), together with the cancellation-free magnitude of
every tangent element: what tests/tangent_cases.py measures the oracle's and the kernels' tangents against.

fbgrad_fp64 / fbgrad_fp32 evaluate the filterbank gradient grad_fb[f, m] = sum_{b,t} spec[b, f, t] gm[b, m, t] together with its
cancellation-free magnitude sum spec |gm| (spec >= 0: the sum cancels only through the sign of the cotangent): what tests/fbgrad_cases.py
measures the oracle's and the kernels' filterbank gradients against.

Reference lines followed: time_frequency.py:21-30 (window), :39,:60-65 (n_fft), :48 (stft),
:53 (power); models.py:38 (DC removal, abs), :42-53 (filterbank, contraction), :73 (log).
"""
from __future__ import annotations

import math

import torch


def n_fft_of(lambd: torch.Tensor) -> int:
    x = int((torch.abs(lambd).detach().float() * 6).cpu().numpy())   # time_frequency.py:39,61
    return 1 << (x - 1).bit_length()


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """torchaudio 0.13.1 functional.melscale_fbanks (htk, norm=None); PARITY-UNPINNED (see dmel_oracle.c)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + (f_min / 700.0))
    m_max = 2595.0 * math.log10(1.0 + (f_max / 700.0))
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


def forward(x: torch.Tensor, lambd: torch.Tensor, hop: int, n_mels: int, sample_rate: int, f_min=0.0, f_max=None,
            normalize_window=False, log=False, eps=1e-10, fb=None) -> torch.Tensor:
    """x (B, L) fp32 CPU, lambd 0-dim (may require grad) -> (B, 1, n_mels, L//hop+1) fp32."""
    f_max = sample_rate // 2 if f_max is None else f_max
    n = n_fft_of(lambd)
    a = torch.abs(lambd)
    m = torch.arange(0, n).float()
    window = torch.exp(-0.5 * torch.pow((m - n / 2) / (a + 1e-15), 2))
    if normalize_window:
        window = window / torch.sqrt(torch.sum(torch.pow(window, 2)))
    xc = x - x.mean(dim=1, keepdim=True)
    s = torch.stft(xc, n_fft=n, hop_length=hop, win_length=n, window=window, return_complex=True, pad_mode="constant")
    p = s.real * s.real + s.imag * s.imag                     # (B, F, T)
    if fb is None:
        fb = melscale_fbanks(n // 2 + 1, f_min, f_max, n_mels, sample_rate)
    mel = torch.matmul(p.transpose(-1, -2), fb).transpose(-1, -2).unsqueeze(1)
    return torch.log(mel + eps) if log else mel


def step(x: torch.Tensor, g: torch.Tensor, lambd_value: float, hop: int, n_mels: int, sample_rate: int, log=True, fb=None):
    """One forward + backward to lambd.grad; returns (out, dlambd)."""
    lam = torch.tensor(float(lambd_value), requires_grad=True)
    out = forward(x, lam, hop, n_mels, sample_rate, log=log, fb=fb)
    (dl,) = torch.autograd.grad((out * g).sum(), lam)
    return out.detach(), float(dl)


def _window_of(lam: torch.Tensor, n: int, normalize_window: bool) -> torch.Tensor:
    """the Gaussian window of n points as a function of lambd, in lambd's dtype"""
    m = torch.arange(0, n, dtype=lam.dtype)
    window = torch.exp(-0.5 * torch.pow((m - n / 2) / (torch.abs(lam) + 1e-15), 2))
    if normalize_window:
        window = window / torch.sqrt(torch.sum(torch.pow(window, 2)))
    return window


def _tangent(dtype, x, lambd, hop, n_mels, sample_rate, f_min, f_max, normalize_window, log, eps, optimized, mean, fb, spectrogram):
    import numpy as np
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    B, L = x32.shape
    lam32 = np.float32(lambd)
    lam = torch.tensor(float(lam32), dtype=dtype)
    n_win = n_fft_of(torch.tensor(float(lam32))) if optimized else L
    n = n_win if optimized else 2 * L
    w = _window_of(lam, n_win, normalize_window)
    dw = torch.autograd.functional.jacobian(lambda l: _window_of(l, n_win, normalize_window), lam, vectorize=True,
                                            strategy="forward-mode").reshape(n_win)
    if mean is None:
        mean = np.float32(x32.astype(np.float64).mean(axis=1))              # the correctly rounded fp32 mean (models.py:38)
    mean = np.asarray(mean, dtype=np.float32).reshape(B, 1)
    xc = torch.tensor(x32).to(dtype) - torch.tensor(mean).to(dtype)
    kw = dict(n_fft=n, hop_length=hop, win_length=n_win, return_complex=True, pad_mode="constant")
    S = torch.stft(xc, window=w, **kw)                                        # (B, F, T)
    D = torch.stft(xc, window=dw, **kw)
    p = S.real * S.real + S.imag * S.imag
    dp = 2.0 * (S.real * D.real + S.imag * D.imag)
    sc = 2.0 * torch.abs(S) * torch.abs(D)
    if not spectrogram:
        if fb is None:
            from oracle import dmel_oracle as O
            fb = O.mel_fbanks(n // 2 + 1, f_min, float(sample_rate // 2) if f_max is None else f_max, n_mels, sample_rate)
        fbt = torch.tensor(np.asarray(fb, dtype=np.float32)).to(dtype)      # (F, M)
        p = torch.einsum("fm,bft->bmt", fbt, p)
        dp = torch.einsum("fm,bft->bmt", fbt, dp)
        sc = torch.einsum("fm,bft->bmt", fbt.abs(), sc)
    if log:
        dp, sc = dp / (p + eps), sc / torch.abs(p + eps)
        p = torch.log(p + eps)
    return tuple(v.unsqueeze(1).to(torch.float64).numpy() for v in (p, dp, sc))


def tangent_fp64(x, lambd, hop, n_mels, sample_rate, f_min=0.0, f_max=None, normalize_window=False, log=False, eps=1e-10,
                 optimized=True, mean=None, fb=None, spectrogram=False):
    """(out, tangent, scale), each (B, 1, n_mels, L//hop+1) fp64 -- with ``spectrogram`` (B, 1, n_fft/2+1, L//hop+1), no bank: the
    SpectrogramLayer.  Everything in torch.float64 from the fp32 clip ``x`` (B, L) and ``lambd`` rounded to fp32:
      window(lambd) of n_fft points (``optimized``) or of L points inside n_fft = 2L, and dw = d window / d lambd by autograd's jacobian
      of that very function (so the normalised window and the sign of a negative lambd come with it);
      S = stft(x - mean, window), D = stft(x - mean, dw);  p = |S|^2,  dp = 2 Re(conj(S) D),  sc = 2 |S| |D|;
      the three contracted with the bank (``fb`` (F, M), else the HTK bank; sc with |fb|), and for ``log`` tangent and scale over mel + eps.
    ``scale`` bounds |tangent| element by element and is free of cancellation: the magnitude an fp32 evaluation of that element can be
    asked to be accurate against.  ``mean``: fp32 clip means given instead of computed, as dmel_oracle.forward(mean=...) takes them."""
    return _tangent(torch.float64, x, lambd, hop, n_mels, sample_rate, f_min, f_max, normalize_window, log, eps, optimized, mean, fb,
                    spectrogram)


def tangent_fp32(x, lambd, hop, n_mels, sample_rate, f_min=0.0, f_max=None, normalize_window=False, log=False, eps=1e-10,
                 optimized=True, mean=None, fb=None, spectrogram=False):
    """tangent_fp64's construction in the reference's own arithmetic: fp32 window, fp32 stft, fp32 contraction (returned as fp64 arrays)"""
    return _tangent(torch.float32, x, lambd, hop, n_mels, sample_rate, f_min, f_max, normalize_window, log, eps, optimized, mean, fb,
                    spectrogram)


def fbgrad_operands(dtype, x, lambd, hop, n_mels, sample_rate, grad_out, out=None, f_min=0.0, f_max=None, normalize_window=False,
                    optimized=True, lengths=None, eps=None, mean=None, fb=None):
    """the two operands of the filterbank gradient in ``dtype``, as fbgrad_fp64 describes them: spec (B, F, T), zero in the pad frames of a
    clip shorter than the batch, and gm (B, M, T), zero there too"""
    import numpy as np
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    B, L = x32.shape
    T = L // hop + 1
    lam32 = np.float32(lambd)
    lam = torch.tensor(float(lam32), dtype=dtype)
    n_win = n_fft_of(torch.tensor(float(lam32))) if optimized else L
    n = n_win if optimized else 2 * L
    F = n // 2 + 1
    w = _window_of(lam, n_win, normalize_window)
    lens = [L] * B if lengths is None else [int(v) for v in np.asarray(lengths).reshape(B)]
    if mean is not None:
        mean = np.asarray(mean, dtype=np.float32).reshape(B)
    p = torch.zeros((B, F, T), dtype=dtype)                                   # frames at or past lengths[b] // hop + 1 stay out of both sums
    for b, Lb in enumerate(lens):
        assert 1 <= Lb <= L, (b, Lb)
        xb = x32[b, :Lb]
        mb = np.float32(xb.astype(np.float64).mean()) if mean is None else mean[b]      # the correctly rounded fp32 mean (models.py:38)
        xc = torch.tensor(xb).to(dtype) - torch.tensor(float(mb), dtype=dtype)
        S = torch.stft(xc[None, :], n_fft=n, hop_length=hop, win_length=n_win, window=w, return_complex=True, pad_mode="constant")[0]
        assert S.shape == (F, Lb // hop + 1), (S.shape, F, Lb, hop)
        p[b, :, :Lb // hop + 1] = S.real * S.real + S.imag * S.imag
    live = torch.tensor([[t < Lb // hop + 1 for t in range(T)] for Lb in lens])[:, None, :]          # (B, 1, T): pad frames are never read
    zero = torch.zeros((), dtype=dtype)
    g = torch.where(live, torch.tensor(np.ascontiguousarray(np.asarray(grad_out, dtype=np.float32).reshape(B, n_mels, T))).to(dtype), zero)
    if out is not None:
        g = g * torch.exp(-torch.where(live, torch.tensor(np.ascontiguousarray(np.asarray(out, dtype=np.float32).reshape(B, n_mels, T))).to(dtype), zero))
    elif eps is not None:
        if fb is None:
            from oracle import dmel_oracle as O
            fb = O.mel_fbanks(F, f_min, float(sample_rate // 2) if f_max is None else f_max, n_mels, sample_rate)
        fbt = torch.tensor(np.asarray(fb, dtype=np.float32)).to(dtype)          # (F, M)
        g = g / (torch.einsum("fm,bft->bmt", fbt, p) + eps)                      # d log(mel + eps) = d mel / (mel + eps) = d mel exp(-out)
    return p, g


def _fbgrad(dtype, *args):
    p, g = fbgrad_operands(dtype, *args)
    gfb = torch.einsum("bft,bmt->fm", p, g)
    sc = torch.einsum("bft,bmt->fm", p, g.abs())
    return gfb.to(torch.float64).numpy(), sc.to(torch.float64).numpy()


def fbgrad_fp64(x, lambd, hop, n_mels, sample_rate, grad_out, out=None, f_min=0.0, f_max=None, normalize_window=False, optimized=True,
                lengths=None, eps=None, mean=None, fb=None):
    """(grad_fb, scale), each (n_fft/2+1, n_mels) fp64: the adjoint of models.py:53 and its cancellation-free magnitude.  Everything in
    torch.float64 from the fp32 clip ``x`` (B, L), ``lambd`` rounded to fp32 and the fp32 cotangent ``grad_out`` (B, 1, n_mels, L//hop+1):
      spec = |stft(x - mean, window(lambd))|^2 as tangent_fp64 forms it (``optimized``: n_fft points; else the whole-clip window in n_fft = 2L);
      gm = grad_out for the linear output (``out`` None and ``eps`` None);  grad_out exp(-out) with the saved LOG output ``out`` -- what the
      kernels are given;  with ``out`` None and ``eps`` set, the log output is computed here: grad_out / (mel + eps), mel through ``fb`` (F, M)
      or the HTK bank;
      grad_fb = sum_{b,t} spec gm,  scale = sum_{b,t} spec |gm|.
    ``lengths``: clip b is x[b, :lengths[b]] with its own mean, and frames at or past lengths[b] // hop + 1 are left out of both sums.
    |grad_fb| <= scale element by element; scale == 0 exactly where no frame of any clip has power in the bin or the cotangent is zero."""
    return _fbgrad(torch.float64, x, lambd, hop, n_mels, sample_rate, grad_out, out, f_min, f_max, normalize_window, optimized, lengths,
                   eps, mean, fb)


def fbgrad_fp32(x, lambd, hop, n_mels, sample_rate, grad_out, out=None, f_min=0.0, f_max=None, normalize_window=False, optimized=True,
                lengths=None, eps=None, mean=None, fb=None):
    """fbgrad_fp64's construction in the reference's own arithmetic: fp32 window, stft, exp and contraction (returned as fp64 arrays)"""
    return _fbgrad(torch.float32, x, lambd, hop, n_mels, sample_rate, grad_out, out, f_min, f_max, normalize_window, optimized, lengths,
                   eps, mean, fb)
