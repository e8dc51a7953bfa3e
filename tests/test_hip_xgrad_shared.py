"""Where the scalar and the K-window waveform gradients meet, on the MI355X: a K-window layer with ONE channel (MultiWindowMelSpectrogram,
BandSplitMelSpectrogram with edges [0, M]) gives zeros + x.grad of MelSpectrogramLayer, bit for bit and NaN for NaN.  Both sides take their
segment sum, frame-row sum, tile-sum mean and tree mean from the same helpers of csrc/dmel_xgrad_plan.h, through kernels that walk a chunk
differently: the scalar combine by rows of four where every row is 16-byte aligned (n_points 4104, hop 8) and element by element where not
(n_points 4101, hop 7: two chunks of 4096, the second of 5 samples), the K-window combine always 16 elements per thread.  lambd 10 is
n_fft 64 (the wave-FFT kernel and the combine pass), lambd 700 n_fft 8192 (the LDS frames kernel and the gather).  Lengths: the whole row,
one sample past the chunk boundary, and a clip shorter than a hop (one frame)."""
import functools

import pytest
import torch

from dmel_amd import BandSplitMelSpectrogram, MelSpectrogramLayer, MultiWindowMelSpectrogram, capi, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, M, SR = 3, 8, 16000
# (n_points, hop, lambd, n_fft): n_fft 32 ... 2048 whose tables fit the LDS take the wave path, 4096 ... 16384 the LDS path
CASES = [(4101, 7, 10.0, 64), (4104, 8, 10.0, 64), (4101, 64, 700.0, 8192), (4104, 64, 700.0, 8192)]
CASE_IDS = ["wave_4101_hop7", "wave_4104_hop8", "lds_4101_hop64", "lds_4104_hop64"]


def _lengths(L, on):
    return torch.tensor([L, 4097, 1], dtype=torch.int32, device=DEV) if on else None


def _inputs(L, hop):
    x = torch.from_numpy(synth.waveforms(B, L, seed=31)).to(DEV)
    g = torch.from_numpy(synth.cotangent((B, 1, M, L // hop + 1), seed=32)).to(DEV)
    return x, g


def _xgrad(layer, x, g, lengths):
    xr = x.detach().clone().requires_grad_(True)
    y = layer(xr) if lengths is None else layer(xr, lengths)
    y.backward(g)
    torch.cuda.synchronize()
    return xr.grad.detach()


@functools.lru_cache(maxsize=None)
def _reference(L, hop, lam, n_fft, with_lengths):
    """zeros + x.grad of the scalar layer: computed once per case, shared by the two K-window layers, never written to"""
    x, g = _inputs(L, hop)
    lay = MelSpectrogramLayer(torch.tensor(lam), n_mels=M, n_points=L, sample_rate=SR, hop_length=hop, device=DEV, optimized=True, log=True,
                              lengths_waveform_grad=with_lengths).to(DEV)
    gx = _xgrad(lay, x, g, _lengths(L, with_lengths))
    assert lay.plan_info()["n_fft"] == n_fft
    return torch.zeros_like(x) + gx


@pytest.mark.parametrize("with_lengths", [False, True], ids=["fixed", "lengths"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", ["multi", "band"])
def test_one_channel_is_the_scalar_layer(kind, case, with_lengths):
    L, hop, lam, n_fft = case
    assert capi.n_fft(lam) == n_fft
    kw = dict(hop_length=hop, log=True)
    kw.update(dict(per_clip_lengths=True, lengths_waveform_grad=True) if with_lengths else dict(waveform_grad=True))
    if kind == "multi":
        lay = MultiWindowMelSpectrogram([lam], M, L, SR, **kw).to(DEV)
    else:
        lay = BandSplitMelSpectrogram([lam], M, L, SR, band_edges=[0, M], **kw).to(DEV)
    x, g = _inputs(L, hop)
    gx = _xgrad(lay, x, g, _lengths(L, with_lengths))
    # the launch lambd asks for is among those issued (a cold sync-free step also issues its neighbours, which return at once), and every
    # one of them lies on the side of 2048 | 4096 that CASES names: that path's kernels wrote x.grad
    launches = lay._plan_for(torch.device(DEV)).last_multi_launch()
    assert (n_fft, 1) in launches and all((n <= 2048) == (n_fft <= 2048) for n, _ in launches), launches
    ref = _reference(L, hop, lam, n_fft, with_lengths)
    assert torch.equal(torch.isnan(gx), torch.isnan(ref))
    assert not torch.isnan(ref).any()                                                     # (every length is valid)
    assert torch.equal(gx, ref), float((gx - ref).abs().max())
    if with_lengths:
        assert int(gx[1, 4097:].abs().max()) == 0 and int(gx[2, 1:].abs().max()) == 0 and bool(gx[0].abs().max() > 0)
