// dmel_xgrad_klen.hip -- the K-window layers' gradient w.r.t. the waveform over clips of per-clip lengths
// (MultiWindowMelSpectrogram / BandSplitMelSpectrogram(lengths_waveform_grad=True), dmel_backward_x_multi_lengths, dmel_backward_x_band_lengths
// and their _dev forms): the product of dmel_xgrad_len.hip (clip bounds from Lc = lengths[b], Tc = Lc / hop + 1) with the channel slot of
// dmel_xgrad_wave_multi_kernel and the row range of dmel_xgrad_wave_band_kernel.  dmel_xgrad_wave_multi_len_kernel<N> and
// dmel_xgrad_wave_band_len_kernel<N> are two more builds of dmel_xgrad_wave_body.inc; dmel_xgrad_combine_multi_len_kernel is the length-aware
// build of the K-window combine body (dmel_xgrad_multi.h): every term formed as dmel_xgrad_combine_len_kernel (wave path) or
// dmel_xgrad_gather_len_kernel (LDS path) forms it, s - mean inside the clip, +0.0 past it.  The LDS path runs dmel_xgrad_len.hip's frames
// kernel per channel on the staged rows (launch_xgrad_frames_len).
#include "dmel_xgrad_multi.h"

namespace dmel {

#define XSTAMP(i) do {} while (0)

#define DMEL_XG_MULTI 1
#define DMEL_XG_LEN 1
#include "dmel_xgrad_wave_body.inc"
#define DMEL_XG_BAND 1
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_BAND
#undef DMEL_XG_LEN
#undef DMEL_XG_MULTI

__global__ void __launch_bounds__(256) dmel_xgrad_combine_multi_len_kernel(XgradCombineMultiLenParams p) { xgrad_combine_multi_body(p); }

static constexpr auto kMultiLenWave = [](auto nn) { return dmel_xgrad_wave_multi_len_kernel<decltype(nn)::value>; };
static constexpr auto kBandLenWave = [](auto nn) { return dmel_xgrad_wave_band_len_kernel<decltype(nn)::value>; };

hipError_t xgrad_klen_prepare_attributes()
{
    const hipError_t e = xgrad_set_wave_attributes(kMultiLenWave);
    return e != hipSuccess ? e : xgrad_set_wave_attributes(kBandLenWave);
}

// the wave-FFT launches (xgrad_launch_wave_multi, dmel_xgrad_multi.h: lengths, fpt and the band edges are checked there)
hipError_t launch_xgrad_wave_multi_len(const XgradMultiLenParams& p, hipStream_t s) { return xgrad_launch_wave_multi(p, kMultiLenWave, s); }
hipError_t launch_xgrad_wave_band_len(const XgradBandLenParams& p, hipStream_t s) { return xgrad_launch_wave_multi(p, kBandLenWave, s); }

hipError_t launch_xgrad_combine_multi_len(const XgradCombineMultiLenParams& p, int batch, hipStream_t s)
{
    if (!p.lengths || batch < 1 || p.L < 1 || p.hop < 1 || p.T != p.L / p.hop + 1) return hipErrorInvalidValue;
    for (int c = 0; c < p.channels; ++c)
        for (int j = 0; j < p.ncand[c]; ++j)
            if (p.tiles[c][j] > 0 && p.fpt[c][j] < 1) return hipErrorInvalidValue;
    const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)batch);
    hipLaunchKernelGGL(dmel_xgrad_combine_multi_len_kernel, g2, dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
