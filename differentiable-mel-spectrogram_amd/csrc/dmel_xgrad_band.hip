// dmel_xgrad_band.hip -- the band-split layer's gradient w.r.t. the waveform (BandSplitMelSpectrogram(waveform_grad=True),
// dmel_backward_x_band / dmel_backward_x_band_dev).  The layer's K channels write ONE (B, 1, M, T) image, channel c its rows
// [e_c, e_c+1), so its cotangent is one image too: channel c's mel gradient is that image's rows [e_c, e_c+1) and +0.0 everywhere else.
// dmel_xgrad_wave_band_kernel<N> is the multi-window layer's wave-FFT kernel (dmel_xgrad_wave_body.inc: channel slot, lambd, window,
// segments, fp64 sums) that stages only those rows: the arithmetic of a bin, fmaf(c1, gm[b0 + 1], c0 * gm[b0]), is the scalar kernel's
// on the masked cotangent, bit for bit.  For the LDS path (n_fft 4096 ... 16384, shapes the wave path refuses)
// dmel_xgrad_band_stage_kernel writes that masked (B, M, T) cotangent out and the scalar frames kernel runs on it.  The combine pass is
// dmel_xgrad_combine_multi_kernel (dmel_xgrad.hip).  A translation unit of its own: the kernels of dmel_xgrad.hip and dmel_xgrad_len.hip
// keep their code.
#include "dmel_xgrad_multi.h"

namespace dmel {

#define XSTAMP(i) do {} while (0)

#define DMEL_XG_MULTI 1
#define DMEL_XG_BAND 1
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_BAND
#undef DMEL_XG_MULTI

// one element per thread and step (element-wide loads: any element-aligned grad_out), rows outside the channel's range by a select
// around the load: what lies there in `out` belongs to other channels
__global__ void __launch_bounds__(256) dmel_xgrad_band_stage_kernel(XgradBandStageParams p)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += step) {
        const int m = (int)((i / p.T) % p.M);
        const bool in = m >= p.e_lo && m < p.e_hi;
        float g = 0.f, y = 0.f;
        if (in) {
            g = p.grad_out[i];
            if (p.out) y = p.out[i];
        }
        p.stage_grad[i] = g;
        if (p.out) p.stage_out[i] = y;
    }
}

static constexpr auto kBandWave = [](auto nn) { return dmel_xgrad_wave_band_kernel<decltype(nn)::value>; };

hipError_t xgrad_band_prepare_attributes() { return xgrad_set_wave_attributes(kBandWave); }

// the band-split layer's wave-FFT launch (xgrad_launch_wave_multi, dmel_xgrad_multi.h: the band edges are checked there)
hipError_t launch_xgrad_wave_band(const XgradBandParams& p, hipStream_t s) { return xgrad_launch_wave_multi(p, kBandWave, s); }

hipError_t launch_xgrad_band_stage(const XgradBandStageParams& p, hipStream_t s)
{
    if (p.n < 1 || p.M < 1 || p.T < 1 || p.e_lo < 0 || p.e_lo >= p.e_hi || p.e_hi > p.M || !p.grad_out || !p.stage_grad || (p.out && !p.stage_out))
        return hipErrorInvalidValue;
    const long long blocks = (p.n + 255) / 256;
    hipLaunchKernelGGL(dmel_xgrad_band_stage_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
