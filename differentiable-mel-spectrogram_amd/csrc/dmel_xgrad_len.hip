// dmel_xgrad_len.hip -- the gradient w.r.t. the waveform over clips of per-clip lengths (MelSpectrogramLayer(lengths_waveform_grad=True),
// dmel_backward_x_lengths / dmel_backward_x_dev_lengths): the kernels of dmel_xgrad.hip with every sample-space bound of a clip (buffer
// resource, interior test, load clamps, the zeroing at windowing time, the clip sum and its quotient, the in-clip test of the gradient's
// own sum) taken from Lc = lengths[b] and every frame-space bound from Tc = Lc / hop + 1.  L stays the row stride of x / grad_x and T
// the row stride of grad_out / out.  A pad frame (t >= Tc) has a zero mel gradient, so one that shares its complex FFT with a frame of the
// clip contributes H = 0; a tile (wave path) or a pair (LDS path) of pad frames only does nothing at all, and the second pass reads
// neither its segment nor its sum: the workspace is plan-owned and holds what an earlier call left there.  grad_x[b, Lc:] = 0; a length
// outside 1 ... L makes the row NaN.  With Lc = L everywhere the arithmetic, operation by operation, is that of dmel_xgrad.hip.
#include "dmel_xgrad_body.h"

namespace dmel {

#define XSTAMP(i) do {} while (0)

// ---- wave path (n_fft 32 ... 2048): dmel_xgrad_wave_len_kernel<N> ---------------------------------------------------------------------
#define DMEL_XG_MULTI 0
#define DMEL_XG_LEN 1
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_LEN
#undef DMEL_XG_MULTI

// ---- LDS path (n_fft 4096 ... 16384, and shapes the wave path refuses), the combine pass: the entry points of the bodies' length-aware builds
template <bool TWLDS> __global__ void __launch_bounds__(kXgThreads) dmel_xgrad_frames_len_kernel(XgradLenParams p) { xgrad_frames_body<TWLDS>(p); }
__global__ void __launch_bounds__(256) dmel_xgrad_gather_len_kernel(XgradLenParams p) { xgrad_gather_body(p); }
__global__ void __launch_bounds__(256) dmel_xgrad_combine_len_kernel(XgradLenParams p) { xgrad_combine_body(p); }

template <> struct XgKernels<XgradLenParams> {
    template <bool TWLDS> static constexpr auto frames = dmel_xgrad_frames_len_kernel<TWLDS>;
    template <int N> static constexpr auto wave = dmel_xgrad_wave_len_kernel<N>;
    static constexpr auto gather = dmel_xgrad_gather_len_kernel, combine = dmel_xgrad_combine_len_kernel;
};

hipError_t xgrad_len_prepare_attributes() { return xgrad_set_attributes<XgradLenParams>(); }

hipError_t launch_xgrad_len(const XgradLenParams& p, hipStream_t s)
{
    if (!p.lengths || p.spec_mode) return hipErrorInvalidValue;
    return xgrad_launch(p, s);
}

// the frames kernel alone (no gather): the K-window layers run it per channel and gather in dmel_xgrad_combine_multi_len_kernel
hipError_t launch_xgrad_frames_len(const XgradLenParams& p, hipStream_t s)
{
    if (!p.lengths || p.spec_mode) return hipErrorInvalidValue;
    return xgrad_launch_frames(p, s);
}

}  // namespace dmel
