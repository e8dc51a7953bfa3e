// dmel_xgrad.hip -- gradient w.r.t. the waveform (optional output of the layer's backward; the reference never asks for
// it, torch autograd would return it for x.requires_grad).  Adjoint of models.py:38 (DC removal),
// time_frequency.py:43-53 (zero padding, framing, window, rfft, |.|^2) and models.py:53 (mel contraction):
//
//   gP[k][t]  = sum_m fb[k][m] gm[m][t]                 gm = grad_out, or grad_out * exp(-out) for the log output
//   dv_t[n]   = sum_{k=0}^{N-1} H_k e^{+2 pi i k n / N}   H_k = c_k gP[k] X_t[k]  (c = 2 at k = 0 and N/2, else 1), Hermitian
//   dx~[i]    = sum over the frames t that cover i of dv_t[i - t hop + N/2] w[i - t hop + N/2]
//   dx        = dx~ - mean(dx~)
//
// Kernel 1 (one workgroup per pair of frames, any power-of-two n_fft up to 16384): both frames go through ONE complex
// FFT held in LDS (in-place decimation in frequency, radix-2 stages fused in pairs, spectrum in bit-reversed order), the two spectra are
// separated, scaled by gP and written back -- conjugated, Hermitian-extended, packed as conj(H_a) + i conj(H_b)... -- at
// the same bit-reversed addresses, which is exactly the input order of an in-place decimation-in-time FFT; its output
// is conj(dv_a + i dv_b) in natural order.  No permutation pass, no second buffer.  The windowed frame gradients go to a
// (B, T, N) workspace.
// Kernel 2 (one workgroup per 4096 samples): overlap-add as a gather in increasing frame order (deterministic, no atomics) minus
// the mean of the clip's gradient, which comes from fp64 per-frame sums left by kernel 1 (a third kernel used to subtract it).
// A correctness-first path: about 10x the time of the fused forward at config 2.
// Kernels 1 and 2 and the combine pass are written once, for these clips and for clips of per-clip lengths (dmel_xgrad_len.hip):
// dmel_xgrad_body.h.  This file holds their fixed-length entry points, the wave-FFT kernels and the multi-window layer's combine pass.
#include "dmel_xgrad_body.h"
#include "dmel_xgrad_multi.h"

namespace dmel {

// the entry points of the fixed-length bodies (dmel_xgrad_body.h)
template <bool TWLDS> __global__ void __launch_bounds__(kXgThreads) dmel_xgrad_frames_kernel(XgradParams p) { xgrad_frames_body<TWLDS>(p); }
__global__ void __launch_bounds__(256) dmel_xgrad_gather_kernel(XgradParams p) { xgrad_gather_body(p); }
__global__ void __launch_bounds__(256) dmel_xgrad_combine_kernel(XgradParams p) { xgrad_combine_body(p); }

// ---- the same gradient on the forward's wave FFT (n_fft 32 ... 2048) ---------------------------------------------------------
// One wave (or G = N / R lanes of it) per PAIR of neighbouring frames, as in the forward's inference mode: the pair rides in one
// complex FFT held in registers (wave_fft, dmel_wavefft.h), the spectrum lands in the pair's LDS slot in natural order, the
// lanes separate the two spectra bin by bin, contract the mel gradient with the filterbank rows (gm of the tile's frames sits
// in LDS; an HTK row has two non-zero columns), write conj(H_a + i H_b) -- Hermitian-extended -- back over the spectrum, and a
// second wave_fft of those N points is conj(dv_a + i dv_b).  Windowed, the two frame gradients stay in the slot: after one
// workgroup barrier the tile's frames are overlap-added as a gather in increasing frame order (deterministic) and only the
// tile's SEGMENT of (FPT - 1) hop + N samples goes to memory -- a quarter of the (B, T, N) frame workspace at BASELINE config 2 --
// together with its fp64 sum over the samples inside the clip.  dmel_xgrad_combine_kernel adds the (at most few) segments that
// cover a sample, in increasing tile order, and subtracts the mean.
#ifdef DMEL_STAMPS
// diagnostic build only (tools/xstamps.py): s_memtime of every wave at the phase boundaries of the wave-FFT kernel
constexpr int kXStampSlots = 16;
__device__ unsigned long long g_xstamps[4096 * 8 * kXStampSlots];
__device__ __forceinline__ void xstamp(int wgid, int wave, int lane, int idx)
{
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (lane == 0 && wgid < 4096) g_xstamps[((size_t)wgid * 8 + wave) * kXStampSlots + idx] = t;
}
#define XSTAMP(i) xstamp(blockIdx.x, wave, lane, i)
#else
#define XSTAMP(i) do {} while (0)
#endif

// (XgPlan<N>, the kernel's geometry: dmel_xgrad_plan.h)
// the kernel itself: dmel_xgrad_wave_kernel<N> (scalar layer) and dmel_xgrad_wave_multi_kernel<N> (multi-window layer, XgradMultiParams)
#define DMEL_XG_MULTI 0
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_MULTI
#define DMEL_XG_MULTI 1
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_MULTI

// the multi-window layer's combine pass: grad_x = 0 + term_0 + term_1 + ... in ascending channel order (dmel_xgrad_multi.h)
__global__ void __launch_bounds__(256) dmel_xgrad_combine_multi_kernel(XgradCombineMultiParams p) { xgrad_combine_multi_body(p); }

// the wave-FFT path takes this shape (otherwise the LDS radix-2 kernels above run)
bool xgrad_wave_shape(int n_fft, int n_mels, int win_n, int* frames_per_tile)
{
    bool ok = false;
    xgrad_with_plan(n_fft, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        ok = xgrad_wave_lds<N>(n_mels, win_n) <= (size_t)XgPlan<N>::LDS_MAX;
        if (frames_per_tile) *frames_per_tile = XgPlan<N>::FPT;
    });
    return ok;
}

template <> struct XgKernels<XgradParams> {
    template <bool TWLDS> static constexpr auto frames = dmel_xgrad_frames_kernel<TWLDS>;
    template <int N> static constexpr auto wave = dmel_xgrad_wave_kernel<N>;
    static constexpr auto gather = dmel_xgrad_gather_kernel, combine = dmel_xgrad_combine_kernel;
};

static constexpr auto kMultiWave = [](auto nn) { return dmel_xgrad_wave_multi_kernel<decltype(nn)::value>; };

hipError_t xgrad_prepare_attributes()
{
    const hipError_t e = xgrad_set_attributes<XgradParams>();
    return e != hipSuccess ? e : xgrad_set_wave_attributes(kMultiWave);
}

hipError_t launch_xgrad(const XgradParams& p, hipStream_t s) { return xgrad_launch(p, s); }
hipError_t launch_xgrad_frames(const XgradParams& p, hipStream_t s) { return xgrad_launch_frames(p, s); }
hipError_t launch_xgrad_gather(const XgradParams& p, hipStream_t s) { return xgrad_launch_second(dmel_xgrad_gather_kernel, p, s); }

// the multi-window layer's wave-FFT launch (xgrad_launch_wave_multi, dmel_xgrad_multi.h)
hipError_t launch_xgrad_wave_multi(const XgradMultiParams& p, hipStream_t s) { return xgrad_launch_wave_multi(p, kMultiWave, s); }

hipError_t launch_xgrad_combine_multi(const XgradCombineMultiParams& p, int batch, hipStream_t s)
{
    const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)batch);
    hipLaunchKernelGGL(dmel_xgrad_combine_multi_kernel, g2, dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel

namespace dmel { int xgrad_chunks(int L) { return (L + kXgChunk - 1) / kXgChunk; } }      // (kept for the workspace layout of dmel_api.cpp)

#ifdef DMEL_STAMPS
extern "C" int dmel_debug_read_xstamps(unsigned long long* host, int count)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(dmel::g_xstamps), sizeof(unsigned long long) * (size_t)count);
}
#endif
