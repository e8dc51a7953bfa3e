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

// grid (chunks, B): the multi-window layer's gradient w.r.t. the waveform, one launch per backward.  Every thread keeps 16 samples
// (i = lo + tid + 256 r: consecutive lanes read consecutive words) and adds the channels' terms in ascending channel order, starting from
// 0.f -- the sum autograd forms over K scalar layers.  A term is what the scalar path of that channel writes: segments in increasing
// tile order minus the sequential fp64 tile-sum mean (dmel_xgrad_combine_kernel), or frame rows in increasing frame order minus the
// mean of the 256-wide fp64 tree (dmel_xgrad_gather_kernel).  One write of grad_x; no atomics.
__global__ void __launch_bounds__(256) dmel_xgrad_combine_multi_kernel(XgradCombineMultiParams p)
{
    __shared__ double red[256];
    constexpr int PER = kXgChunk / 256;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    float acc[PER];
    static_for<0, PER>([&](auto rr) { acc[decltype(rr)::value] = 0.f; });
    for (int c = 0; c < p.channels; ++c) {
        int j = 0;
        if (p.lam_dev) {                                              // the n_fft lambd[c] asks for: one of the launches issued for it?
            const int n = lam_n_fft(__builtin_fabsf(p.lam_dev[c]));
            j = -1;
            for (int q = 0; q < p.ncand[c]; ++q) if (p.n[c][q] == n) j = q;
        }
        if (j < 0) {
            static_for<0, PER>([&](auto rr) { constexpr int r = decltype(rr)::value; acc[r] = acc[r] + __builtin_nanf(""); });
            continue;
        }
        const int N = p.n[c][j], tiles = p.tiles[c][j], half = N / 2;
        if (tiles > 0) {
            const int span = p.span[c][j], ts = p.tile_step[c][j];
            const float* sg = p.frames[c] + (size_t)b * tiles * (size_t)span;
            const int u_lo = lo + half, u_hi = hi - 1 + half;
            const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
            const int qb = min(tiles - 1, u_hi / ts);
            double dacc = 0.0;
            for (int q = 0; q < tiles; ++q) dacc += p.csum[c][(size_t)b * tiles + q];
            const float mean = (float)(dacc / (double)p.L);
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < hi) {
                    const int u = i + half;
                    float s = 0.f;
                    for (int q = qa; q <= qb; ++q) {
                        const int off = u - q * ts;
                        if (off >= 0 && off < span) s += sg[(size_t)q * span + off];
                    }
                    acc[r] = acc[r] + (s - mean);
                }
            });
        } else {
            const int T = p.T, hop = p.hop;
            __syncthreads();                                          // (red of the previous channel has been read)
            double dacc = 0.0;
            for (int t = tid; t < T; t += 256) dacc += p.csum[c][(size_t)b * T + t];
            red[tid] = dacc;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
            const float mean = (float)(red[0] / (double)p.L);
            const float* fr = p.frames[c] + (size_t)b * T * N;
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < hi) {
                    int t_lo = i + half - N + 1;
                    t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
                    int t_hi = (i + half) / hop;
                    if (t_hi > T - 1) t_hi = T - 1;
                    float s = 0.f;
                    for (int t = t_lo; t <= t_hi; ++t) s += fr[(size_t)t * N + (i - t * hop + half)];
                    acc[r] = acc[r] + (s - mean);
                }
            });
        }
    }
    float* gx = p.grad_x + (size_t)b * p.L;
    static_for<0, PER>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int i = lo + tid + 256 * r;
        if (i < hi) gx[i] = acc[r];
    });
}

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

hipError_t xgrad_prepare_attributes()
{
    hipError_t e = xgrad_set_attributes<XgradParams>();
    for (int n = 32; n <= 2048 && e == hipSuccess; n *= 2)
        xgrad_with_plan(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<N>::LDS_MAX);
        });
    return e;
}

hipError_t launch_xgrad(const XgradParams& p, hipStream_t s) { return xgrad_launch(p, s); }
hipError_t launch_xgrad_frames(const XgradParams& p, hipStream_t s) { return xgrad_launch_frames(p, s); }
hipError_t launch_xgrad_gather(const XgradParams& p, hipStream_t s) { return xgrad_launch_second(dmel_xgrad_gather_kernel, p, s); }

// the multi-window layer: one wave-FFT launch for the `count` channels of ch_list at p.p.N (ch_grid = B x tiles workgroups each)
hipError_t launch_xgrad_wave_multi(const XgradMultiParams& p, hipStream_t s)
{
    const long long grid = (long long)p.count * p.ch_grid;
    if (p.count < 1 || p.ch_grid < 1 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    xgrad_with_plan(p.p.N, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        XgradMultiParams q = p;
        q.p.tw2_off = (int)xgrad_wave_tw2_off<N>(p.p.M, p.p.win_n);
        hipLaunchKernelGGL(dmel_xgrad_wave_multi_kernel<N>, dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), xgrad_wave_lds<N>(p.p.M, p.p.win_n), s, q);
        e = hipGetLastError();
    });
    return e;
}

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
