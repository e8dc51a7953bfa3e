// dmel_xgrad_plan.h -- what the four translation units of the gradient w.r.t. the waveform share:
//   dmel_xgrad.hip       clips of n_points samples: the scalar layer, the multi-window layer's wave kernel and combine pass
//   dmel_xgrad_len.hip   the scalar layer over clips of per-clip lengths
//   dmel_xgrad_band.hip  the band-split layer's wave kernel and its staging kernel
//   dmel_xgrad_klen.hip  the K-window layers over clips of per-clip lengths
// The geometry of the wave-FFT kernel (csrc/dmel_xgrad_wave_body.inc), its LDS layout, the dispatch over n_fft, the clip-length load and the
// per-sample arithmetic of the second pass: every kernel that forms a sample of grad_x takes its sums and its mean from the four helpers at
// the end of this file, which is what makes the K-window layers' x.grad the K scalar layers' sum bit for bit.  (The launch parameters are in
// dmel_kernels.h; the scalar kernels' bodies and launch logic in dmel_xgrad_body.h, the K-window ones in dmel_xgrad_multi.h.)
#pragma once
#include <type_traits>
#include "dmel_kernels.h"
#include "dmel_wavefft.h"

namespace dmel {

constexpr int kXgThreads = 256;

// DMEL_FLAG_CHECK_NFFT (the optimized=True layer with x.requires_grad and lambd left on the device): the step's forward ran one
// launch per candidate n_fft and only the one lambd asks for did the work (lam_prologue); the backward does the same
__device__ __forceinline__ bool xgrad_not_this_nfft(const XgradParams& p)
{
    return p.check_nfft && p.lam_dev && lam_n_fft(__builtin_fabsf(*(const __attribute__((address_space(4))) float*)p.lam_dev)) != p.N;
}

// the length-aware build of a kernel body or launcher: its parameters carry the per-clip lengths
template <class P> constexpr bool kXgLen = std::is_same<P, XgradLenParams>::value;

// the clip's length: one scalar load, uniform over the workgroup (as dmel_fwd_len_kernel); an invalid one reads as 1 until the caller returns
struct ClipLen { int Lc, Tc; bool ok; };
__device__ __forceinline__ ClipLen clip_len(const int* lengths, int b, int L, int hop)
{
    const int raw = *(const __attribute__((address_space(4))) int*)(lengths + b);
    ClipLen c;
    c.ok = raw >= 1 && raw <= L;
    c.Lc = __builtin_amdgcn_readfirstlane(c.ok ? raw : 1);
    c.Tc = c.Lc / hop + 1;
    return c;
}

// samples of a clip per workgroup of the gather / combine kernels
constexpr int kXgChunk = 4096;

template <int N> struct XgPlan {
    using P = FftPlanSel<N, true>;
    static constexpr int R = P::R, C = P::C, G = N / R, FPW = 64 / G;
    // (2048 with 8 waves -- one workgroup per CU, 16-frame tiles: kernel 81 us against 77 at BASELINE config 3, combine pass 8.8 against 10.1)
    static constexpr int WAVES = (N == 1024) ? 8 : 4;
    static constexpr int LDS_MAX = 80 * 1024;                          // two workgroups per CU
    static constexpr int SLOTS = WAVES * FPW, FPT = 2 * SLOTS, THREADS = 64 * WAVES;
    static constexpr int SS = slot_stride_f2(N, R, C, 0, 0);          // float2 entries per slot
    static constexpr int MINW = (N >= 2048) ? 2 : 4;                   // waves per SIMD the LDS footprint admits
    static constexpr int PADP = (R == 16 && C > 1) ? 16 : 0;           // the C groups of 16 lanes write a plane on different banks
};

template <int N> static size_t xgrad_wave_tw2_off(int M, int win_n)
{
    using PL = XgPlan<N>;
    size_t gm = (size_t)(M + 1) * PL::FPT * sizeof(float);          // one zero row behind the last mel band
    if (gm < PL::THREADS * sizeof(double)) gm = PL::THREADS * sizeof(double);
    return (size_t)PL::SLOTS * PL::SS * 8 + (size_t)((win_n + 3) & ~3) * sizeof(float) + gm;
}

template <int N> static size_t xgrad_wave_lds(int M, int win_n)
{
    using PL = XgPlan<N>;
    return xgrad_wave_tw2_off<N>(M, win_n) + (PL::C > 1 ? (size_t)PL::R * PL::C * 8 : 0) + 64;      // + one partial sum per wave
}

template <class F> static bool xgrad_with_plan(int n, F&& f)
{
    switch (n) {
    case 32: f(IC<32>{}); return true;
    case 64: f(IC<64>{}); return true;
    case 128: f(IC<128>{}); return true;
    case 256: f(IC<256>{}); return true;
    case 512: f(IC<512>{}); return true;
    case 1024: f(IC<1024>{}); return true;
    case 2048: f(IC<2048>{}); return true;
    default: return false;
    }
}

// raises the dynamic-LDS limit of the wave-FFT kernels kernel_of(IC<N>) names, n_fft 32 ... 2048
template <class K> static hipError_t xgrad_set_wave_attributes(K kernel_of)
{
    hipError_t e = hipSuccess;
    for (int n = 32; n <= 2048 && e == hipSuccess; n *= 2)
        xgrad_with_plan(n, [&](auto nn) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_of(nn)), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<decltype(nn)::value>::LDS_MAX);
        });
    return e;
}

// ---- a sample of grad_x: s - mean ---------------------------------------------------------------------------------------------------------
// The one copy of the second pass's arithmetic (gather, combine and the K-window combine).  The order of the additions is the contract.

// wave path: the segments (span samples each, tile starts ts apart) that cover clip sample u - n_fft / 2, tiles qa ... qb in increasing order
__device__ __forceinline__ float xgrad_segment_sum(const float* sg, int u, int qa, int qb, int span, int ts)
{
    float s = 0.f;
    for (int q = qa; q <= qb; ++q) {
        const int off = u - q * ts;
        if (off >= 0 && off < span) s += sg[(size_t)q * span + off];
    }
    return s;
}

// LDS path: the rows of fr (Tc frames of N samples) with 0 <= i - t hop + half < N (half = N / 2), in increasing t
__device__ __forceinline__ float xgrad_frame_sum(const float* fr, int i, int N, int half, int hop, int Tc)
{
    int t_lo = i + half - N + 1;
    t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
    int t_hi = (i + half) / hop;
    if (t_hi > Tc - 1) t_hi = Tc - 1;
    float s = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) s += fr[(size_t)t * N + (i - t * hop + half)];
    return s;
}

// wave path: the first ctiles of clip b's fp64 tile sums (rows of `tiles`) added one after the other (uniform: every thread adds the same
// values in the same order), over Lc
__device__ __forceinline__ float xgrad_tile_mean(const double* csum, int b, int tiles, int ctiles, int Lc)
{
    double acc = 0.0;
    for (int q = 0; q < ctiles; ++q) acc += csum[(size_t)b * tiles + q];
    return (float)(acc / (double)Lc);
}

// LDS path: the clip's Tc fp64 frame sums csum[row ...] as 256 strided partial sums and a tree over them in red (256 doubles of LDS; every
// thread of the workgroup calls, barriers inside, and nobody is still reading red), over Lc
__device__ __forceinline__ float xgrad_frame_mean(const double* csum, size_t row, int Tc, int Lc, double* red, int tid)
{
    double acc = 0.0;
    for (int t = tid; t < Tc; t += 256) acc += csum[row + t];
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    return (float)(red[0] / (double)Lc);
}

}  // namespace dmel
