// dmel_xgrad_klen.hip -- the K-window layers' gradient w.r.t. the waveform over clips of per-clip lengths
// (MultiWindowMelSpectrogram / BandSplitMelSpectrogram(lengths_waveform_grad=True), dmel_backward_x_multi_lengths, dmel_backward_x_band_lengths
// and their _dev forms): the product of dmel_xgrad_len.hip (clip bounds from Lc = lengths[b], Tc = Lc / hop + 1) with the channel slot of
// dmel_xgrad_wave_multi_kernel and the row range of dmel_xgrad_wave_band_kernel.  dmel_xgrad_wave_multi_len_kernel<N> and
// dmel_xgrad_wave_band_len_kernel<N> are two more builds of dmel_xgrad_wave_body.inc; dmel_xgrad_combine_multi_len_kernel adds the channels'
// terms in ascending channel order, every term formed as dmel_xgrad_combine_len_kernel (wave path) or dmel_xgrad_gather_len_kernel (LDS
// path) forms it: s - mean inside the clip, +0.0 past it.  The LDS path runs dmel_xgrad_len.hip's frames kernel per channel on the staged
// rows (launch_xgrad_frames_len).  A translation unit of its own: the kernels of dmel_xgrad.hip, dmel_xgrad_len.hip and
// dmel_xgrad_band.hip keep their code.
#include "dmel_xgrad_plan.h"

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

// grid (chunks, B), as dmel_xgrad_combine_multi_kernel: 16 samples per thread, the channels' terms added to 0.f in ascending channel order, one
// write of grad_x, no atomics.  Clip b ends at Lc: a sample at or past it takes no segment and no frame row -- every term there is +0.0,
// so its sum stays the +0.0 it starts from (one test per sample, `i < end`: a second nesting level costs the 16 unrolled samples 32 scalar
// registers of saved execution masks, which this kernel does not have) -- and only the clip's own tiles (q < ceil(Tc / fpt)) or frames (t < Tc) enter a sum: the workspace is plan-owned and the others hold what
// an earlier call left there.  A length outside 1 ... L writes NaN over the row (uniform over the workgroup: before any barrier).
__global__ void __launch_bounds__(256) dmel_xgrad_combine_multi_len_kernel(XgradCombineMultiLenParams p)
{
    __shared__ double red[256];
    constexpr int PER = kXgChunk / 256;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    float* gx = p.grad_x + (size_t)b * p.L;
    const ClipLen cl = clip_len(p.lengths, b, p.L, p.hop);
    if (!cl.ok) {
        for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
        return;
    }
    const int Lc = cl.Lc, Tc = cl.Tc;                                 // (Tc <= T: the launcher checks T = L / hop + 1)
    const int end = min(hi, Lc);                                      // samples of the chunk at or past it take no term
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
            const int span = p.span[c][j], ts = p.tile_step[c][j], fpt = p.fpt[c][j];
            const int ctiles = min(tiles, (Tc + fpt - 1) / fpt);  // tiles of the clip that were computed
            const float* sg = p.frames[c] + (size_t)b * tiles * (size_t)span;
            const int u_lo = lo + half, u_hi = hi - 1 + half;
            const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
            const int qb = min(ctiles - 1, u_hi / ts);
            double dacc = 0.0;
            for (int q = 0; q < ctiles; ++q) dacc += p.csum[c][(size_t)b * tiles + q];
            const float mean = (float)(dacc / (double)Lc);
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < end) {
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
            for (int t = tid; t < Tc; t += 256) dacc += p.csum[c][(size_t)b * T + t];
            red[tid] = dacc;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
            const float mean = (float)(red[0] / (double)Lc);
            const float* fr = p.frames[c] + (size_t)b * T * N;
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < end) {
                    int t_lo = i + half - N + 1;
                    t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
                    int t_hi = (i + half) / hop;
                    if (t_hi > Tc - 1) t_hi = Tc - 1;
                    float s = 0.f;
                    for (int t = t_lo; t <= t_hi; ++t) s += fr[(size_t)t * N + (i - t * hop + half)];
                    acc[r] = acc[r] + (s - mean);
                }
            });
        }
    }
    static_for<0, PER>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int i = lo + tid + 256 * r;
        if (i < hi) gx[i] = acc[r];
    });
}

hipError_t xgrad_klen_prepare_attributes()
{
    hipError_t e = hipSuccess;
    for (int n = 32; n <= 2048 && e == hipSuccess; n *= 2)
        xgrad_with_plan(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_multi_len_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<N>::LDS_MAX);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_band_len_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<N>::LDS_MAX);
        });
    return e;
}

// one wave-FFT launch for the `count` channels of ch_list at p.p.N (ch_grid = B x tiles workgroups each), as launch_xgrad_wave_multi / _band
template <class P, class K> static hipError_t xgrad_klen_launch_wave(const P& p, K kernel_of, hipStream_t s)
{
    const long long grid = (long long)p.count * p.ch_grid;
    if (p.count < 1 || p.ch_grid < 1 || grid > 0x7fffffffLL || p.p.spec_mode || !p.lengths) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    xgrad_with_plan(p.p.N, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        if (p.fpt != XgPlan<N>::FPT) return;
        if (xgrad_wave_lds<N>(p.p.M, p.p.win_n) > (size_t)XgPlan<N>::LDS_MAX) return;
        P q = p;
        q.p.tw2_off = (int)xgrad_wave_tw2_off<N>(p.p.M, p.p.win_n);
        hipLaunchKernelGGL(kernel_of(nn), dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), xgrad_wave_lds<N>(p.p.M, p.p.win_n), s, q);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_xgrad_wave_multi_len(const XgradMultiLenParams& p, hipStream_t s)
{
    return xgrad_klen_launch_wave(p, [](auto nn) { return dmel_xgrad_wave_multi_len_kernel<decltype(nn)::value>; }, s);
}

hipError_t launch_xgrad_wave_band_len(const XgradBandLenParams& p, hipStream_t s)
{
    for (int c = 0; c < kMaxChannels; ++c)
        if (p.band_edges[c] < 0 || p.band_edges[c] > p.band_edges[c + 1] || p.band_edges[c + 1] > p.p.M) return hipErrorInvalidValue;
    return xgrad_klen_launch_wave(p, [](auto nn) { return dmel_xgrad_wave_band_len_kernel<decltype(nn)::value>; }, s);
}

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
