// dmel_xgrad_multi.h -- what the K-window layers' units of the gradient w.r.t. the waveform share (dmel_xgrad.hip, dmel_xgrad_band.hip,
// dmel_xgrad_klen.hip): the body of the combine pass, written once for XgradCombineMultiParams and XgradCombineMultiLenParams, and the launcher
// of the four K-window builds of the wave-FFT kernel (dmel_xgrad_wave_body.inc).  Each unit keeps its own __global__ entry points.
#pragma once
#include "dmel_xgrad_plan.h"

namespace dmel {

// grid (chunks, B): the K-window layers' gradient w.r.t. the waveform, one launch per backward.  Every thread keeps 16 samples
// (i = lo + tid + 256 r: consecutive lanes read consecutive words) and adds the channels' terms in ascending channel order, starting from
// 0.f -- the sum autograd forms over K scalar layers.  A term is what the scalar path of that channel writes, from the same helpers
// (dmel_xgrad_plan.h): segments in increasing tile order minus the sequential fp64 tile-sum mean (xgrad_combine_body), or frame rows in
// increasing frame order minus the mean of the 256-wide fp64 tree (xgrad_gather_body).  One write of grad_x; no atomics.
// LEN (P = XgradCombineMultiLenParams): clip b ends at Lc.  A sample at or past it takes no segment and no frame row -- every term there is
// +0.0, so its sum stays the +0.0 it starts from (one test per sample, `i < end`: a second nesting level costs the 16 unrolled samples 32
// scalar registers of saved execution masks, which this kernel does not have) -- and only the clip's own tiles (q < ceil(Tc / fpt)) or
// frames (t < Tc) enter a sum: the workspace is plan-owned and the others hold what an earlier call left there.  A length outside 1 ... L
// writes NaN over the row (uniform over the workgroup: before any barrier).
template <class P>
__device__ __forceinline__ void xgrad_combine_multi_body(const P& p)
{
    constexpr bool LEN = std::is_same<P, XgradCombineMultiLenParams>::value;
    __shared__ double red[256];
    constexpr int PER = kXgChunk / 256;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    float* gx = p.grad_x + (size_t)b * p.L;
    int Lc = p.L, Tc = p.T, end = hi;                                 // the clip's samples and frames; samples of the chunk at or past `end` take no term
    if constexpr (LEN) {
        const ClipLen cl = clip_len(p.lengths, b, p.L, p.hop);
        if (!cl.ok) {
            for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
            return;
        }
        Lc = cl.Lc; Tc = cl.Tc;                                       // (Tc <= T: the launcher checks T = L / hop + 1)
        end = min(hi, Lc);
    }
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
            int ctiles = tiles;                                       // tiles of the clip that were computed
            if constexpr (LEN) ctiles = min(tiles, (Tc + p.fpt[c][j] - 1) / p.fpt[c][j]);
            const float* sg = p.frames[c] + (size_t)b * tiles * (size_t)span;
            const int u_lo = lo + half, u_hi = hi - 1 + half;
            const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
            const int qb = min(ctiles - 1, u_hi / ts);
            const float mean = xgrad_tile_mean(p.csum[c], b, tiles, ctiles, Lc);
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < end) acc[r] = acc[r] + (xgrad_segment_sum(sg, i + half, qa, qb, span, ts) - mean);
            });
        } else {
            __syncthreads();                                          // (red of the previous channel has been read)
            const float mean = xgrad_frame_mean(p.csum[c], (size_t)b * p.T, Tc, Lc, red, tid);
            const float* fr = p.frames[c] + (size_t)b * p.T * N;
            static_for<0, PER>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int i = lo + tid + 256 * r;
                if (i < end) acc[r] = acc[r] + (xgrad_frame_sum(fr, i, N, half, p.hop, Tc) - mean);
            });
        }
    }
    static_for<0, PER>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int i = lo + tid + 256 * r;
        if (i < hi) gx[i] = acc[r];
    });
}

// 0 <= e_0 <= e_1 <= ... <= e_kMaxChannels <= M (the host has validated the K + 1 edges of the layer and repeats the last one behind them)
static bool xgrad_band_edges_ok(const XgradBandParams& p)
{
    for (int c = 0; c < kMaxChannels; ++c)
        if (p.band_edges[c] < 0 || p.band_edges[c] > p.band_edges[c + 1] || p.band_edges[c + 1] > p.p.M) return false;
    return true;
}

// One wave-FFT launch for the `count` channels of ch_list at p.p.N (ch_grid = B x tiles workgroups each): P is one of XgradMultiParams,
// XgradBandParams, XgradMultiLenParams, XgradBandLenParams and kernel_of(IC<N>) its build of dmel_xgrad_wave_body.inc.  The four share the
// strictest checks any of them had: the spectrogram mode (these kernels have none) and the LDS fit are refusals the host never reaches --
// backward_x_multi_impl sets spec_mode = 0 and takes this path only where xgrad_wave_shape fits -- and `lengths` / `fpt` are checked where
// the parameters have them.
template <class P, class K> static hipError_t xgrad_launch_wave_multi(const P& p, K kernel_of, hipStream_t s)
{
    constexpr bool LEN = std::is_same<P, XgradMultiLenParams>::value || std::is_same<P, XgradBandLenParams>::value;
    const long long grid = (long long)p.count * p.ch_grid;
    if (p.count < 1 || p.ch_grid < 1 || grid > 0x7fffffffLL || p.p.spec_mode) return hipErrorInvalidValue;
    if constexpr (LEN) if (!p.lengths) return hipErrorInvalidValue;
    if constexpr (std::is_base_of<XgradBandParams, P>::value) if (!xgrad_band_edges_ok(p)) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    xgrad_with_plan(p.p.N, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        if constexpr (LEN) if (p.fpt != XgPlan<N>::FPT) return;
        const size_t lds = xgrad_wave_lds<N>(p.p.M, p.p.win_n);
        if (lds > (size_t)XgPlan<N>::LDS_MAX) return;
        P q = p;
        q.p.tw2_off = (int)xgrad_wave_tw2_off<N>(p.p.M, p.p.win_n);
        hipLaunchKernelGGL(kernel_of(nn), dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), lds, s, q);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace dmel
