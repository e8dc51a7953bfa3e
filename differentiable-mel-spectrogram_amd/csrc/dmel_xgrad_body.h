// dmel_xgrad_body.h -- the LDS radix-2 frames kernel, the gather and the combine pass of the gradient w.r.t. the waveform, and their launch
// logic, written once for the two parameter types: XgradParams (dmel_xgrad.hip: clips of n_points samples) and XgradLenParams
// (dmel_xgrad_len.hip: clips of per-clip lengths).  Each translation unit wraps the bodies in its own __global__ entry points and names them in
// a specialisation of XgKernels.
//
// What LEN (P = XgradLenParams) changes: every sample-space bound of a clip is Lc = lengths[b] instead of L and every frame-space bound
// Tc = Lc / hop + 1 instead of T (L and T stay the row strides); a pair of pad frames returns at once and the second pass reads neither its rows
// nor its sums (the workspace is plan-owned and holds what an earlier call left there); grad_x[b, Lc:] = 0; a length outside 1 ... L makes the row
// NaN; there is no spectrogram mode.  With Lc = L everywhere the arithmetic, operation by operation, is the fixed-length one.
#pragma once
#include "dmel_xgrad_plan.h"
#include "dmel_ldsfft.h"

namespace dmel {

// the bounds of clip b: its own length and frame count (LEN), or those of every clip
template <class P> __device__ __forceinline__ ClipLen xgrad_clip(const P& p, int b, int T)
{
    if constexpr (kXgLen<P>) return clip_len(p.lengths, b, p.L, p.hop);
    else return ClipLen{p.L, T, true};
}

// One workgroup per pair of frames, any power-of-two n_fft up to 16384 (see the head of dmel_xgrad.hip).
template <bool TWLDS, class P>
__device__ __forceinline__ void xgrad_frames_body(const P& p)
{
    constexpr bool LEN = kXgLen<P>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* Z = reinterpret_cast<float2*>(smem_raw);
    if (xgrad_not_this_nfft(p)) return;
    // twiddle table in LDS behind the sequence when it fits (n_fft <= 8192): every butterfly stage would otherwise wait for
    // a global (L1) load per twiddle, twenty-odd dependent round trips per workgroup
    float2* twl = Z + p.N;                                     // TWLDS only
    auto twiddle = [&](int k) -> float2 { if constexpr (TWLDS) return twl[k]; else return p.tw[k]; };
    const int tid = threadIdx.x;
    const int N = p.N, M = p.M, T = p.T, sh = 32 - p.logN;
    const int tiles = (T + 1) / 2;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int tA = 2 * tile, tB = tA + 1;
    const ClipLen cl = xgrad_clip(p, b, T);
    const int Lc = cl.Lc, Tc = cl.Tc;
    if constexpr (LEN) if (!cl.ok || tA >= Tc) return;
    const bool hasB = tB < Tc;
    const float* xb = p.x + (size_t)b * p.L;
    const float mean = clip_mean_psum(p.psum, p.nchunks, b, Lc);
    for (int n = tid; n < N; n += kXgThreads) {
        const long long ia = (long long)tA * p.hop - N / 2 + n, ib = ia + p.hop;
        const float va = (ia >= 0 && ia < Lc) ? (xb[ia] - mean) : 0.f;
        const float vb = (hasB && ib >= 0 && ib < Lc) ? (xb[ib] - mean) : 0.f;
        const float w = p.win2[n].x;
        Z[n] = make_float2(va * w, vb * w);
    }
    if constexpr (TWLDS) for (int k = tid; k < (N >> 1); k += kXgThreads) twl[k] = p.tw[k];
    __syncthreads();
    // forward: decimation in frequency, natural order in, bit-reversed order out
    lds_fft_dif<kXgThreads, false>(Z, N, p.logN, tid, twiddle);
    // spectra of the two frames, gradient of the power spectrum, conj(H_a) + i conj(H_b) back in place
    const float* ga = p.grad_out + (size_t)b * M * T + tA;
    const float* ya = p.out ? p.out + (size_t)b * M * T + tA : nullptr;
    const bool spec = !LEN && p.spec_mode;
    for (int k = tid; k <= (N >> 1); k += kXgThreads) {
        const unsigned ak = N > 1 ? __brev((unsigned)k) >> sh : 0u, an = N > 1 ? __brev((unsigned)((N - k) & (N - 1))) >> sh : 0u;
        const float2 zk = Z[ak], zn = Z[an];
        // X_a = (Z_k + conj Z_{N-k}) / 2,  X_b = (Z_k - conj Z_{N-k}) / (2i)
        const float xar = 0.5f * (zk.x + zn.x), xai = 0.5f * (zk.y - zn.y);
        const float xbr = 0.5f * (zk.y + zn.y), xbi = -0.5f * (zk.x - zn.x);
        float gpa = 0.f, gpb = 0.f;
        if (spec) {
            // DSPEC (models.py:171-200): the layer's output IS the power spectrogram, its gradient arrives per bin
            const float* gs = p.grad_out + ((size_t)b * p.F + k) * T + tA;
            gpa = gs[0];
            gpb = hasB ? gs[1] : 0.f;
        }
        const int2 band = spec ? make_int2(0, 0) : p.rowband[k];
        for (int m = band.x; m < band.y; ++m) {
            const float c = p.fb[(size_t)k * M + m];
            float g0 = ga[(size_t)m * T], g1 = hasB ? ga[(size_t)m * T + 1] : 0.f;
            if (ya) { g0 *= expf(-ya[(size_t)m * T]); if (hasB) g1 *= expf(-ya[(size_t)m * T + 1]); }
            gpa = fmaf(c, g0, gpa);
            gpb = fmaf(c, g1, gpb);
        }
        const bool edge = (k == 0) || (2 * k == N);
        const float sc = edge ? 2.f : 1.f;
        const float har = sc * gpa * xar, hai = edge ? 0.f : gpa * xai;      // X is real at k = 0 and N/2
        const float hbr = sc * gpb * xbr, hbi = edge ? 0.f : gpb * xbi;
        // U_k = conj(H_a,k + i H_b,k) = (har + hbi) + i (-(hai) + ... ): conj(a + i b) with a = har + i hai, b = hbr + i hbi
        //     = conj(har - hbi + i (hai + hbr)) = (har - hbi) - i (hai + hbr)
        Z[ak] = make_float2(har - hbi, -(hai + hbr));
        // k' = N - k carries conj(H_a,k) + i conj(H_b,k) = (har + hbi) + i (hbr - hai); conjugated: (har + hbi) - i (hbr - hai)
        if (!edge) Z[an] = make_float2(har + hbi, hai - hbr);
    }
    __syncthreads();
    // decimation in time, bit-reversed order in, natural order out: R = FFT(conj W) = conj(dv_a + i dv_b)
    lds_fft_dit<kXgThreads, false>(Z, N, p.logN, tid, twiddle);
    float* fa = p.frames + ((size_t)b * T + tA) * N;
    double sa = 0.0, sb = 0.0;                                 // what each frame contributes to the sum of the clip's gradient
    for (int n = tid; n < N; n += kXgThreads) {
        const float2 r = Z[n];
        const float w = p.win2[n].x;
        const float va = r.x * w, vb = -r.y * w;
        fa[n] = va;
        if (hasB) fa[N + n] = vb;
        const long long ia = (long long)tA * p.hop - N / 2 + n, ib = ia + p.hop;
        if (ia >= 0 && ia < Lc) sa += (double)va;
        if (hasB && ib >= 0 && ib < Lc) sb += (double)vb;
    }
    // fixed-order tree over the 256 threads (the sequence is dead: its first 4 KB hold the partials)
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem_raw);
    red[tid] = sa; red[kXgThreads + tid] = sb;
    __syncthreads();
    for (int o = kXgThreads / 2; o > 0; o >>= 1) {
        if (tid < o) { red[tid] += red[tid + o]; red[kXgThreads + tid] += red[kXgThreads + tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { p.csum[(size_t)b * T + tA] = red[0]; if (hasB) p.csum[(size_t)b * T + tB] = red[kXgThreads]; }
}

// grid (chunks, B): every workgroup overlap-adds one chunk of kXgChunk samples of one clip as a gather in increasing frame
// order (deterministic, no atomics) and subtracts the mean of the clip's gradient (models.py:38 removes the clip's DC, so the
// gradient has none either).  The mean comes from the per-frame sums the first kernel left: every workgroup adds them up in the
// same fixed order (strided partial sums, then a tree), so every chunk of a clip subtracts the same bits.
template <class P>
__device__ __forceinline__ void xgrad_gather_body(const P& p)
{
    constexpr bool LEN = kXgLen<P>;
    __shared__ double red[256];
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int N = p.N, T = p.T, hop = p.hop, half = N / 2;
    const ClipLen cl = xgrad_clip(p, b, T);
    const int Lc = cl.Lc, Tc = min(cl.Tc, T);
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    if constexpr (LEN) if (!cl.ok) {
        for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
        return;
    }
    float mean = 0.f;
    if (p.remove_dc) mean = xgrad_frame_mean(p.csum, (size_t)b * T, Tc, Lc, red, tid);
    const float* fr = p.frames + (size_t)b * T * N;
    for (int i = lo + tid; i < hi; i += 256) {
        float v = 0.f;
        if (!LEN || i < Lc) v = xgrad_frame_sum(fr, i, N, half, hop, Tc) - mean;
        gx[i] = v;
    }
}

// grid (chunks, B): clip sample i is covered by the segments of tiles q with q TS - N/2 <= i < q TS - N/2 + span (TS = FPT hop
// samples between tile starts); they are added in increasing q and the mean of the clip's gradient is subtracted.  LEN: only the
// tiles q < ceil(Tc / FPT) of the clip were computed.
template <class P>
__device__ __forceinline__ void xgrad_combine_body(const P& p)
{
    constexpr bool LEN = kXgLen<P>;
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int tiles = p.tiles, span = p.span, ts = p.tile_step, half = p.N / 2;
    const ClipLen cl = xgrad_clip(p, b, p.T);
    const int Lc = cl.Lc;
    int ctiles = tiles;                                          // tiles of the clip that were computed
    if constexpr (LEN) ctiles = min(tiles, (cl.Tc + p.fpt - 1) / p.fpt);
    const float* sg = p.frames + (size_t)b * tiles * (size_t)span;
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    if constexpr (LEN) if (!cl.ok) {
        for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
        return;
    }
    const int end = LEN ? Lc : hi;                               // samples of the chunk at or past it take no segment
    // tiles that can cover a sample of this chunk: two divisions per workgroup, a range test per sample and tile
    const int u_lo = lo + half, u_hi = hi - 1 + half;
    const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
    const int qb = min(ctiles - 1, u_hi / ts);
    // rows of four samples when every row involved starts on a 16-byte boundary (hop, n_fft / 2 and the row stride multiples of 4) and,
    // LEN, the clip ends between two rows (Lc a multiple of 4: a row is inside the clip or past it as a whole)
    const bool vec = ((p.hop | half | p.L | span | (LEN ? Lc : 0)) & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.frames) | reinterpret_cast<uintptr_t>(p.grad_x)) & 15) == 0;
    if (vec) {
        constexpr int PER = kXgChunk / (256 * 4);                  // rows of 4 per thread
        float4 acc[PER];
        static_for<0, PER>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            const int i = lo + (tid + 256 * r) * 4;
            acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < end) {
                const int u = i + half;
                for (int q = qa; q <= qb; ++q) {
                    const int off = u - q * ts;                   // a multiple of 4: the four samples are inside or outside together
                    if (off >= 0 && off < span) {
                        const float4 v = *reinterpret_cast<const float4*>(sg + (size_t)q * span + off);
                        acc[r].x += v.x; acc[r].y += v.y; acc[r].z += v.z; acc[r].w += v.w;
                    }
                }
            }
        });
        const float mean = p.remove_dc ? xgrad_tile_mean(p.csum, b, tiles, ctiles, Lc) : 0.f;   // (its loads travel with the segment loads above)
        static_for<0, PER>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            const int i = lo + (tid + 256 * r) * 4;
            if (i < hi)
                *reinterpret_cast<float4*>(gx + i) = i < end ? make_float4(acc[r].x - mean, acc[r].y - mean, acc[r].z - mean, acc[r].w - mean)
                                                             : make_float4(0.f, 0.f, 0.f, 0.f);
        });
        return;
    }
    const float mean = p.remove_dc ? xgrad_tile_mean(p.csum, b, tiles, ctiles, Lc) : 0.f;
    #pragma unroll 4
    for (int i = lo + tid; i < hi; i += 256) {
        gx[i] = i < end ? xgrad_segment_sum(sg, i + half, qa, qb, span, ts) - mean : 0.f;
    }
}

// ---- launch logic -------------------------------------------------------------------------------------------------------------------------
// the __global__ entry points over the bodies above and the wave-FFT kernel of dmel_xgrad_wave_body.inc for the parameter type P: members
// frames<TWLDS>, gather, combine and wave<N>, specialised by the translation unit that defines them
template <class P> struct XgKernels;

template <class P> static hipError_t xgrad_launch_frames(const P& p, hipStream_t s)
{
    const long long grid = (long long)p.B * ((p.T + 1) / 2);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    P q = p;
    q.tw_in_lds = p.N <= 8192 ? 1 : 0;
    size_t lds = (size_t)p.N * sizeof(float2) + (q.tw_in_lds ? (size_t)(p.N / 2) * sizeof(float2) : 0);
    if (lds < 2 * kXgThreads * sizeof(double)) lds = 2 * kXgThreads * sizeof(double);      // the per-frame sums are reduced where the sequence was
    if (q.tw_in_lds) hipLaunchKernelGGL(XgKernels<P>::template frames<true>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    else hipLaunchKernelGGL(XgKernels<P>::template frames<false>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    return hipGetLastError();
}

template <class P> static hipError_t xgrad_launch_second(void (*kernel)(P), const P& p, hipStream_t s)      // the gather or the combine pass
{
    const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)p.B);
    hipLaunchKernelGGL(kernel, g2, dim3(256), 0, s, p);
    return hipGetLastError();
}

// wave-FFT path (p.tiles > 0): (B x tiles) workgroups, then the combine pass; otherwise the frames kernel, then the gather
template <class P> static hipError_t xgrad_launch(const P& p, hipStream_t s)
{
    if (p.tiles == 0) {
        const hipError_t e = xgrad_launch_frames(p, s);
        return e != hipSuccess ? e : xgrad_launch_second(XgKernels<P>::gather, p, s);
    }
    const long long grid = (long long)p.B * p.tiles;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const int M = p.spec_mode ? 0 : p.M;
    hipError_t e = hipErrorInvalidValue;
    xgrad_with_plan(p.N, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        if constexpr (kXgLen<P>) if (p.fpt != XgPlan<N>::FPT) return;
        P q = p;
        q.tw2_off = (int)xgrad_wave_tw2_off<N>(M, p.win_n);
        hipLaunchKernelGGL(XgKernels<P>::template wave<N>, dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), xgrad_wave_lds<N>(M, p.win_n), s, q);
        e = hipGetLastError();
    });
    return e != hipSuccess ? e : xgrad_launch_second(XgKernels<P>::combine, p, s);
}

// raises the dynamic-LDS limit of P's frames and wave kernels
template <class P> static hipError_t xgrad_set_attributes()
{
    auto set = [](auto kernel, int bytes) { return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
    hipError_t e = set(XgKernels<P>::template frames<false>, kMaxNfft * (int)sizeof(float2));
    if (e == hipSuccess) e = set(XgKernels<P>::template frames<true>, 8192 * 12);
    return e != hipSuccess ? e : xgrad_set_wave_attributes([](auto nn) { return XgKernels<P>::template wave<decltype(nn)::value>; });
}

}  // namespace dmel
