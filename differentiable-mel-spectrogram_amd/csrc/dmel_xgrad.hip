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
#include "dmel_xgrad_plan.h"
#include "dmel_ldsfft.h"

namespace dmel {

// (dmel_xgrad_len.hip holds a copy of this kernel with per-clip bounds, dmel_xgrad_frames_len_kernel: a fix here belongs there too)
template <bool TWLDS>
__global__ void __launch_bounds__(kXgThreads) dmel_xgrad_frames_kernel(XgradParams p)
{
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
    const bool hasB = tB < T;
    const float* xb = p.x + (size_t)b * p.L;
    float mean = 0.f;
    {
        mean = clip_mean_psum(p.psum, p.nchunks, b, p.L);
    }
    for (int n = tid; n < N; n += kXgThreads) {
        const long long ia = (long long)tA * p.hop - N / 2 + n, ib = ia + p.hop;
        const float va = (ia >= 0 && ia < p.L) ? (xb[ia] - mean) : 0.f;
        const float vb = (hasB && ib >= 0 && ib < p.L) ? (xb[ib] - mean) : 0.f;
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
    for (int k = tid; k <= (N >> 1); k += kXgThreads) {
        const unsigned ak = N > 1 ? __brev((unsigned)k) >> sh : 0u, an = N > 1 ? __brev((unsigned)((N - k) & (N - 1))) >> sh : 0u;
        const float2 zk = Z[ak], zn = Z[an];
        // X_a = (Z_k + conj Z_{N-k}) / 2,  X_b = (Z_k - conj Z_{N-k}) / (2i)
        const float xar = 0.5f * (zk.x + zn.x), xai = 0.5f * (zk.y - zn.y);
        const float xbr = 0.5f * (zk.y + zn.y), xbi = -0.5f * (zk.x - zn.x);
        float gpa = 0.f, gpb = 0.f;
        if (p.spec_mode) {
            // DSPEC (models.py:171-200): the layer's output IS the power spectrogram, its gradient arrives per bin
            const float* gs = p.grad_out + ((size_t)b * p.F + k) * T + tA;
            gpa = gs[0];
            gpb = hasB ? gs[1] : 0.f;
        }
        const int2 band = p.spec_mode ? make_int2(0, 0) : p.rowband[k];
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
        if (ia >= 0 && ia < p.L) sa += (double)va;
        if (hasB && ib >= 0 && ib < p.L) sb += (double)vb;
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
__global__ void __launch_bounds__(256) dmel_xgrad_gather_kernel(XgradParams p)
{
    __shared__ double red[256];
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int N = p.N, T = p.T, hop = p.hop, half = N / 2;
    float mean = 0.f;
    if (p.remove_dc) {
        double acc = 0.0;
        for (int t = tid; t < T; t += 256) acc += p.csum[(size_t)b * T + t];
        red[tid] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        mean = (float)(red[0] / (double)p.L);
    }
    const float* fr = p.frames + (size_t)b * T * N;
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    for (int i = lo + tid; i < hi; i += 256) {
        // frames with 0 <= i - t hop + N/2 < N, in increasing t
        int t_lo = i + half - N + 1;
        t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
        int t_hi = (i + half) / hop;
        if (t_hi > T - 1) t_hi = T - 1;
        float s = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) s += fr[(size_t)t * N + (i - t * hop + half)];
        gx[i] = s - mean;
    }
}

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

// grid (chunks, B): clip sample i is covered by the segments of tiles q with q TS - N/2 <= i < q TS - N/2 + span (TS = FPT hop
// samples between tile starts); they are added in increasing q and the mean of the clip's gradient is subtracted
__global__ void __launch_bounds__(256) dmel_xgrad_combine_kernel(XgradParams p)
{
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int tiles = p.tiles, span = p.span, ts = p.tile_step, half = p.N / 2;
    const float* sg = p.frames + (size_t)b * tiles * (size_t)span;
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    // tiles that can cover a sample of this chunk: two divisions per workgroup, a range test per sample and tile
    const int u_lo = lo + half, u_hi = hi - 1 + half;
    const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
    const int qb = min(tiles - 1, u_hi / ts);
    auto clip_mean = [&]() {
        float mean = 0.f;
        if (p.remove_dc) {
            double acc = 0.0;
            for (int q = 0; q < tiles; ++q) acc += p.csum[(size_t)b * tiles + q];  // uniform: every thread adds the same values in the same order
            mean = (float)(acc / (double)p.L);
        }
        return mean;
    };
    // rows of four samples when every row involved starts on a 16-byte boundary (hop, n_fft / 2 and the clip length multiples of 4)
    const bool vec = ((p.hop | half | p.L | span) & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.frames) | reinterpret_cast<uintptr_t>(p.grad_x)) & 15) == 0;
    if (vec) {
        constexpr int PER = kXgChunk / (256 * 4);                  // rows of 4 per thread
        float4 acc[PER];
        static_for<0, PER>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            const int i = lo + (tid + 256 * r) * 4;
            acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < hi) {
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
        const float mean = clip_mean();                            // (its loads travel with the segment loads above)
        static_for<0, PER>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            const int i = lo + (tid + 256 * r) * 4;
            if (i < hi) *reinterpret_cast<float4*>(gx + i) = make_float4(acc[r].x - mean, acc[r].y - mean, acc[r].z - mean, acc[r].w - mean);
        });
        return;
    }
    const float mean = clip_mean();
    #pragma unroll 4
    for (int i = lo + tid; i < hi; i += 256) {
        const int u = i + half;
        float s = 0.f;
        for (int q = qa; q <= qb; ++q) {
            const int off = u - q * ts;
            if (off >= 0 && off < span) s += sg[(size_t)q * span + off];
        }
        gx[i] = s - mean;
    }
}

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

hipError_t xgrad_prepare_attributes()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_frames_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kMaxNfft * (int)sizeof(float2));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_frames_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 12);
    for (int n = 32; n <= 2048 && e == hipSuccess; n *= 2)
        xgrad_with_plan(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<N>::LDS_MAX);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        XgPlan<N>::LDS_MAX);
        });
    return e;
}

hipError_t launch_xgrad(const XgradParams& p, hipStream_t s)
{
    if (p.tiles > 0) {
        // wave-FFT path: (B x tiles) workgroups, then the combine pass
        const long long grid = (long long)p.B * p.tiles;
        if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
        hipError_t e = hipErrorInvalidValue;
        xgrad_with_plan(p.N, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            XgradParams q = p;
            q.tw2_off = (int)xgrad_wave_tw2_off<N>(p.spec_mode ? 0 : p.M, p.win_n);
            hipLaunchKernelGGL(dmel_xgrad_wave_kernel<N>, dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), xgrad_wave_lds<N>(p.spec_mode ? 0 : p.M, p.win_n), s, q);
            e = hipGetLastError();
        });
        if (e != hipSuccess) return e;
        const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)p.B);
        hipLaunchKernelGGL(dmel_xgrad_combine_kernel, g2, dim3(256), 0, s, p);
        return hipGetLastError();
    }
    hipError_t e = launch_xgrad_frames(p, s);
    if (e != hipSuccess) return e;
    return launch_xgrad_gather(p, s);
}

hipError_t launch_xgrad_frames(const XgradParams& p, hipStream_t s)
{
    const long long grid = (long long)p.B * ((p.T + 1) / 2);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    XgradParams q = p;
    q.tw_in_lds = p.N <= 8192 ? 1 : 0;
    size_t lds = (size_t)p.N * sizeof(float2) + (q.tw_in_lds ? (size_t)(p.N / 2) * sizeof(float2) : 0);
    if (lds < 2 * kXgThreads * sizeof(double)) lds = 2 * kXgThreads * sizeof(double);      // the per-frame sums are reduced where the sequence was
    if (q.tw_in_lds) hipLaunchKernelGGL(dmel_xgrad_frames_kernel<true>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    else hipLaunchKernelGGL(dmel_xgrad_frames_kernel<false>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    return hipGetLastError();
}

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

hipError_t launch_xgrad_gather(const XgradParams& p, hipStream_t s)
{
    const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)p.B);
    hipLaunchKernelGGL(dmel_xgrad_gather_kernel, g2, dim3(256), 0, s, p);
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
