// dmel_xgrad_len.hip -- the gradient w.r.t. the waveform over clips of per-clip lengths (MelSpectrogramLayer(lengths_waveform_grad=True),
// dmel_backward_x_lengths / dmel_backward_x_dev_lengths): the kernels of dmel_xgrad.hip with every sample-space bound of a clip (buffer
// resource, interior test, load clamps, the zeroing at windowing time, the clip sum and its quotient, the in-clip test of the gradient's
// own sum) taken from Lc = lengths[b] and every frame-space bound from Tc = Lc / hop + 1.  L stays the row stride of x / grad_x and T
// the row stride of grad_out / out.  A pad frame (t >= Tc) has a zero mel gradient, so one that shares its complex FFT with a frame of the
// clip contributes H = 0; a tile (wave path) or a pair (LDS path) of pad frames only does nothing at all, and the second pass reads
// neither its segment nor its sum: the workspace is plan-owned and holds what an earlier call left there.  grad_x[b, Lc:] = 0; a length
// outside 1 ... L makes the row NaN.  With Lc = L everywhere the arithmetic, operation by operation, is that of dmel_xgrad.hip.
// A translation unit of its own: dmel_xgrad.hip's kernels are compiled exactly as before.
#include "dmel_xgrad_plan.h"
#include "dmel_ldsfft.h"

namespace dmel {

#define XSTAMP(i) do {} while (0)

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

// ---- wave path (n_fft 32 ... 2048): dmel_xgrad_wave_len_kernel<N> ---------------------------------------------------------------------
#define DMEL_XG_MULTI 0
#define DMEL_XG_LEN 1
#include "dmel_xgrad_wave_body.inc"
#undef DMEL_XG_LEN
#undef DMEL_XG_MULTI

// grid (chunks, B): dmel_xgrad_combine_kernel over the tiles q < ceil(Tc / FPT) of the clip -- the others were skipped: their segments and
// sums are stale -- in increasing q, minus the sequential fp64 sum of those tiles' csum divided by Lc
__global__ void __launch_bounds__(256) dmel_xgrad_combine_len_kernel(XgradLenParams p)
{
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int tiles = p.tiles, span = p.span, ts = p.tile_step, half = p.N / 2;
    const ClipLen cl = clip_len(p.lengths, b, p.L, p.hop);
    const int Lc = cl.Lc;
    const int ctiles = min(tiles, (cl.Tc + p.fpt - 1) / p.fpt);   // tiles of the clip that were computed
    const float* sg = p.frames + (size_t)b * tiles * (size_t)span;
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    if (!cl.ok) {
        for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
        return;
    }
    const int u_lo = lo + half, u_hi = hi - 1 + half;
    const int qa = u_lo < span ? 0 : (u_lo - span) / ts + 1;
    const int qb = min(ctiles - 1, u_hi / ts);
    auto clip_mean = [&]() {
        float mean = 0.f;
        if (p.remove_dc) {
            double acc = 0.0;
            for (int q = 0; q < ctiles; ++q) acc += p.csum[(size_t)b * tiles + q];  // uniform: every thread adds the same values in the same order
            mean = (float)(acc / (double)Lc);
        }
        return mean;
    };
    // rows of four samples when every row involved starts on a 16-byte boundary (hop, n_fft / 2 and the row stride multiples of 4) and the
    // clip ends between two rows (Lc a multiple of 4: a row is inside the clip or past it as a whole)
    const bool vec = ((p.hop | half | p.L | span | Lc) & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.frames) | reinterpret_cast<uintptr_t>(p.grad_x)) & 15) == 0;
    if (vec) {
        constexpr int PER = kXgChunk / (256 * 4);                  // rows of 4 per thread
        float4 acc[PER];
        static_for<0, PER>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            const int i = lo + (tid + 256 * r) * 4;
            acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < Lc) {
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
            if (i < hi)
                *reinterpret_cast<float4*>(gx + i) = i < Lc ? make_float4(acc[r].x - mean, acc[r].y - mean, acc[r].z - mean, acc[r].w - mean)
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
        });
        return;
    }
    const float mean = clip_mean();
    #pragma unroll 4
    for (int i = lo + tid; i < hi; i += 256) {
        const int u = i + half;
        float s = 0.f;
        if (i < Lc)
            for (int q = qa; q <= qb; ++q) {
                const int off = u - q * ts;
                if (off >= 0 && off < span) s += sg[(size_t)q * span + off];
            }
        gx[i] = i < Lc ? s - mean : 0.f;
    }
}

// ---- LDS path (n_fft 4096 ... 16384, and shapes the wave path refuses) ------------------------------------------------------------------
// dmel_xgrad_frames_kernel: one workgroup per pair of frames; a pair of pad frames returns at once (its rows of the frame workspace and its
// sums stay stale, the gather reads neither).  A COPY of dmel_xgrad_frames_kernel (dmel_xgrad.hip) with the clip's bounds and without the
// spectrogram mode, kept apart so that dmel_xgrad.hip's object does not change: a fix to the transform, the separation of the two spectra or
// the reduction belongs in both.
template <bool TWLDS>
__global__ void __launch_bounds__(kXgThreads) dmel_xgrad_frames_len_kernel(XgradLenParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* Z = reinterpret_cast<float2*>(smem_raw);
    if (xgrad_not_this_nfft(p)) return;
    float2* twl = Z + p.N;                                     // TWLDS only
    auto twiddle = [&](int k) -> float2 { if constexpr (TWLDS) return twl[k]; else return p.tw[k]; };
    const int tid = threadIdx.x;
    const int N = p.N, M = p.M, T = p.T, sh = 32 - p.logN;
    const int tiles = (T + 1) / 2;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int tA = 2 * tile, tB = tA + 1;
    const ClipLen cl = clip_len(p.lengths, b, p.L, p.hop);
    const int Lc = cl.Lc, Tc = cl.Tc;
    if (!cl.ok || tA >= Tc) return;
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
    for (int k = tid; k <= (N >> 1); k += kXgThreads) {
        const unsigned ak = N > 1 ? __brev((unsigned)k) >> sh : 0u, an = N > 1 ? __brev((unsigned)((N - k) & (N - 1))) >> sh : 0u;
        const float2 zk = Z[ak], zn = Z[an];
        // X_a = (Z_k + conj Z_{N-k}) / 2,  X_b = (Z_k - conj Z_{N-k}) / (2i)
        const float xar = 0.5f * (zk.x + zn.x), xai = 0.5f * (zk.y - zn.y);
        const float xbr = 0.5f * (zk.y + zn.y), xbi = -0.5f * (zk.x - zn.x);
        float gpa = 0.f, gpb = 0.f;
        const int2 band = p.rowband[k];
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
        Z[ak] = make_float2(har - hbi, -(hai + hbr));                       // conj(H_a + i H_b) at k ...
        if (!edge) Z[an] = make_float2(har + hbi, hai - hbr);               // ... and at N - k (Hermitian extension)
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

// grid (chunks, B): dmel_xgrad_gather_kernel over the clip's Tc frames: the mean from their sums (the same strided partials and tree) over
// Lc, the overlap-add clamped to frame Tc - 1
__global__ void __launch_bounds__(256) dmel_xgrad_gather_len_kernel(XgradLenParams p)
{
    __shared__ double red[256];
    if (xgrad_not_this_nfft(p)) return;
    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int N = p.N, T = p.T, hop = p.hop, half = N / 2;
    const ClipLen cl = clip_len(p.lengths, b, p.L, hop);
    const int Lc = cl.Lc, Tc = min(cl.Tc, T);
    float* gx = p.grad_x + (size_t)b * p.L;
    const int lo = chunk * kXgChunk, hi = min(lo + kXgChunk, p.L);
    if (!cl.ok) {
        for (int i = lo + tid; i < hi; i += 256) gx[i] = __builtin_nanf("");
        return;
    }
    float mean = 0.f;
    if (p.remove_dc) {
        double acc = 0.0;
        for (int t = tid; t < Tc; t += 256) acc += p.csum[(size_t)b * T + t];
        red[tid] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        mean = (float)(red[0] / (double)Lc);
    }
    const float* fr = p.frames + (size_t)b * T * N;
    for (int i = lo + tid; i < hi; i += 256) {
        float v = 0.f;
        if (i < Lc) {
            // frames with 0 <= i - t hop + N/2 < N, in increasing t
            int t_lo = i + half - N + 1;
            t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
            int t_hi = (i + half) / hop;
            if (t_hi > Tc - 1) t_hi = Tc - 1;
            float s = 0.f;
            for (int t = t_lo; t <= t_hi; ++t) s += fr[(size_t)t * N + (i - t * hop + half)];
            v = s - mean;
        }
        gx[i] = v;
    }
}

hipError_t xgrad_len_prepare_attributes()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_frames_len_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kMaxNfft * (int)sizeof(float2));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_frames_len_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 12);
    for (int n = 32; n <= 2048 && e == hipSuccess; n *= 2)
        xgrad_with_plan(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(dmel_xgrad_wave_len_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, XgPlan<N>::LDS_MAX);
        });
    return e;
}

hipError_t launch_xgrad_len(const XgradLenParams& p, hipStream_t s)
{
    if (!p.lengths || p.spec_mode) return hipErrorInvalidValue;
    const dim3 g2((unsigned)((p.L + kXgChunk - 1) / kXgChunk), (unsigned)p.B);
    if (p.tiles > 0) {
        // wave-FFT path: (B x tiles) workgroups, then the combine pass
        const long long grid = (long long)p.B * p.tiles;
        if (grid > 0x7fffffffLL || p.fpt < 1) return hipErrorInvalidValue;
        hipError_t e = hipErrorInvalidValue;
        xgrad_with_plan(p.N, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            if (p.fpt != XgPlan<N>::FPT) return;
            XgradLenParams q = p;
            q.tw2_off = (int)xgrad_wave_tw2_off<N>(p.M, p.win_n);
            hipLaunchKernelGGL(dmel_xgrad_wave_len_kernel<N>, dim3((unsigned)grid), dim3(XgPlan<N>::THREADS), xgrad_wave_lds<N>(p.M, p.win_n), s, q);
            e = hipGetLastError();
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(dmel_xgrad_combine_len_kernel, g2, dim3(256), 0, s, p);
        return hipGetLastError();
    }
    const long long grid = (long long)p.B * ((p.T + 1) / 2);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    XgradLenParams q = p;
    q.tw_in_lds = p.N <= 8192 ? 1 : 0;
    size_t lds = (size_t)p.N * sizeof(float2) + (q.tw_in_lds ? (size_t)(p.N / 2) * sizeof(float2) : 0);
    if (lds < 2 * kXgThreads * sizeof(double)) lds = 2 * kXgThreads * sizeof(double);      // the per-frame sums are reduced where the sequence was
    if (q.tw_in_lds) hipLaunchKernelGGL(dmel_xgrad_frames_len_kernel<true>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    else hipLaunchKernelGGL(dmel_xgrad_frames_len_kernel<false>, dim3((unsigned)grid), dim3(kXgThreads), lds, s, q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dmel_xgrad_gather_len_kernel, g2, dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace dmel
