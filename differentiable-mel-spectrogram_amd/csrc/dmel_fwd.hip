// dmel_fwd.hip -- fused forward of the DMEL layer for gfx950 (MI355X).
//
// One workgroup (4 or 8 waves) produces a tile of consecutive STFT frames of one clip, from waveform
// samples to log-mel values, without touching HBM in between:
//
//   phase 0: the window table (w, dw/dlambd) is built in LDS and, for clips up to 32768 samples, the clip
//            is summed for the DC removal (longer clips: partial sums from dmel_prep_kernel).
//   phase 1 (VALU + LDS, per wave): DC-removed, Gaussian-windowed frame -> complex FFT.  A wave
//            holds R points per lane and transforms 64/G frames at a time: radix-R butterflies in
//            registers, one transposition through LDS, radix-R again, and a radix-C stage across
//            adjacent lanes with DPP quad permutes (tools/wavefft_sim.py is the index model).
//            Two real sequences ride in one complex FFT: (x~ w, x~ dw/dlambd) when the tangent is
//            wanted (training), two neighbouring frames otherwise.  The pairing pass separates them
//            once per bin and leaves PD[k] = (|X|^2, d|X|^2/dlambd) (or the two frames' |X|^2) in LDS.
//            n_fft 2048 and 4096 use the compact layout (FftPlan::BPERM / SPLIT): the transposition moves one
//            plane of floats at a time and the pairing pass gets Z[N-k] from the lane that holds it
//            (ds_bpermute_b32), so a frame in flight needs N*4 bytes of LDS instead of N*8.
//   phase 2 (MFMA): the mel contraction of models.py:53.  A operands are plain reads of PD,
//            B fragments are the non-zero 4x16 blocks of the filterbank (prefetched into registers
//            before phase 1), v_mfma_f32_16x16x4_f32 accumulates exact fp32.  With 4 waves each wave
//            owns two mel tiles; with 8 waves each owns one tile and the k-steps of the wide tiles are dealt
//            over the waves with narrow (or no) tiles: their sums reach the owner through LDS.
//   epilogue: scale, log(mel + eps) (models.py:73), tangent d out / d lambd, straight from the
//            accumulators into the (B,1,M,T) layout of models.py:36.
//
// Reference semantics restated here: models.py:33-56 (layer forward), time_frequency.py:21-30
// (window), :32-58 (STFT, |.|^2), models.py:73 (log).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#if DMEL_FWD_PART == 0
// ---- prep kernel: per-clip partial sums (DC removal, models.py:38) + window tables -----------
__global__ void __launch_bounds__(kThreads) dmel_prep_kernel(PrepParams p)
{
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    if (blockIdx.y == (unsigned)p.B) {
        // window block: time_frequency.py:21-30 in fp32; second entry = w d^2 2^(-2e), the tangent window up to the
        // factor lam_tangent_scale() that the forward kernels apply in their epilogue (fp64 here: d^2 needs 30 bits)
        if (blockIdx.x != 0) return;
        LamState ls = lam_prologue(p.lam, p.N, false);
        if (ls.action != kLamRun) return;
        if (p.N >= kMinFastNfft && p.N <= kMaxFastNfft && (p.N & (p.N - 1)) == 0 && !p.normalize) ls = lam_clip_scale(ls, p.L);      // the fused kernel's table (n_fft 8192 / 16384): as its epilogue
        const float denom = ls.denom;
        const double s2 = (double)ls.s2;
        double s_ww = 0.0, s_wd = 0.0;
        for (int n = tid; n < p.N; n += kThreads) {
            const float d = (float)n - p.center;
            const float t = d / denom;
            float w = expf(-0.5f * (t * t));
            if (p.win_half && (n < p.N / 4 || n >= 3 * p.N / 4)) w = 0.f;
            const double dw = (double)w * (double)d * (double)d * s2;
            p.win2[n] = make_float2(w, (float)dw);
            s_ww += (double)w * (double)w;
            s_wd += (double)w * dw;
        }
        if (!p.normalize) return;
        // time_frequency.py:25: w / sqrt(sum w^2); derivative of the quotient
        red[tid] = s_ww; __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        const double ww = red[0]; __syncthreads();
        red[tid] = s_wd; __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        const double wd = red[0];
        const double nrm = sqrt(ww);
        for (int n = tid; n < p.N; n += kThreads) {
            const double w = (double)p.win2[n].x;
            const float d = (float)n - p.center;
            const double dwe = w * (double)d * (double)d * s2;       // recomputed in fp64 (the table holds it rounded)
            p.win2[n] = make_float2((float)(w / nrm), (float)(dwe / nrm - w * wd / (nrm * nrm * nrm)));
        }
        return;
    }
    const int b = blockIdx.y, c = blockIdx.x;
    const long long lo = (long long)c * p.chunk;
    long long hi = lo + p.chunk; if (hi > p.L) hi = p.L;
    if (p.lengths) {
        // per-clip lengths: the sums stop at the clip's end (a chunk past it adds up nothing)
        const int lb = p.lengths[b];
        const long long end = (lb >= 1 && lb <= p.L) ? lb : 1;
        if (hi > end) hi = end;
        if (hi < lo) hi = lo;
    }
    const float* xbase = p.x;
    if (p.x_ind) { typedef const float* cfp; xbase = *(const __attribute__((address_space(4))) cfp*)p.x_ind; }      // the batch by address
    const float* xb = xbase + (size_t)b * p.L;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    long long i = lo + tid;
    if (((reinterpret_cast<uintptr_t>(xb + lo)) & 15) == 0) {
        // 16-byte aligned chunk: dwordx4 loads, four per thread in flight before anything is added (round 4: a plain loop waited
        // for every load before it issued the next -- the kernel took 6.9 us for 5 MB at the reference's ESC-50 shape, a third of that
        // step; the sums' order is fixed either way)
        const float4* x4 = reinterpret_cast<const float4*>(xb + lo);
        const long long n4 = (hi - lo) / 4;
        for (long long base = 0; base < n4; base += 4 * kThreads) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const long long q = base + tid + (long long)u * kThreads; v[u] = x4[q < n4 ? q : n4 - 1]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = base + tid + (long long)u * kThreads < n4;
                acc0 += ok ? v[u].x : 0.f; acc1 += ok ? v[u].y : 0.f; acc2 += ok ? v[u].z : 0.f; acc3 += ok ? v[u].w : 0.f;
            }
        }
        i = lo + n4 * 4 + tid;
    } else {
        for (; i + 3 * kThreads < hi; i += 4 * kThreads) {
            acc0 += xb[i]; acc1 += xb[i + kThreads]; acc2 += xb[i + 2 * kThreads]; acc3 += xb[i + 3 * kThreads];
        }
    }
    for (; i < hi; i += kThreads) acc0 += xb[i];
    // fixed order: the four accumulators of a thread, the 64 lanes of a wave (DPP butterfly in fp64, the same value in every lane), the four
    // waves ascending -- one barrier instead of the eight of a 256-entry tree in LDS
    double s = ((double)acc0 + (double)acc1) + ((double)acc2 + (double)acc3);
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) p.psum[(size_t)b * p.nchunks + c] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

hipError_t launch_prep(const PrepParams& p, hipStream_t s)
{
    dim3 grid(p.nchunks, p.B + 1);
    hipLaunchKernelGGL(dmel_prep_kernel, grid, dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

#endif   // DMEL_FWD_PART == 0

// ---- fused forward --------------------------------------------------------------------------

#include "dmel_fwd_log.h"

#ifdef DMEL_STAMPS
// Diagnostic build only (tools/stamps.py): s_memtime stamps of every wave at the phase boundaries of the
// fused kernel, kept in a buffer nothing else reads.  Never compiled into libdmel_hip.so.
constexpr int kStampSlots = 32;     // 0-2 prologue, 12-13 placement, 3-11 tile 0, 16 + (2..11) tile 1 (2 = tile start)
__device__ unsigned long long g_stamps[4096 * 8 * kStampSlots];
__device__ __forceinline__ void stamp(int wgid, int wave, int lane, int idx)
{
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (lane == 0 && wgid < 4096) g_stamps[((size_t)wgid * 8 + wave) * kStampSlots + idx] = t;
}
#define STAMP(i) stamp(blockIdx.x, wave, lane, i)
// where the workgroup runs: HW_ID (wave / SIMD / CU / SH / SE ids) and XCC_ID, slots 12 and 13
__device__ __forceinline__ void stamp_place(int wgid, int wave, int lane)
{
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (lane == 0 && wgid < 4096) {
        g_stamps[((size_t)wgid * 8 + wave) * kStampSlots + 12] = hw;
        g_stamps[((size_t)wgid * 8 + wave) * kStampSlots + 13] = xcc;
    }
}
#define STAMP_PLACE() stamp_place(blockIdx.x, wave, lane)
#else
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)
#endif

// TPW = tiles one workgroup produces, one after the other.  With TPW = 2 the prologue (lambd, window table, clip sum: a third
// of a tile's lifetime, mostly spent waiting for memory) is paid once for twice the frames, the samples of the second tile
// are requested while the first is transformed, and a launch needs half the workgroups (one round of resident workgroups
// instead of two at BASELINE config 2).
#define DMEL_FWD_MULTI 0
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_MULTI
#define DMEL_FWD_MULTI 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_MULTI

// two tiles per workgroup are built for the sizes whose launches are large enough to use them (forward_tiles_per_wg)
template <int N, bool PAIR> constexpr bool has_tpw2() { return N >= 256 && (N <= 512 || (N == 1024 && geom<N, PAIR>().G == 64)); }   // (32 x 32 plan at 1024: 16-frame tiles, two of them spill)

// kTrainH (dense contraction on the bf16 matrix pipe) exists for the sizes whose frames live inside one wave, one tile per workgroup
template <int N> constexpr bool has_hsplit() { return N >= kHsplitMinNfft && N <= kHsplitMaxNfft; }

// this file's variant (dmel_fwd_dispatch.h): every mode; the contraction variants one tile per workgroup, the others also two where has_tpw2
struct FwdVariant {
    using Params = FwdParams;
    using Modes = FwdModes<kTrain, kInfer, kSpec, kSpecTrain, kTrainH, kTrainW, kTrainWW>;
    template <int N, int MODE, int TPW> static constexpr bool exists()
    {
        if (MODE == kTrainH) return TPW == 1 && has_hsplit<N>();
        if (MODE == kTrainW) return TPW == 1 && wlc_size(N);
        if (MODE == kTrainWW) return TPW == 1 && wlc_wide_size(N);
        return TPW == 1 || (TPW == 2 && has_tpw2<N, mode_pairs(MODE)>());
    }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdParams) = {dmel_fwd_kernel<N, MODE, TPW>, dmel_fwd_multi_kernel<N, MODE, TPW>};
    static int pick(const FwdParams& p) { return p.ch_out ? 1 : 0; }
};
DMEL_FWD_PARTS_OF(FwdVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdParams& p, int grid, hipStream_t s) { return fwd_launch<FwdVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_prepare_attributes() { return fwd_set_attr<FwdVariant>(); }

// (forward_has_hsplit, _has_wlc, _wlc_one_frame, _plan_rc, _waves, _nbpre: dmel_tables.cpp, where a program without kernels links them)
bool forward_has_wlc_wide(int n_fft) { return wlc_wide_size(n_fft); }
bool forward_window_in_lds(int n_fft) { return n_fft >= kMinFastNfft && n_fft <= kWinLdsMaxNfft; }

// the geometry of the plan for a run-time (n_fft, pair)
template <class F> static bool with_geom(int n_fft, bool pair, F&& f)
{
    return with_nfft(n_fft, [&](auto nn) { constexpr int N = decltype(nn)::value; f(pair ? geom<N, true>() : geom<N, false>()); });
}

int forward_lds_bytes(int n_fft, int mode)
{
    int v = -1;
    with_geom(n_fft, mode_pairs(mode), [&](const FftGeom& g) { v = g.LDS_BYTES; });
    if (mode == kTrainWW && n_fft == 1024 && wlc_wide_size(1024)) return geom<1024, false, true, true>().LDS_BYTES;
    if (mode == kTrainW) {
        switch (n_fft) {                                   // (the sizes kTrainW may be built for)
            case 512: v = geom<512, false, true>().LDS_BYTES; break;
            case 1024: v = geom<1024, false, true>().LDS_BYTES; break;
            case 2048: v = geom<2048, false, true>().LDS_BYTES; break;
            case 4096: v = geom<4096, false, true>().LDS_BYTES; break;
        }
    }
    return v;
}

int forward_frames_per_tile(int n_fft, int mode)
{
    if (mode == kTrainWW && n_fft == 1024 && wlc_wide_size(1024)) return geom<1024, false, true, true>().SLOTS;
    if (mode == kTrainW && n_fft == 512) return geom<512, false, true>().SLOTS;          // (its plan has its own number of waves)
    int slots = -1;
    with_geom(n_fft, mode_pairs(mode), [&](const FftGeom& g) { slots = g.SLOTS; });
    if (slots < 0) return -1;
    return mode_pairs(mode) ? 2 * slots : slots;
}

bool forward_two_tiles(int n_fft, int mode)
{
    if (mode_wlc(mode) || mode == kTrainH) return false;          // one tile per workgroup (launch_mode)
    bool two = false;
    with_nfft(n_fft, [&](auto nn) { constexpr int N = decltype(nn)::value; two = mode_pairs(mode) ? has_tpw2<N, true>() : has_tpw2<N, false>(); });
    return two;
}

// Tiles per workgroup for a launch over `batch` clips of `tiles_per_clip` tiles.  A launch runs in rounds of the workgroups
// the chip holds at once (160 KB of LDS per CU, 256 CUs); a two-tile workgroup lives about 1.9 times as long as a one-tile
// one (it pays the prologue once: measured 21.97 against 23.1 us at BASELINE config 2 with the 16 x 16 x 4 plan, one round instead of
// two).  Two tiles are used when that model says the launch gets shorter -- e.g. not for 5 rounds becoming 3 double ones.
// Workgroups of the (n_fft, mode) instantiation the device holds at once: LDS-limited (160 KB per CU), at most 32 waves per CU
int forward_resident_workgroups(int n_fft, int mode)
{
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        return n;
    }();
    const int lds = forward_lds_bytes(n_fft, mode), waves = (mode == kTrainW && n_fft == 512) ? geom<512, false, true>().WAVES : forward_waves(n_fft);
    int per_cu = (lds > 0 && 163840 / lds > 0) ? 163840 / lds : 1;
    if (waves > 0 && per_cu * waves > 32) per_cu = 32 / waves;
    return cus * (per_cu > 0 ? per_cu : 1);
}

int forward_tiles_per_wg(int n_fft, int mode, int batch, int tiles_per_clip)
{
    if (!forward_two_tiles(n_fft, mode) || tiles_per_clip < 2 || batch < 1) return 1;
    const long long resident = forward_resident_workgroups(n_fft, mode);
    const long long wg1 = (long long)batch * tiles_per_clip, wg2 = (long long)batch * ((tiles_per_clip + 1) / 2);
    const long long r1 = (wg1 + resident - 1) / resident, r2 = (wg2 + resident - 1) / resident;
    return 19 * r2 < 10 * r1 ? 2 : 1;
}

#endif   // DMEL_FWD_PART == 0

}  // namespace dmel

#ifdef DMEL_STAMPS
extern "C" int dmel_debug_read_stamps(unsigned long long* host, int count)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(dmel::g_stamps), sizeof(unsigned long long) * (size_t)count);
}
#endif
