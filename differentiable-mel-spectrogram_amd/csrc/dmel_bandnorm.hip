// dmel_bandnorm.hip -- BandNorm: length-aware per-band standardisation as a stage of its own behind the mel layers:
//   y = (s - mu) rstd gamma[band] + beta[band]  on the valid frames t < Tc of a row,  +0.0 on its pad frames,  rstd = 1 / sqrt(var + eps)
// over rows of T frames (one row = one (clip[, channel], band) triple; band = row % n_mels, clip = row / rows_per_clip, Tc = lengths[clip]).
// mu and var (biased) are those of the row's own valid frames (clip statistics: utterance-level CMVN) or of every valid frame of every row of
// the band (batch statistics: batch normalisation over the mel bins, with running buffers).
//
// Three roles, forward and backward alike:
//   row statistics   one pass over the valid frames of each row, frames one per lane (loads along T stay contiguous), sums in fp64, the lanes
//                    of a row combined by a fixed butterfly in registers.  Rows of up to 32 frames share a wave as dmel_pcen.hip packs them
//                    (64 / W rows of W = the next power of two >= T lanes each); longer rows get a wave each and walk chunks of 64 frames,
//                    and only the chunks that hold valid frames: a pad chunk is skipped, not masked.  The forward's mean is taken first and
//                    the squared deviations from it second (the first chunk stays in its register, later chunks come back from the cache).
//   band combine     one wave per band: lane l takes rows band + (l + 64 i) n_mels, i ascending, the 64 lane sums go through a fixed
//                    butterfly (the order of dmel_pcen_reduce_kernel).  Row means and squared deviations are merged by the pairwise update
//                    (Chan et al.): no difference of two large sums.  The forward's combine also updates the running buffers.
//   apply            y (or ds) on the valid frames in fp64 from the fp32 input and the fp64 (mu, rstd) pair, rounded once; +0.0 is stored
//                    on pad frames and NaN on every frame of a clip whose length is outside 1 ... T, without a load.
// s and g are never loaded at a pad frame.  lengths[clip] is a scalar load where a wave holds one row.  No atomics, every order is fixed:
// the same inputs give the same bits.  Offsets are 64-bit.
//
// Backward, with yh = (s - mu) rstd:  ds = gamma rstd (g - mean(g) - yh mean(g yh)), the means over the statistic's own population (eval mode
// of the batch statistics: ds = gamma rstd g);  dweight[band] = sum g yh,  dbias[band] = sum g over the valid frames of the band's rows.
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

struct BnRow {
    long long row, off;     // off = row * T
    int j;                  // lane inside the segment
    int band;
    int n;                  // valid frames of the row; 0 for a row past the end or of a clip with an invalid length
    bool rowok, bad;        // bad: the clip's length is outside 1 ... T
};

__device__ __forceinline__ int bn_valid(const BandNormParams& p, long long clip, bool& bad)
{
    return stage_valid(stage_length(p.lengths, clip, p.T), p.T, bad);
}

// W lanes per row (a power of two <= 64; 64: one row per wave), 4 waves per workgroup; 64-bit rows: a launch may hold more than 2^31 of them
__device__ __forceinline__ BnRow bn_row(const BandNormParams& p)
{
    BnRow q;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    q.j = lane & (p.W - 1);
    if (p.logw == 6) {                                             // the row is the wave's: its length comes through a scalar load
        q.row = wave;
        q.rowok = q.row < p.rows;
        const long long clip = (q.rowok ? q.row : 0) / p.rows_per_clip;      // (a 64-bit quotient is formed in vector registers)
        const unsigned lo = __builtin_amdgcn_readfirstlane((int)(clip & 0xFFFFFFFFLL)), hi = __builtin_amdgcn_readfirstlane((int)(clip >> 32));
        const int tc = p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[(long long)(((unsigned long long)hi << 32) | lo)] : p.T;
        q.n = stage_valid(tc, p.T, q.bad);
    } else {
        q.row = wave * (64 >> p.logw) + (lane >> p.logw);
        q.rowok = q.row < p.rows;
        const long long rs = q.rowok ? q.row : 0;
        q.n = bn_valid(p, rs / p.rows_per_clip, q.bad);
    }
    q.band = q.rowok ? (int)(q.row % p.n_mels) : 0;
    q.off = q.row * (long long)p.T;
    if (!q.rowok) { q.n = 0; q.bad = false; }                      // rows past the end load nothing and store nothing
    return q;
}

__device__ __forceinline__ double bn_wave_sum(double v)
{
    return stage_seg_sum(v, 64);
}

__device__ __forceinline__ double2 bn_pair(const double* base, long long i)
{
    return *reinterpret_cast<const double2*>(base + 2 * i);
}

// forward, role 1.  Clip statistics: stats[row] = (mu, rstd).  Batch statistics: partials[row] = (mean, sum of squared deviations from it).
__global__ void __launch_bounds__(256) dmel_bandnorm_rowstat_kernel(BandNormParams p)
{
    const BnRow q = bn_row(p);
    const int W = p.W;
    double sum = 0.0;
    float x0 = 0.f;
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        const float x = (t < q.n) ? p.s[q.off + t] : 0.f;
        if (t0 == 0) x0 = x;
        sum += (double)x;
    }
    const double mean = stage_seg_sum(sum, W) / (double)(q.n > 0 ? q.n : 1);
    double m2 = 0.0;
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        const float x = (t0 == 0) ? x0 : ((t < q.n) ? p.s[q.off + t] : 0.f);
        const double d = (t < q.n) ? (double)x - mean : 0.0;
        m2 = __builtin_fma(d, d, m2);
    }
    m2 = stage_seg_sum(m2, W);
    if (q.rowok && q.j == 0) {
        double2 out;
        if (p.batch_stats) out = make_double2(mean, m2);          // (0, 0) for a clip with an invalid length: it contributes nothing
        else out = make_double2(mean, 1.0 / sqrt(m2 / (double)(q.n > 0 ? q.n : 1) + p.eps));
        *reinterpret_cast<double2*>((p.batch_stats ? p.partials : p.stats) + 2 * q.row) = out;
    }
}

// forward, role 2 (batch statistics): stats[band] = (mu, rstd) of the band; training also moves the running buffers by nn.BatchNorm2d's
// rule (the unbiased variance; left alone below two valid frames, both left alone without any) and counts the batch
__global__ void __launch_bounds__(256) dmel_bandnorm_combine_kernel(BandNormParams p)
{
    const int lane = threadIdx.x & 63;
    const int band = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (band >= p.n_mels) return;                                  // whole waves: no shuffle is left without its partner
    if (p.eval) {
        if (lane == 0)
            *reinterpret_cast<double2*>(p.stats + 2 * (long long)band) =
                make_double2((double)p.running_mean[band], 1.0 / sqrt((double)p.running_var[band] + p.eps));
        return;
    }
    const long long first = band + (long long)lane * p.n_mels, step = 64LL * p.n_mels;
    double cnt = 0.0, sm = 0.0;
    for (long long row = first; row < p.rows; row += step) {
        bool bad;
        const double n = (double)bn_valid(p, row / p.rows_per_clip, bad);
        cnt += n;
        sm = __builtin_fma(n, bn_pair(p.partials, row).x, sm);
    }
    cnt = bn_wave_sum(cnt);
    const double mu = bn_wave_sum(sm) / cnt;                       // no valid frame at all: NaN, and every row of the band is NaN anyway
    double m2 = 0.0;
    for (long long row = first; row < p.rows; row += step) {
        bool bad;
        const int n = bn_valid(p, row / p.rows_per_clip, bad);
        const double2 v = bn_pair(p.partials, row);
        const double d = v.x - mu;
        m2 += (n > 0) ? __builtin_fma((double)n * d, d, v.y) : 0.0;
    }
    m2 = bn_wave_sum(m2);
    if (lane == 0) {
        *reinterpret_cast<double2*>(p.stats + 2 * (long long)band) = make_double2(mu, 1.0 / sqrt(m2 / cnt + p.eps));
        if (p.running_mean && cnt >= 1.0) p.running_mean[band] = (float)((1.0 - p.momentum) * (double)p.running_mean[band] + p.momentum * mu);
        if (p.running_var && cnt >= 2.0) p.running_var[band] = (float)((1.0 - p.momentum) * (double)p.running_var[band] + p.momentum * (m2 / (cnt - 1.0)));
        if (p.num_batches_tracked && band == 0) *p.num_batches_tracked += 1;
    }
}

struct BnAffine { double mu, rstd, gamma, beta; };

__device__ __forceinline__ BnAffine bn_affine(const BandNormParams& p, const BnRow& q)
{
    BnAffine a;
    const double2 st = q.rowok ? bn_pair(p.stats, p.batch_stats ? (long long)q.band : q.row) : make_double2(0.0, 0.0);
    a.mu = st.x;
    a.rstd = st.y;
    a.gamma = p.gamma ? (double)p.gamma[q.band] : 1.0;
    a.beta = p.beta ? (double)p.beta[q.band] : 0.0;
    return a;
}

// the frames from the first chunk without a valid frame on: +0.0, or NaN for a clip with an invalid length; nothing is loaded
__device__ __forceinline__ void bn_fill(const BandNormParams& p, const BnRow& q, float* out)
{
    const float fill = q.bad ? __builtin_nanf("") : 0.f;
    if (!q.rowok) return;
    for (int t0 = (q.n + 63) & ~63; t0 < p.T; t0 += 64) {
        const int t = t0 + q.j;
        if (t < p.T) out[q.off + t] = fill;
    }
}

// forward, role 3
__global__ void __launch_bounds__(256) dmel_bandnorm_apply_kernel(BandNormParams p)
{
    const BnRow q = bn_row(p);
    const BnAffine a = bn_affine(p, q);
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        float y = 0.f;
        if (t < q.n) y = (float)__builtin_fma(((double)p.s[q.off + t] - a.mu) * a.rstd, a.gamma, a.beta);
        if (t < p.T) p.y[q.off + t] = y;
    }
    bn_fill(p, q, p.y);
}

// backward, role 1: partials[row] = (sum g, sum g yh) over the row's valid frames
__global__ void __launch_bounds__(256) dmel_bandnorm_bwd_rowstat_kernel(BandNormParams p)
{
    const BnRow q = bn_row(p);
    const BnAffine a = bn_affine(p, q);
    double sg = 0.0, sgy = 0.0;
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        if (t < q.n) {
            const double g = (double)p.g[q.off + t];
            const double yh = ((double)p.s[q.off + t] - a.mu) * a.rstd;
            sg += g;
            sgy = __builtin_fma(g, yh, sgy);
        }
    }
    sg = stage_seg_sum(sg, p.W);
    sgy = stage_seg_sum(sgy, p.W);
    if (q.rowok && q.j == 0) *reinterpret_cast<double2*>(p.partials + 2 * q.row) = make_double2(sg, sgy);
}

// backward, role 2: dbias[band] = sum g, dweight[band] = sum g yh; training with batch statistics also band_means[band] = both over the
// band's valid frames
__global__ void __launch_bounds__(256) dmel_bandnorm_bwd_combine_kernel(BandNormParams p)
{
    const int lane = threadIdx.x & 63;
    const int band = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (band >= p.n_mels) return;
    double cnt = 0.0, sg = 0.0, sgy = 0.0;
    for (long long row = band + (long long)lane * p.n_mels; row < p.rows; row += 64LL * p.n_mels) {
        bool bad;
        cnt += (double)bn_valid(p, row / p.rows_per_clip, bad);
        const double2 v = bn_pair(p.partials, row);
        sg += v.x;
        sgy += v.y;
    }
    cnt = bn_wave_sum(cnt);
    sg = bn_wave_sum(sg);
    sgy = bn_wave_sum(sgy);
    if (lane == 0) {
        if (p.dbias) p.dbias[band] = (float)sg;
        if (p.dweight) p.dweight[band] = (float)sgy;
        if (p.band_means) *reinterpret_cast<double2*>(p.band_means + 2 * (long long)band) = make_double2(sg / cnt, sgy / cnt);
    }
}

// backward, role 3
__global__ void __launch_bounds__(256) dmel_bandnorm_bwd_apply_kernel(BandNormParams p)
{
    const BnRow q = bn_row(p);
    const BnAffine a = bn_affine(p, q);
    const double scale = a.gamma * a.rstd;
    double mg = 0.0, mgy = 0.0;
    if (!p.eval && q.rowok) {
        if (p.batch_stats) {
            const double2 v = bn_pair(p.band_means, q.band);
            mg = v.x;
            mgy = v.y;
        } else if (q.n > 0) {
            const double2 v = bn_pair(p.partials, q.row);
            mg = v.x / (double)q.n;
            mgy = v.y / (double)q.n;
        }
    }
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        float d = 0.f;
        if (t < q.n) {
            const double g = (double)p.g[q.off + t];
            if (p.eval) d = (float)(scale * g);
            else {
                const double yh = ((double)p.s[q.off + t] - a.mu) * a.rstd;
                d = (float)(scale * (g - mg - yh * mgy));
            }
        }
        if (t < p.T) p.ds[q.off + t] = d;
    }
    bn_fill(p, q, p.ds);
}

static void bandnorm_geometry(BandNormParams& p)
{
    p.logw = stage_logw(p.T);
    p.W = 1 << p.logw;
}

#define BN_LAUNCH(kernel, grid)                                                        \
    do {                                                                               \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(256), 0, s, p);        \
        const hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) return e_;                                               \
    } while (0)

// clip statistics: row statistics, apply.  Batch statistics: row statistics and combine (eval: the combine alone reads the buffers), apply.
hipError_t launch_bandnorm_fwd(BandNormParams p, hipStream_t s)
{
    bandnorm_geometry(p);
    const long long rows_grid = stage_row_blocks(p.rows, p.T), band_grid = (p.n_mels + 3) / 4;
    if (!(p.batch_stats && p.eval)) BN_LAUNCH(dmel_bandnorm_rowstat_kernel, rows_grid);
    if (p.batch_stats) BN_LAUNCH(dmel_bandnorm_combine_kernel, band_grid);
    BN_LAUNCH(dmel_bandnorm_apply_kernel, rows_grid);
    return hipSuccess;
}

// the row sums when anything needs them (the means of ds, the parameter gradients), the combine for the parameter gradients and the band's
// means, the apply when ds is asked for
hipError_t launch_bandnorm_bwd(BandNormParams p, hipStream_t s)
{
    bandnorm_geometry(p);
    const long long rows_grid = stage_row_blocks(p.rows, p.T), band_grid = (p.n_mels + 3) / 4;
    const bool want_p = p.dweight || p.dbias;
    const bool band_mean = p.batch_stats && !p.eval && p.ds;
    const bool row_mean = !p.batch_stats && p.ds;
    if (!band_mean) p.band_means = nullptr;
    if (want_p || band_mean || row_mean) BN_LAUNCH(dmel_bandnorm_bwd_rowstat_kernel, rows_grid);
    if (want_p || band_mean) BN_LAUNCH(dmel_bandnorm_bwd_combine_kernel, band_grid);
    if (p.ds) BN_LAUNCH(dmel_bandnorm_bwd_apply_kernel, rows_grid);
    return hipSuccess;
}

}  // namespace dmel
