// dmel_statspool.hip -- StatsPool: length-aware mean / std / max pooling over time behind the mel layers ("statistics pooling").  A row is
// one (clip, channel, band) triple of a contiguous (B, C, M, T) tensor: T frames; clip = row / rows_per_clip, Tc = lengths[clip] (nullptr: T).
//   mean  mu = (sum_{t < Tc} s[t]) / Tc                                    the sum and the quotient in fp64, rounded to fp32 once
//   std   sd = sqrt(m2 / Tc + eps),  m2 = sum_{t < Tc} (s[t] - mu)^2       the mean first, the squared deviations from the unrounded mu second
//   max   s[am] moved as a word; am by the order: a NaN beats a non-NaN, then the larger value, then the lower t (-0.0 and +0.0 tie)
// The output has S = popcount(which) groups of rows_per_clip values per clip, in torch.cat([mean, std, max], dim=1) order: input row r goes
// to element (r / rows_per_clip) S rows_per_clip + o rows_per_clip + r % rows_per_clip of group o (include/dmel.h is the specification).
//
// One forward and one backward kernel on the geometry of dmel_bandnorm.hip's row statistics: frames one per lane (loads along T stay
// contiguous), rows of up to 32 frames packed 64 / W to a wave (W = the next power of two >= T lanes each), longer rows a wave each, lane j
// taking frames j, j + 64, ... of the chunks that hold valid frames: a pad chunk is skipped, not masked, and s is never loaded at a pad
// frame.  The first chunk stays in its register for the second pass, later chunks come back from the cache.  The lanes of a row are combined
// by fixed butterflies in registers -- the sums in fp64, the maximum by an order that is total (ties go to the lower frame), so the tree
// cannot change what wins.  No LDS, no barrier, no atomics: the same inputs give the same bits, and a row's result depends on its own
// valid frames and (T, Tc) only.  lengths[clip] is a scalar load where a wave holds one row.  Lane 0 of the segment stores the row's S
// results, the unrounded (mu, sd) pair and am.  A length outside 1 ... T makes every output element of its clip NaN (am = -1).
//
// Backward, element-wise:  ds[t] = g_mean / Tc + g_std (s[t] - mu) / (Tc sd) + [t == am] g_max  on t < Tc, in fp64 from the stored (mu, sd)
// and am, rounded once; +0.0 on pad frames; s is read only when std is selected, never at a pad frame.
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

struct SpRow {
    long long row, off, out;    // off = row * T; out: the row's element of group 0 of y (or g)
    int j;                      // lane inside the segment
    int n;                      // valid frames of the row; 0 for a row past the end or of a clip with an invalid length
    bool rowok, bad;            // bad: the clip's length is outside 1 ... T
};

// W lanes per row (a power of two <= 64; 64: one row per wave), 4 waves per workgroup
__device__ __forceinline__ SpRow sp_row(const StatsPoolParams& p)
{
    SpRow q;
    const int lane = threadIdx.x & 63;
    // (the launcher keeps rows below 2^31: 32-bit quotients)
    const unsigned wid = stage_wave();
    q.j = lane & (p.W - 1);
    unsigned row, clip;
    int tc;
    if (p.logw == 6) {                                             // the row is the wave's: its length comes through a scalar load
        row = wid;
        q.rowok = row < (unsigned)p.rows;
        clip = (q.rowok ? row : 0u) / (unsigned)p.rows_per_clip;
        tc = p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[clip] : p.T;
    } else {
        row = wid * (unsigned)(64 >> p.logw) + (unsigned)(lane >> p.logw);
        q.rowok = row < (unsigned)p.rows;
        clip = (q.rowok ? row : 0u) / (unsigned)p.rows_per_clip;
        tc = p.lengths ? p.lengths[clip] : p.T;
    }
    q.bad = stage_bad(tc, p.T);
    q.n = q.bad ? 0 : tc;
    q.row = row;
    q.off = (long long)row * p.T;
    q.out = (long long)clip * p.S * p.rows_per_clip + ((long long)row - (long long)clip * p.rows_per_clip);
    if (!q.rowok) { q.n = 0; q.bad = false; }                      // rows past the end load nothing and store nothing
    return q;
}

// a comes strictly before b in the order of the maximum, frames aside: a NaN beats a non-NaN, then the larger value (-0.0 == +0.0)
__device__ __forceinline__ bool sp_beats(unsigned a, unsigned b)
{
    const float fa = __uint_as_float(a), fb = __uint_as_float(b);
    if (fb != fb) return false;
    if (fa != fa) return true;
    return fa > fb;
}

__global__ void __launch_bounds__(256) dmel_statspool_fwd_kernel(StatsPoolParams p)
{
    const SpRow q = sp_row(p);
    const int W = p.W;
    const unsigned* sw = reinterpret_cast<const unsigned*>(p.s) + q.off;
    double sum = 0.0;
    unsigned w0 = 0u;
    unsigned bw = 0u;                                              // the lane's best frame so far: its word and its frame; -1: none yet
    int bt = -1;
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        if (t < q.n) {
            const unsigned w = sw[t];
            if (t0 == 0) w0 = w;
            sum += (double)__uint_as_float(w);
            if (bt < 0 || sp_beats(w, bw)) { bw = w; bt = t; }     // frames ascend: a tie keeps the lower one
        }
    }
    if ((p.which & 4) || p.argmax) {
        for (int d = W >> 1; d >= 1; d >>= 1) {
            const unsigned ow = (unsigned)__shfl_xor((int)bw, d, 64);
            const int ot = __shfl_xor(bt, d, 64);
            if (ot >= 0 && (bt < 0 || sp_beats(ow, bw) || (!sp_beats(bw, ow) && ot < bt))) { bw = ow; bt = ot; }
        }
    }
    const double cnt = (double)(q.n > 0 ? q.n : 1);
    const double mean = stage_seg_sum(sum, W) / cnt;
    double sd = 0.0;
    if ((p.which & 2) || p.stats) {
        double m2 = 0.0;
        for (int t0 = 0; t0 < q.n; t0 += 64) {
            const int t = t0 + q.j;
            if (t < q.n) {
                const double d = (double)__uint_as_float(t0 == 0 ? w0 : sw[t]) - mean;
                m2 = __builtin_fma(d, d, m2);
            }
        }
        sd = sqrt(stage_seg_sum(m2, W) / cnt + p.eps);
    }
    if (q.rowok && q.j == 0) {
        const unsigned nan = 0x7FC00000u;
        unsigned* y = reinterpret_cast<unsigned*>(p.y) + q.out;
        const long long gs = p.rows_per_clip;
        int o = 0;
        if (p.which & 1) y[(o++) * gs] = q.bad ? nan : __float_as_uint((float)mean);
        if (p.which & 2) y[(o++) * gs] = q.bad ? nan : __float_as_uint((float)sd);
        if (p.which & 4) y[o * gs] = q.bad ? nan : bw;
        if (p.stats) {
            const double dn = __builtin_nan("");
            *reinterpret_cast<double2*>(p.stats + 2 * q.row) = q.bad ? make_double2(dn, dn) : make_double2(mean, sd);
        }
        if (p.argmax) p.argmax[q.row] = q.bad ? -1 : bt;
    }
}

__global__ void __launch_bounds__(256) dmel_statspool_bwd_kernel(StatsPoolParams p)
{
    const SpRow q = sp_row(p);
    if (!q.rowok) return;                                          // (no shuffle in this kernel)
    double cm = 0.0, cs = 0.0, mu = 0.0, gx = 0.0;
    int am = -1;
    if (q.n > 0) {
        const float* g = p.g + q.out;
        const long long gs = p.rows_per_clip;
        int o = 0;
        if (p.which & 1) cm = (double)g[(o++) * gs] / (double)q.n;
        if (p.which & 2) {
            const double2 st = *reinterpret_cast<const double2*>(p.stats + 2 * q.row);
            mu = st.x;
            cs = (double)g[(o++) * gs] / ((double)q.n * st.y);
        }
        if (p.which & 4) {
            gx = (double)g[o * gs];
            am = p.argmax[q.row];
        }
    }
    const float fill = q.bad ? __builtin_nanf("") : 0.f;
    for (int t0 = 0; t0 < p.T; t0 += 64) {
        const int t = t0 + q.j;
        if (t < p.T) {
            float d = fill;
            if (t < q.n) {
                double acc = cm;
                if (p.which & 2) acc = __builtin_fma(cs, (double)p.s[q.off + t] - mu, acc);
                if (t == am) acc += gx;
                d = (float)acc;
            }
            p.ds[q.off + t] = d;
        }
    }
}

hipError_t launch_statspool(StatsPoolParams p, bool backward, hipStream_t s)
{
    p.logw = stage_logw(p.T);
    p.W = 1 << p.logw;
    const long long blocks = stage_row_blocks(p.rows, p.T);
    if (backward) hipLaunchKernelGGL(dmel_statspool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(dmel_statspool_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
