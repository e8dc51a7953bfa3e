// dmel_attnpool.hip -- AttentivePool: length-aware attentive statistics pooling over time behind the mel layers (x-vector / ECAPA).  A row
// is one (clip, channel, band) triple of a contiguous (B, C, M, T) tensor; a clip has R = rows_per_clip rows and A logit rows of T frames,
// A divides R, row r of the clip reads logit row r / (R / A).  clip = row / R, Tc = lengths[clip] (nullptr: T).  Over t < Tc only:
//   per logit row   m = max a[t],  p[t] = exp((double)a[t] - (double)m),  Z = sum p[t],  w[t] = p[t] / Z
//   per row         mu = (sum p[t] s[t]) / Z,  var = (sum p[t] (s[t] - mu)^2) / Z  (the mean first, the deviations from the unrounded mu
//                   second),  sd = sqrt(var + eps); sums in fp64, mean and std rounded to fp32 once.  mu is evaluated around the row's
//                   first frame, s[0] + (sum p[t] (s[t] - s[0])) / Z: the same number, and a constant row c has mu == c, var == 0 exactly
// The output has S = popcount(which) groups of R values per clip in torch.cat([mean, std], dim=1) order, StatsPool's group layout
// (include/dmel.h is the specification).
//
// Forward, one launch on the row geometry of dmel_statspool.hip (ap_row is sp_row with the logit-row fields; both are built from dmel_stage.h): frames one per lane, rows
// of up to 32 frames packed 64 / W to a wave (W = the next power of two >= T lanes each), longer rows a wave each, lane j taking frames j,
// j + 64, ... of the chunks that hold valid frames: a pad chunk is skipped, not masked, and neither s nor a is loaded at a pad frame.  Every
// row's lanes recompute m and Z from the row's logit row (T exponentials per row more than a weights pass would need, and one launch less);
// the first chunk's logit, weight and value stay in registers for the later passes, later chunks come back from the cache and their
// exponentials are taken again.  The lanes of a row meet through fixed butterflies in registers, the sums in fp64: no LDS, no barrier, no
// atomics -- the same inputs give the same bits, and a row's result depends on its own valid frames, its logit row and (T, Tc) only.
// lengths[clip] is a scalar load where a wave holds one row.  Lane 0 of the segment stores the row's S results and the unrounded (mu, var)
// pair; the first row of a logit row's group also stores (m, Z).  A length outside 1 ... T makes every output element of its clip NaN.
//
// Backward, one launch, frames across lanes and a loop over rows: an owner is one (clip, logit row, 64-frame chunk) triple, lane l holds
// frame 64 chunk + l and w[t] = exp(a[t] - m) / Z from the stored pair.  The owner's R / A rows are walked with g and the (mu, var) pair
// as uniform loads: with d = s[t] - mu,
//   ds[r, t] = w[t] (g_mean[r] + g_std[r] d / sd[r])                           stored as the walk goes
//   da[t]    = w[t] sum_r (g_mean[r] d + g_std[r] (d^2 - var[r]) / (2 sd[r]))  the bracket accumulated per lane in fp64
// (the softmax Jacobian with its mean term taken in closed form: sum_u w[u] d[u] = 0 and sum_u w[u] d[u]^2 = var, so no reduction over
// frames exists here).  1, 2, 4, 8 or 16 waves of a workgroup share an owner's rows (the largest that R / A fills; workgroups of 4 waves,
// of 8 or 16 where so many share) and meet once in LDS, summed in the waves' order; a wave keeps four rows in flight, their loads issued
// before the first of their stores.  Where every row has a logit row of its own (R / A == 1) nothing is shared: dmel_attnpool_bwd_row_kernel
// is the same arithmetic straight through, a wave per row's chunk.  +0.0 on pad frames, a chunk without a valid frame stores its zeros without loading, NaN for a clip with an invalid length.
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

struct ApRow {
    long long row, off, aoff, lrow, out;  // off = row * T; lrow: the logit row, aoff = lrow * T; out: the row's element of group 0 of y
    int j;                      // lane inside the segment
    int n;                      // valid frames of the row; 0 for a row past the end or of a clip with an invalid length
    bool rowok, bad, first;     // bad: the clip's length is outside 1 ... T; first: the first row of its logit row's group
};

// W lanes per row (a power of two <= 64; 64: one row per wave), 4 waves per workgroup
__device__ __forceinline__ ApRow ap_row(const AttnPoolParams& p)
{
    ApRow q;
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
    const unsigned in_clip = (q.rowok ? row : 0u) - clip * (unsigned)p.rows_per_clip;
    const unsigned arow = in_clip / (unsigned)p.group;
    q.first = in_clip - arow * (unsigned)p.group == 0u;
    q.lrow = (long long)clip * p.logit_rows + arow;
    q.aoff = q.lrow * p.T;
    q.out = (long long)clip * p.S * p.rows_per_clip + in_clip;
    if (!q.rowok) { q.n = 0; q.bad = false; }                      // rows past the end load nothing and store nothing
    return q;
}

__global__ void __launch_bounds__(256) dmel_attnpool_fwd_kernel(AttnPoolParams p)
{
    const ApRow q = ap_row(p);
    const int W = p.W;
    const float* sr = p.s + q.off;
    const float* ar = p.a + q.aoff;
    float a0 = 0.f, s0 = 0.f;
    float mx = -__builtin_inff();
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        if (t < q.n) {
            const float av = ar[t];
            if (t0 == 0) a0 = av;
            mx = fmaxf(mx, av);
        }
    }
    for (int d = W >> 1; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    const double m = (double)mx;
    const double ref = q.n > 0 ? (double)sr[0] : 0.0;              // the row's first frame: the mean is taken around it (see above)
    double z = 0.0, ps = 0.0, p0 = 0.0;
    for (int t0 = 0; t0 < q.n; t0 += 64) {
        const int t = t0 + q.j;
        if (t < q.n) {
            const double pe = exp((double)(t0 == 0 ? a0 : ar[t]) - m);
            const float sv = sr[t];
            if (t0 == 0) { p0 = pe; s0 = sv; }
            z += pe;
            ps = __builtin_fma(pe, (double)sv - ref, ps);
        }
    }
    const double Z = stage_seg_sum(z, W);
    const double mean = ref + stage_seg_sum(ps, W) / Z;
    double var = 0.0;
    if ((p.which & 2) || p.stats) {
        double v = 0.0;
        for (int t0 = 0; t0 < q.n; t0 += 64) {
            const int t = t0 + q.j;
            if (t < q.n) {
                const double pe = t0 == 0 ? p0 : exp((double)ar[t] - m);
                const double d = (double)(t0 == 0 ? s0 : sr[t]) - mean;
                v = __builtin_fma(pe * d, d, v);
            }
        }
        var = stage_seg_sum(v, W) / Z;
    }
    if (q.rowok && q.j == 0) {
        const unsigned nan = 0x7FC00000u;
        unsigned* y = reinterpret_cast<unsigned*>(p.y) + q.out;
        const long long gs = p.rows_per_clip;
        int o = 0;
        if (p.which & 1) y[(o++) * gs] = q.bad ? nan : __float_as_uint((float)mean);
        if (p.which & 2) y[o * gs] = q.bad ? nan : __float_as_uint((float)sqrt(var + p.eps));
        const double dn = __builtin_nan("");
        if (p.stats) *reinterpret_cast<double2*>(p.stats + 2 * q.row) = q.bad ? make_double2(dn, dn) : make_double2(mean, var);
        if (p.norm && q.first) *reinterpret_cast<double2*>(p.norm + 2 * q.lrow) = q.bad ? make_double2(dn, dn) : make_double2(m, Z);
    }
}

__global__ void __launch_bounds__(1024) dmel_attnpool_bwd_kernel(AttnPoolParams p)
{
    __shared__ double part[16][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int split = 1 << p.logsplit;
    const int sub = wave & (split - 1);
    const long long owner = (long long)blockIdx.x * ((int)(blockDim.x >> 6) >> p.logsplit) + (wave >> p.logsplit);
    const bool ok = owner < p.owners;                              // (an owner past the end still meets its workgroup at the barrier)
    const long long ow = ok ? owner : 0;
    const long long lrow = ow / p.chunks;
    const int chunk = (int)(ow - lrow * p.chunks);
    const long long clip = lrow / p.logit_rows;
    const long long arow = lrow - clip * p.logit_rows;
    bool bad;
    const int n = stage_valid(p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[clip] : p.T, p.T, bad);
    const int t = chunk * 64 + lane;
    const bool in_row = t < p.T, valid = t < n;
    const bool any = chunk * 64 < n;                               // the chunk holds a valid frame (uniform)
    double w = 0.0;
    if (valid) {
        const stage_const_doubles nm = (stage_const_doubles)(unsigned long long)p.norm + 2 * lrow;
        w = exp((double)p.a[lrow * p.T + t] - nm[0]) / nm[1];
    }
    const long long r0 = clip * p.rows_per_clip + arow * p.group;
    const stage_const_floats g = (stage_const_floats)(unsigned long long)p.g + (clip * p.S * p.rows_per_clip + arow * p.group);
    const stage_const_doubles st = (stage_const_doubles)(unsigned long long)p.stats + 2 * r0;
    const long long gs = p.rows_per_clip;
    const float fill = bad ? __builtin_nanf("") : 0.f;
    double acc = 0.0;
    constexpr int U = 4;                                           // rows in flight: their loads are issued before the first of their stores
    if (ok) {
        const int group = (int)p.group;                            // (rows_per_clip is below 2^31)
        const float* sp = p.s + r0 * p.T + t;
        float* dsp = p.ds + r0 * p.T + t;
        for (int k0 = sub; k0 < group; k0 += U * split) {
            double mu[U], var[U], gm[U], gsd[U];
            float sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * split;
                mu[u] = var[u] = gm[u] = gsd[u] = 0.0;
                sv[u] = 0.f;
                if (any && k < group) {
                    mu[u] = st[2 * k];
                    var[u] = st[2 * k + 1];
                    int o = 0;
                    if (p.which & 1) gm[u] = (double)g[k + (o++) * gs];
                    if (p.which & 2) gsd[u] = (double)g[k + o * gs];
                    if (valid) sv[u] = sp[(long long)k * p.T];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * split;
                if (k < group) {
                    float out = fill;
                    if (valid) {
                        const double q = (p.which & 2) ? gsd[u] / sqrt(var[u] + p.eps) : 0.0;
                        const double d = (double)sv[u] - mu[u];
                        out = (float)(w * __builtin_fma(q, d, gm[u]));
                        acc += __builtin_fma(gm[u], d, 0.5 * q * __builtin_fma(d, d, -var[u]));
                    }
                    if (in_row) dsp[(long long)k * p.T] = out;
                }
            }
        }
    }
    if (split > 1) {                                               // the waves that shared the rows meet once, summed in their order
        part[wave][lane] = acc;
        __syncthreads();
        if (sub == 0)
            for (int i = 1; i < split; ++i) acc += part[wave + i][lane];
    }
    if (ok && sub == 0 && in_row) p.da[lrow * p.T + t] = valid ? (float)(w * acc) : fill;
}

// the backward where every row has a logit row of its own (R / A == 1): an owner is one row's chunk, nothing is shared and nothing meets
__global__ void __launch_bounds__(256) dmel_attnpool_bwd_row_kernel(AttnPoolParams p)
{
    const int lane = threadIdx.x & 63;
    const long long owner = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (owner >= p.owners) return;                                 // (no barrier in this kernel)
    const long long row = owner / p.chunks;                        // the row and its logit row
    const int chunk = (int)(owner - row * p.chunks);
    const long long clip = row / p.rows_per_clip;
    const int tc = p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[clip] : p.T;
    const bool bad = stage_bad(tc, p.T);
    const int t = chunk * 64 + lane;
    const float fill = bad ? __builtin_nanf("") : 0.f;
    float dsv = fill, dav = fill;
    if (!bad && t < tc) {
        const stage_const_doubles nm = (stage_const_doubles)(unsigned long long)p.norm + 2 * row;
        const stage_const_doubles st = (stage_const_doubles)(unsigned long long)p.stats + 2 * row;
        const stage_const_floats g = (stage_const_floats)(unsigned long long)p.g + (clip * p.S * p.rows_per_clip + (row - clip * p.rows_per_clip));
        const double mu = st[0], var = st[1];
        double gm = 0.0, q = 0.0;
        int o = 0;
        if (p.which & 1) gm = (double)g[(o++) * p.rows_per_clip];
        if (p.which & 2) q = (double)g[o * p.rows_per_clip] / sqrt(var + p.eps);
        const double w = exp((double)p.a[row * p.T + t] - nm[0]) / nm[1];
        const double d = (double)p.s[row * p.T + t] - mu;
        dsv = (float)(w * __builtin_fma(q, d, gm));
        dav = (float)(w * __builtin_fma(gm, d, 0.5 * q * __builtin_fma(d, d, -var)));
    }
    if (t < p.T) {
        p.ds[row * p.T + t] = dsv;
        p.da[row * p.T + t] = dav;
    }
}

static void attnpool_geometry(AttnPoolParams& p)
{
    p.logw = stage_logw(p.T);
    p.W = 1 << p.logw;
    p.group = p.logit_rows > 0 ? p.rows_per_clip / p.logit_rows : 1;
    p.chunks = (p.T + 63) / 64;
    p.logsplit = p.group >= 16 ? 4 : p.group >= 8 ? 3 : p.group >= 4 ? 2 : p.group >= 2 ? 1 : 0;
    p.owners = p.rows_per_clip > 0 ? p.rows / p.rows_per_clip * p.logit_rows * p.chunks : 0;
}

long long attnpool_blocks(long long rows, long long rows_per_clip, long long logit_rows, int T, bool backward)
{
    AttnPoolParams p{};
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.logit_rows = logit_rows; p.T = T;
    attnpool_geometry(p);
    const long long per_block = backward ? ((p.logsplit > 2 ? 1 << p.logsplit : 4) >> p.logsplit) : 4LL * (64 >> p.logw);
    return ((backward ? p.owners : rows) + per_block - 1) / per_block;
}

hipError_t launch_attnpool(AttnPoolParams p, bool backward, hipStream_t s)
{
    attnpool_geometry(p);
    const long long blocks = attnpool_blocks(p.rows, p.rows_per_clip, p.logit_rows, p.T, backward);
    if (backward && p.group == 1) hipLaunchKernelGGL(dmel_attnpool_bwd_row_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    else if (backward) hipLaunchKernelGGL(dmel_attnpool_bwd_kernel, dim3((unsigned)blocks), dim3(p.logsplit > 2 ? 64u << p.logsplit : 256u), 0, s, p);
    else hipLaunchKernelGGL(dmel_attnpool_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
