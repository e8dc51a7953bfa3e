// dmel_deltas.hip -- Deltas: length-aware delta ("velocity") and delta-delta ("acceleration") channels behind the mel layers.  A row is one
// (clip, channel, band) triple of a contiguous (B, C, M, T) tensor: T frames; clip = row / rows_per_clip, Tc = lengths[clip] (nullptr: T).
//   d[t]  = ( sum_{j = 1 .. n} j (x[min(t + j, Tc - 1)] - x[max(t - j, 0)]) ) / denom   for t < Tc,   +0.0 for t >= Tc
//   dd[t] = the same stencil on the STORED fp32 row d[0 .. Tc - 1]
// The output has G = include_static + order groups of rows_per_clip rows per clip, in torch.cat([s, d, dd], dim=1) order: input row r goes to
// output row (r / rows_per_clip) G rows_per_clip + o rows_per_clip + r % rows_per_clip of group o.  The static group is s moved as words on
// every frame.  The edge of the stencil is the CLIP's last frame, not the batch's (include/dmel.h is the specification).
//
// One forward and one backward kernel, the same geometry: frames one per lane (loads and stores along T are contiguous and element-wide).
//   T <= 32   rows of W = the next power of two >= T lanes, 64 / W rows packed into a wave (as dmel_pcen.hip and dmel_bandnorm.hip pack them)
//   T <= 64   a wave per row
//   T >  64   a wave per chunk of step = 64 - 4 n output frames with a halo of 2 n frames on either side: lane l holds frame
//             chunk * step - 2 n + l, lanes 2 n ... 63 - 2 n store
// In all three the lane's neighbours come through __shfl: no LDS allocation, no barrier.  The source lane of a tap is that of the CLAMPED
// FRAME, base + clamp(clamp(f) +- j, 0, Tc - 1) - f0, never a clamped lane: a halo lane whose frame f lies outside 0 ... Tc - 1 evaluates the
// stencil at clamp(f), so it holds d[clamp(f)] (and no tap ever reads such a lane: every tap frame lies inside 0 ... Tc - 1).  Every frame's
// value is the same arithmetic wherever its lane sits, so dd is the kernel applied to its own stored d bit for bit.
// The differences and the sum over j are taken in fp64 (both exact for fp32 data of like magnitude: a constant row, Tc = 1 and a row of
// silent frames give +0.0), scaled by 1 / denom and rounded to fp32 once.
// A chunk without a valid frame stores its zeros (and moves the static group) without loading s or g; s, g_d and g_dd are never loaded at
// a pad frame.  A length outside 1 ... T makes every output row of its clip NaN.  lengths[clip] is a scalar load where a wave holds one row.
//
// Backward: ds = g_static + D^T (g_d + D^T g_dd), D the Tc x Tc matrix of the clamped stencil.  Lane u GATHERS its own ds[u] (no atomics):
//   (D^T v)[u] = ( sum_{k = 0 .. n} a_k(u) v[u - k] - b_k(u) v[u + k] ) / denom   over the taps inside 0 ... Tc - 1,
//   a_k = k, except at u = Tc - 1 where the folded taps add up to w_k = sum_{j = max(k, 1) .. n} j;  b_k = k, except at u = 0 where it is w_k.
// h = g_d + D^T g_dd is rounded to fp32 (it travels through __shfl), ds once more.  On pad frames ds is g_static's word, or +0.0.
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

struct DlLane {
    long long row_in, clip;     // the lane's row of the (rows, T) side and its clip
    int j, base, f0, f, tc;     // lane inside the segment, the segment's first lane, the frame of lane 0 of the segment, the lane's frame
    bool rowok, bad, store;     // store: the lane owns frame f of an existing row (0 <= f < T, not a halo lane)
};

__device__ __forceinline__ DlLane dl_lane(const DeltasParams& p)
{
    DlLane q;
    const int lane = threadIdx.x & 63;
    // (the launcher keeps rows and the number of waves below 2^31: 32-bit quotients)
    const unsigned wid = stage_wave();
    q.j = lane & (p.W - 1);
    q.base = lane - q.j;
    unsigned row, chunk = 0;
    if (p.logw == 6) {                                             // the row is the wave's: its length comes through a scalar load
        row = wid / (unsigned)p.chunks;
        chunk = wid - row * (unsigned)p.chunks;
        q.rowok = row < (unsigned)p.rows;
        const unsigned clip = (q.rowok ? row : 0u) / (unsigned)p.rows_per_clip;
        q.clip = clip;
        q.tc = p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[clip] : p.T;
    } else {
        row = wid * (unsigned)(64 >> p.logw) + (unsigned)(lane >> p.logw);
        q.rowok = row < (unsigned)p.rows;
        q.clip = (q.rowok ? row : 0u) / (unsigned)p.rows_per_clip;
        q.tc = p.lengths ? p.lengths[q.clip] : p.T;
    }
    q.row_in = row;
    q.bad = q.tc < 1 || q.tc > p.T;
    if (q.bad) q.tc = 1;                                           // (keeps the clamps below in range; nothing of such a clip is loaded)
    q.f0 = (int)chunk * p.step - p.halo;
    q.f = q.f0 + q.j;
    q.store = q.rowok && q.j >= p.halo && q.j < p.halo + p.step && q.f < p.T;
    return q;
}

// the clamped stencil at the lane's clamped frame on the values v the segment's lanes hold; fp64 sum times 1 / denom, rounded once
__device__ __forceinline__ float dl_stencil(const DeltasParams& p, const DlLane& q, float v)
{
    const int tf = min(max(q.f, 0), q.tc - 1);
    double acc = 0.0;
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
        if (j <= p.n) {
            const int lp = min(max(min(tf + j, q.tc - 1) - q.f0, 0), p.W - 1), lm = min(max(max(tf - j, 0) - q.f0, 0), p.W - 1);
            const float a = __shfl(v, q.base + lp, 64), b = __shfl(v, q.base + lm, 64);
            acc += (double)j * ((double)a - (double)b);             // the difference first, j times it second
        }
    }
    return (float)(acc * p.inv_denom);
}

// denom (D^T v)[f] gathered by the lane of frame f; v is +0.0 on every lane whose frame lies outside 0 ... Tc - 1
__device__ __forceinline__ double dl_adjoint(const DeltasParams& p, const DlLane& q, float v)
{
    const bool last = q.f == q.tc - 1, first = q.f == 0;
    const int w0 = p.n * (p.n + 1) / 2;
    double acc = 0.0;
    if (last) acc = (double)w0 * (double)v;
    if (first) acc -= (double)w0 * (double)v;
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
        if (k <= p.n) {
            const int wk = w0 - k * (k - 1) / 2;
            const float a = __shfl(v, q.base + max(q.j - k, 0), 64), b = __shfl(v, q.base + min(q.j + k, p.W - 1), 64);
            if (q.f - k >= 0) acc = __builtin_fma((double)(last ? wk : k), (double)a, acc);
            if (q.f + k <= q.tc - 1) acc = __builtin_fma(-(double)(first ? wk : k), (double)b, acc);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(256) dmel_deltas_fwd_kernel(DeltasParams p)
{
    const DlLane q = dl_lane(p);
    const int st = p.include_static;
    const long long gs = p.rows_per_clip * (long long)p.T;         // one group of one clip
    const long long rin = q.row_in - q.clip * p.rows_per_clip;
    unsigned* y = reinterpret_cast<unsigned*>(p.out) + q.clip * p.groups * gs + rin * p.T + q.f;       // group 0, the lane's frame
    const unsigned* s = reinterpret_cast<const unsigned*>(p.in) + q.row_in * p.T + q.f;
    const bool valid = q.rowok && !q.bad && q.f >= 0 && q.f < q.tc;
    const unsigned nan = 0x7FC00000u;
    unsigned w = 0u;
    if (valid || (st && q.store && !q.bad)) w = *s;                // a pad frame is loaded for the static group only
    if (st && q.store) y[0] = q.bad ? nan : w;
    if (!__any(valid)) {                                           // a pad chunk, a clip with an invalid length, rows past the end: nothing to compute
        if (q.store) {
            y[st * gs] = q.bad ? nan : 0u;
            if (p.order == 2) y[(st + 1) * gs] = q.bad ? nan : 0u;
        }
        return;
    }
    const float d = dl_stencil(p, q, __uint_as_float(w));
    if (q.store) y[st * gs] = q.bad ? nan : (valid ? __float_as_uint(d) : 0u);
    if (p.order == 2) {
        const float dd = dl_stencil(p, q, d);
        if (q.store) y[(st + 1) * gs] = q.bad ? nan : (valid ? __float_as_uint(dd) : 0u);
    }
}

__global__ void __launch_bounds__(256) dmel_deltas_bwd_kernel(DeltasParams p)
{
    const DlLane q = dl_lane(p);
    const int st = p.include_static;
    const long long gs = p.rows_per_clip * (long long)p.T;
    const long long rin = q.row_in - q.clip * p.rows_per_clip;
    const unsigned* g = reinterpret_cast<const unsigned*>(p.in) + q.clip * p.groups * gs + rin * p.T + q.f;
    unsigned* ds = reinterpret_cast<unsigned*>(p.out) + q.row_in * p.T + q.f;
    const bool valid = q.rowok && !q.bad && q.f >= 0 && q.f < q.tc;
    const unsigned nan = 0x7FC00000u;
    unsigned w = 0u;                                               // g_static's word: every frame the lane stores
    if (st && q.store && !q.bad) w = g[0];
    if (!__any(valid)) {
        if (q.store) *ds = q.bad ? nan : w;
        return;
    }
    float h = valid ? __uint_as_float(g[st * gs]) : 0.f;
    if (p.order == 2) {
        const float gdd = valid ? __uint_as_float(g[(st + 1) * gs]) : 0.f;
        const double t = dl_adjoint(p, q, gdd);
        h = valid ? (float)__builtin_fma(t, p.inv_denom, (double)h) : 0.f;
    }
    const double t = dl_adjoint(p, q, h);
    if (q.store) *ds = q.bad ? nan : (valid ? __float_as_uint((float)__builtin_fma(t, p.inv_denom, (double)__uint_as_float(w))) : w);
}

static void deltas_geometry(DeltasParams& p)
{
    p.logw = stage_logw(p.T);
    p.halo = 0;
    p.step = 64;
    p.chunks = 1;
    if (p.T > 64) {
        p.halo = 2 * p.n;
        p.step = 64 - 2 * p.halo;
        p.chunks = (p.T + p.step - 1) / p.step;
    }
    p.W = 1 << p.logw;
}

long long deltas_waves(long long rows, int T, int n)
{
    DeltasParams p{};
    p.T = T;
    p.n = n;
    deltas_geometry(p);
    const long long per_wave = 64 >> p.logw;
    return p.logw == 6 ? rows * p.chunks : (rows + per_wave - 1) / per_wave;
}

hipError_t launch_deltas(DeltasParams p, bool backward, hipStream_t s)
{
    deltas_geometry(p);
    const long long blocks = (deltas_waves(p.rows, p.T, p.n) + 3) / 4;
    if (backward) hipLaunchKernelGGL(dmel_deltas_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(dmel_deltas_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
