// dmel_pcen.hip -- PCEN (per-channel energy normalisation, Wang et al. 2017) as a stage of its own behind the mel layers:
//   M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t];   D = eps + M;  a = E D^(-alpha);  u = a + delta;  y = u^r - delta^r
// over rows of T frames (one row = one (clip[, channel], band) pair; alpha, delta, r, s indexed by band = row % n_mels).
//
// The recurrence is a first-order linear scan with one coefficient per row, so it is done across lanes: frames sit one per lane (loads
// and stores along T stay contiguous), log2(W) combine steps with (1 - s)^(2^k), W = the segment width.  Rows of up to 32 frames share a
// wave -- 64 / W rows of W = the next power of two >= T lanes each, a segmented scan: a lane only ever takes a value from its own
// segment --, longer rows get a wave each and walk chunks of 64 frames with the last lane's value carried into the next chunk.  The
// backward is the same scan from the last frame to the first.
// Cross-lane moves are __shfl_up / __shfl_down (ds_bpermute: in-register, no LDS allocation, no barrier).  DPP row shifts would need the
// row_bcast15 / row_bcast31 fix-ups with a per-lane power of the coefficient to cross the 16-lane rows, for six moves per 64 frames of a
// kernel that spends its time in its powers (measured: both kernels run well below the HBM rate); the shuffle form is the same code for every
// segment width.
//
// Powers are exp2(y log2 x) (pcen_pow) with log2 and exp2 evaluated in fp32 pairs on reduced arguments: x = m 2^e with m in [sqrt(1/2),
// sqrt(2)), y e split exactly with an fma, the integer part through ldexp.  u^r and delta^r use this one routine: a frame with E = 0 has
// u == delta bit for bit and therefore y == +0.0.
//
// Parameter gradients: every row writes its four partial sums (fp64, fixed butterfly over its lanes) to caller scratch; a second launch adds
// the partials of each band in fp64 in a fixed order -- NOT one ascending pass over the rows: lane l of the band's wave takes rows l, l + 64,
// ... of the band in ascending order and the 64 lane sums are combined by a fixed butterfly.  No floating-point atomics: two runs give the
// same bits.
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

// log2(x) = e + hi + lo for a normal x > 0: x = m 2^e with m in [sqrt(1/2), sqrt(2)), log2 m = (2 / ln 2) atanh(t), t = (m - 1) / (m + 1),
// |t| <= 0.172, as t + t^3 / 3 + ... + t^11 / 11 with the rounding of m + 1, of the quotient and of the product carried in lo: |error| ~ 1e-9.
// (The hardware's v_log_f32 is an ulp of the result off, 6e-8 here, and v_exp_f32 an ulp of its own: with both, two powers put dE 5.6e-7 of its
// scale off at T = 1, where libm's powf stays at 6e-8.)
struct PcenLog2 { float hi, lo; int e; };
__device__ __forceinline__ PcenLog2 pcen_log2(float x)
{
#pragma clang fp contract(off)      // every fma is written out: two inlined copies must round alike (u^r against delta^r)
    constexpr double kC = 2.8853900817779268;                      // 2 / ln 2
    constexpr float c_hi = (float)kC, c_lo = (float)(kC - (double)c_hi);
    float m = __builtin_amdgcn_frexp_mantf(x);                     // [0.5, 1)
    int e = __builtin_amdgcn_frexp_expf(x);
    const bool low = m < 0.70710678f;
    m = low ? m + m : m;
    e = low ? e - 1 : e;
    const float d = m - 1.f;                                       // exact
    const float sm = m + 1.f;
    const float sm_lo = m - (sm - 1.f);                            // exact: m + 1 = sm + sm_lo
    const float t = d / sm;
    const float t_lo = (__builtin_fmaf(-t, sm, d) - t * sm_lo) * __builtin_amdgcn_rcpf(sm);
    const float p = t * t;
    float poly = __builtin_fmaf(p, 1.f / 11.f, 1.f / 9.f);
    poly = __builtin_fmaf(p, poly, 1.f / 7.f);
    poly = __builtin_fmaf(p, poly, 1.f / 5.f);
    poly = __builtin_fmaf(p, poly, 1.f / 3.f);
    const float tail = __builtin_fmaf(t, p * poly, t_lo);          // atanh(t) - t, and the quotient's rounding
    const float h0 = c_hi * t;
    const float l0 = __builtin_fmaf(c_hi, t, -h0) + __builtin_fmaf(c_hi, tail, c_lo * t);
    PcenLog2 r;
    r.hi = h0 + l0;                                                // |l0| << |h0|: hi + lo is the sum exactly
    r.lo = l0 - (r.hi - h0);
    r.e = e;
    return r;
}

// x^y = exp2(y log2 x): the integer part of y log2 x goes through ldexp, the rest g (|g| <= 1/2, carried as g + gl) through
// exp2(g) = 1 + g (ln 2 + g (...)) to degree 8, with the rounding of g ln 2 carried: about 0.7 ulp of the result in all
__device__ __forceinline__ float pcen_pow(float x, float y)
{
#pragma clang fp contract(off)
    constexpr double kL = 0.69314718055994531;
    constexpr float l_hi = (float)kL, l_lo = (float)(kL - (double)l_hi);
    const PcenLog2 L = pcen_log2(x);
    const float fe = (float)L.e;
    const float zh = y * fe;
    const float zl = __builtin_fmaf(y, fe, -zh);                   // y e = zh + zl exactly
    const float ph = y * L.hi;
    const float pl = __builtin_fmaf(y, L.hi, -ph) + __builtin_fmaf(y, L.lo, zl);
    const float n = __builtin_rintf(zh + ph);
    const float a1 = zh - n;                                       // exact
    const float g = a1 + ph;
    const float bb = g - a1;
    const float gl = ((a1 - (g - bb)) + (ph - bb)) + pl;          // a1 + ph = g + (its rounding), and the lower parts
    float q = __builtin_fmaf(g, 1.3215486790144307e-6f, 1.5252733804059841e-5f);
    q = __builtin_fmaf(g, q, 1.5403530393381608e-4f);
    q = __builtin_fmaf(g, q, 1.3333558146428443e-3f);
    q = __builtin_fmaf(g, q, 9.618129107628477e-3f);
    q = __builtin_fmaf(g, q, 5.550410866482158e-2f);
    q = __builtin_fmaf(g, q, 2.402265069591007e-1f);
    const float u1 = g * l_hi;
    float small = __builtin_fmaf(g, l_hi, -u1) + g * l_lo;
    small = __builtin_fmaf(g * g, q, small);
    small = __builtin_fmaf(l_hi * gl, 1.f + u1, small);
    const float s1 = u1 + small;                                   // |small| << |u1| or both tiny
    const float s1e = small - (s1 - u1);
    const float r0 = 1.f + s1;
    const float res = r0 + (((1.f - r0) + s1) + s1e);              // one rounding of 1 + u1 + small
    const int ni = (int)__builtin_fminf(__builtin_fmaxf(n, -400.f), 400.f);
    return __builtin_ldexpf(res, ni);
}

// ln x in fp64 from the same logarithm
__device__ __forceinline__ double pcen_ln(float x)
{
    const PcenLog2 L = pcen_log2(x);
    return 0.69314718055994531 * ((double)L.e + ((double)L.hi + (double)L.lo));
}

struct PcenRow {
    long long row, off;     // off = row * T
    int j;                  // lane inside the segment
    bool rowok;
    float alpha, delta, r, s, c;
};

// W lanes per row (a power of two <= 64; 64: one row per wave), 4 waves per workgroup
__device__ __forceinline__ PcenRow pcen_row(const PcenParams& p)
{
    PcenRow q;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int seg = lane >> p.logw;
    q.j = lane & (p.W - 1);
    q.row = wave * (64 >> p.logw) + seg;
    q.rowok = q.row < p.rows;
    q.off = q.row * (long long)p.T;
    const int band = q.rowok ? (int)(q.row % p.n_mels) : 0;
    // rows past the end compute on harmless values and store nothing
    q.alpha = q.rowok ? p.alpha[band] : 0.f;
    q.delta = q.rowok ? p.delta[band] : 1.f;
    q.r = q.rowok ? p.r[band] : 1.f;
    q.s = q.rowok ? p.s[band] : 0.5f;
    q.c = 1.f - q.s;
    return q;
}

// c^n for 1 <= n <= 64 from the same squarings the scan uses
__device__ __forceinline__ float pcen_cpow(float c, int n)
{
    float pw = 1.f, cc = c;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        pw = ((n >> k) & 1) ? pw * cc : pw;
        cc *= cc;
    }
    return pw;
}

__global__ void __launch_bounds__(256) dmel_pcen_fwd_kernel(PcenParams p)
{
    const PcenRow q = pcen_row(p);
    const int W = p.W;
    const float dpr = pcen_pow(q.delta, q.r);
    const float cin = (p.T > 64) ? pcen_cpow(q.c, q.j + 1) : 0.f;
    float carry = 0.f;
    for (int t0 = 0; t0 < p.T; t0 += 64) {                        // one pass unless W == 64 and T > 64
        const int t = t0 + q.j;
        const bool valid = q.rowok && t < p.T;
        const float e = valid ? p.E[q.off + t] : 0.f;
        float v = (t == 0) ? e : q.s * e;
        float cp = q.c;
        for (int d = 1; d < W; d <<= 1) {
            const float o = __shfl_up(v, d, 64);
            v = (q.j >= d) ? __builtin_fmaf(cp, o, v) : v;
            cp *= cp;
        }
        if (t0 > 0) v = __builtin_fmaf(cin, carry, v);
        carry = __shfl(v, 63, 64);
        const float D = p.eps + v;
        const float a = e * pcen_pow(D, -q.alpha);
        const float u = a + q.delta;
        const float y = pcen_pow(u, q.r) - dpr;
        if (valid) {
            p.y[q.off + t] = y;
            if (p.M) p.M[q.off + t] = v;
        }
    }
}

__global__ void __launch_bounds__(256) dmel_pcen_bwd_kernel(PcenParams p)
{
    const PcenRow q = pcen_row(p);
    const int W = p.W;
    const float dpr = pcen_pow(q.delta, q.r);
    const float qd = q.r * dpr / q.delta;                          // r delta^(r-1)
    const float cin = (p.T > 64) ? pcen_cpow(q.c, 64 - q.j) : 0.f;
    float carry = 0.f;
    double pa = 0.0, pd = 0.0, pr = 0.0, ps = 0.0;
    const int last = (p.T - 1) & ~63;
    for (int t0 = last; t0 >= 0; t0 -= 64) {
        const int t = t0 + q.j;
        const bool valid = q.rowok && t < p.T;
        const float g = valid ? p.g[q.off + t] : 0.f;
        const float e = valid ? p.E[q.off + t] : 0.f;
        const float m = valid ? p.Min[q.off + t] : 0.f;
        const float mprev = (valid && t >= 1) ? p.Min[q.off + t - 1] : 0.f;
        const float D = p.eps + m;
        const float Dp = pcen_pow(D, -q.alpha);
        const float a = e * Dp;
        const float u = a + q.delta;
        const float ur = pcen_pow(u, q.r);
        const float qq = q.r * ur / u;                             // r u^(r-1)
        const float gq = g * qq;
        const float h = gq * (-q.alpha * a / D);
        float v = h;
        float cp = q.c;
        for (int d = 1; d < W; d <<= 1) {
            const float o = __shfl_down(v, d, 64);
            v = (q.j + d < W) ? __builtin_fmaf(cp, o, v) : v;
            cp *= cp;
        }
        if (t0 != last) v = __builtin_fmaf(cin, carry, v);
        carry = __shfl(v, 0, 64);
        if (valid) {
            if (p.dE) p.dE[q.off + t] = __builtin_fmaf(t == 0 ? 1.f : q.s, v, gq * Dp);
            // q - r delta^(r-1) and u^r ln u - delta^r ln delta without the difference of two nearly equal powers (a << delta):
            // with lp = ln(u / delta) = log1p(a / delta) they are  r delta^(r-1) expm1((r-1) lp)  and  delta^r (expm1(r lp) ln u + lp)
            const float lp = log1pf(a / q.delta);
            // (the products of a summand in fp64: a band's gradient is a sum of many terms of both signs)
            pa -= ((double)g * (double)q.r * (double)ur / (double)u) * ((double)e * (double)Dp) * pcen_ln(D);
            pd += (double)g * ((double)qd * (double)expm1f((q.r - 1.f) * lp));
            pr += (double)g * ((double)dpr * ((double)expm1f(q.r * lp) * pcen_ln(u) + (double)lp));
            ps += (t >= 1) ? (double)v * (double)(e - mprev) : 0.0;
        }
    }
    if (p.partials) {
        // (the fp64 sums of the row, rounded once)
        const float4 sums = make_float4((float)stage_seg_sum(pa, W), (float)stage_seg_sum(pd, W), (float)stage_seg_sum(pr, W), (float)stage_seg_sum(ps, W));
        if (q.rowok && q.j == 0) *reinterpret_cast<float4*>(p.partials + q.row * 4) = sums;
    }
}

// one wave per band: lane l adds the partials of rows band + (l + 64 i) n_mels, i ascending, in fp64; the 64 lane sums are combined by a
// fixed butterfly.  dparams = (4, n_mels): alpha, delta, r, s
__global__ void __launch_bounds__(256) dmel_pcen_reduce_kernel(const float* __restrict__ partials, long long rows, int n_mels,
                                                               float* __restrict__ dparams)
{
    const int lane = threadIdx.x & 63;
    const int band = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (band >= n_mels) return;                                    // whole waves: no shuffle is left without its partner
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long row = band + (long long)lane * n_mels; row < rows; row += 64LL * n_mels) {
        const float4 v = *reinterpret_cast<const float4*>(partials + row * 4);
        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        a0 += __shfl_xor(a0, d, 64);
        a1 += __shfl_xor(a1, d, 64);
        a2 += __shfl_xor(a2, d, 64);
        a3 += __shfl_xor(a3, d, 64);
    }
    if (lane == 0) {
        dparams[band] = (float)a0;
        dparams[n_mels + band] = (float)a1;
        dparams[2 * (long long)n_mels + band] = (float)a2;
        dparams[3 * (long long)n_mels + band] = (float)a3;
    }
}

static void pcen_geometry(PcenParams& p)
{
    p.logw = stage_logw(p.T);
    p.W = 1 << p.logw;
}

hipError_t launch_pcen_fwd(PcenParams p, hipStream_t s)
{
    pcen_geometry(p);
    hipLaunchKernelGGL(dmel_pcen_fwd_kernel, dim3((unsigned)stage_row_blocks(p.rows, p.T)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_pcen_bwd(PcenParams p, float* dparams, hipStream_t s)
{
    pcen_geometry(p);
    hipLaunchKernelGGL(dmel_pcen_bwd_kernel, dim3((unsigned)stage_row_blocks(p.rows, p.T)), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dparams) return e;
    hipLaunchKernelGGL(dmel_pcen_reduce_kernel, dim3((unsigned)((p.n_mels + 3) / 4)), dim3(256), 0, s, p.partials, p.rows, p.n_mels, dparams);
    return hipGetLastError();
}

}  // namespace dmel
