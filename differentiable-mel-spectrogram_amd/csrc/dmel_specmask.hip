// dmel_specmask.hip -- SpecMask: length-aware SpecAugment stripes as a stage of its own behind the mel layers.  An image is one (clip,
// channel) pair of a contiguous (B[, C], n_mels, T) tensor, i = clip * C + channel: n_mels * T consecutive elements.  Every image draws n_time
// time stripes over its clip's valid frames t < Tc and n_freq frequency stripes over its bands, independently of every other image:
//   y = fill  where a valid frame lies in a time stripe or its band in a frequency stripe;  y = s bit for bit elsewhere and on every pad frame
// Everything is integer arithmetic: a numpy restatement gives every stripe and every output bit (tests/specmask_cases.py).
//
// Two roles:
//   draw    one workgroup; a lane per (image, stripe) in rounds of 1024.  Philox4x32-10, key = seed, counter = (calls lo, calls hi, image,
//           stripe / 2), the stripe takes the word pair 2 (stripe % 2): width = mulhi(w_a, cap), lo = mulhi(w_b, size - width).  The table
//           (images, n_time + n_freq, 2) of [lo, hi) pairs is all the apply kernel and the backward read.  `calls` is read by every lane
//           before its first draw and stored as calls + 1 by lane 0 behind the workgroup's barrier: no race, no atomic, no host read.
//   apply   a wave takes a run of consecutive elements of ONE image (rows of any length share it), so the image's stripe pairs and its
//           clip's length are wave-uniform: read once per wave through scalar loads, tested from scalar registers.  Elements are moved as
//           2- or 4-byte words, never converted.  16 bytes per lane where s and y of the image sit alike inside a 16-byte granule (the
//           lanes' granules are those of y; the partial ones at both ends of the image go element by element), element-wide accesses
//           otherwise -- chosen per image from the two addresses.  The loads are issued first and the masks computed under them.  Offsets are 64-bit.
// The backward is the apply kernel on the cotangent with fill +0.0.  A length outside 1 ... T makes every element of its clip NaN (and the
// draw leaves that clip's table rows zero).
#include "dmel_kernels.h"
#include "dmel_stage.h"

namespace dmel {

struct SmWord4 { unsigned x, y, z, w; };

__device__ __forceinline__ SmWord4 sm_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return SmWord4{c0, c1, c2, c3};
}

__global__ void __launch_bounds__(1024) dmel_specmask_draw_kernel(SpecMaskDrawParams p)
{
    const unsigned long long seed = p.rng_state[0], calls = p.rng_state[1];
    const int n = p.n_time + p.n_freq;
    const long long items = p.images * n;
    for (long long item = threadIdx.x; item < items; item += 1024) {
        const long long image = item / n;
        const int k = (int)(item - image * n);
        const int tc = stage_length(p.lengths, image / p.channels, p.T);
        int lo = 0, hi = 0;
        if (!stage_bad(tc, p.T)) {
            const SmWord4 w = sm_philox((unsigned)calls, (unsigned)(calls >> 32), (unsigned)image, (unsigned)(k >> 1), (unsigned)seed,
                                        (unsigned)(seed >> 32));
            const unsigned wa = (k & 1) ? w.z : w.x, wb = (k & 1) ? w.w : w.y;
            int size, param;
            if (k < p.n_time) {
                size = tc;
                const long long adaptive = (long long)tc * p.time_permille / 1000;
                param = adaptive < p.time_param ? (int)adaptive : p.time_param;
            } else {
                size = p.n_mels;
                param = p.freq_param;
            }
            const unsigned cap = (unsigned)(param < size ? param : size);
            const unsigned width = __umulhi(wa, cap);
            lo = (int)__umulhi(wb, (unsigned)size - width);
            hi = lo + (int)width;
        }
        p.stripes[2 * item] = lo;
        p.stripes[2 * item + 1] = hi;
    }
    __syncthreads();                                               // every lane has read `calls` (before its first draw)
    if (p.advance && threadIdx.x == 0) p.rng_state[1] = calls + 1;
}

constexpr int kSmIter = 2;      // 16-byte granules per lane: both loads are issued before anything waits for them

// E: the element as an unsigned word (4 bytes: fp32, 2 bytes: bf16); VE elements per 16 bytes.  Three phases: the loads (they depend on
// the addresses only), the image's length and stripe pairs and the masks of the lane's granules while the loads fly, the selects and stores.
// EDGE = false: every granule of the wave is a whole one (or past the image's end) -- 16-byte accesses only, what nearly every wave runs;
// EDGE = true: granules that are not whole are gathered and stored element by element.
template <typename E, int VE, bool EDGE>
__device__ __forceinline__ void sm_apply_body(const SpecMaskParams& p, unsigned image, const E* s, E* y, int nt, const int (&e0)[kSmIter],
                                              const bool (&whole)[kSmIter])
{
    uint4 v[kSmIter];                                              // the granule's 16 bytes as one load ...
    unsigned ew[kSmIter][4];                                       // ... or (EDGE) gathered element by element
#pragma unroll
    for (int it = 0; it < kSmIter; ++it) {
        v[it] = make_uint4(0u, 0u, 0u, 0u);
        if (whole[it]) v[it] = *reinterpret_cast<const uint4*>(s + e0[it]);
    }
#pragma unroll
    for (int it = 0; it < kSmIter; ++it) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ew[it][q] = 0u;
        if (EDGE && !whole[it]) {
#pragma unroll
            for (int j = 0; j < VE; ++j) {
                const int e = e0[it] + j;
                if (e >= 0 && e < nt) ew[it][j * (int)sizeof(E) / 4] |= (unsigned)s[e] << (8 * ((j * (int)sizeof(E)) & 3));
            }
        }
    }

    const unsigned clip = image / (unsigned)p.channels;
    const int tc = p.lengths ? ((stage_const_ints)(unsigned long long)p.lengths)[clip] : p.T;
    const bool bad = tc < 1 || tc > p.T;
    // the image's stripe pairs: uniform addresses in the constant address space (the draw kernel finished before this one started)
    const int n = p.n_time + p.n_freq;
    const stage_const_ints tab = (stage_const_ints)(unsigned long long)p.stripes + (long long)image * (2 * n);
    int lo[8], hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        lo[k] = hi[k] = 0;
        if (k < n) { lo[k] = tab[2 * k]; hi[k] = tab[2 * k + 1]; }
    }
    const unsigned fill = p.fill_bits, nan = sizeof(E) == 4 ? 0x7FC00000u : 0x7FC0u;
    const unsigned put = bad ? nan : fill;

#pragma unroll
    for (int it = 0; it < kSmIter; ++it) {
        if (e0[it] >= nt) continue;
        if (!EDGE && !whole[it]) continue;
        // (band, frame) of the granule's first element: first / T by the launcher's multiplier, exact below 2^30
        const unsigned first = (unsigned)(e0[it] < 0 ? 0 : e0[it]);
        int band = (int)(((unsigned long long)first * p.t_magic) >> p.t_shift), t = (int)first - band * p.T;
        // the VE positions, then one uniform branch per stripe (not one select per element and stripe)
        int tj[VE], bj[VE];
        unsigned valid = 0u;
#pragma unroll
        for (int j = 0; j < VE; ++j) {
            tj[j] = t;
            bj[j] = band;
            valid |= ((t < tc) ? 1u : 0u) << j;
            if (e0[it] + j >= 0 && ++t == p.T) { t = 0; ++band; }
        }
        unsigned hit = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < n) {
                const int l = lo[k];
                const unsigned w = (unsigned)(hi[k] - l);
                if (k < p.n_time) {
#pragma unroll
                    for (int j = 0; j < VE; ++j) hit |= (((unsigned)(tj[j] - l) < w) ? 1u : 0u) << j;
                } else {
#pragma unroll
                    for (int j = 0; j < VE; ++j) hit |= (((unsigned)(bj[j] - l) < w) ? 1u : 0u) << j;
                }
            }
        }
        // a time stripe lies inside the valid frames by construction; a frequency stripe spares the pad frames
        const unsigned masked = bad ? ~0u : (hit & valid);
        const bool vec = !EDGE || whole[it];
        const unsigned words[4] = {vec ? v[it].x : ew[it][0], vec ? v[it].y : ew[it][1], vec ? v[it].z : ew[it][2], vec ? v[it].w : ew[it][3]};
        unsigned res[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (sizeof(E) == 4) {
                res[q] = ((masked >> q) & 1u) ? put : words[q];
            } else {
                const unsigned a = ((masked >> (2 * q)) & 1u) ? put : (words[q] & 0xFFFFu);
                const unsigned b = ((masked >> (2 * q + 1)) & 1u) ? put : (words[q] >> 16);
                res[q] = a | (b << 16);
            }
        }
        if (vec) {
            *reinterpret_cast<uint4*>(y + e0[it]) = make_uint4(res[0], res[1], res[2], res[3]);
        } else {
#pragma unroll
            for (int j = 0; j < VE; ++j) {
                const int e = e0[it] + j;
                if (e >= 0 && e < nt) y[e] = (E)(res[j * (int)sizeof(E) / 4] >> (8 * ((j * (int)sizeof(E)) & 3)));
            }
        }
    }
}

template <typename E, int VE>
__global__ void __launch_bounds__(256) dmel_specmask_apply_kernel(SpecMaskParams p)
{
    const int lane = threadIdx.x & 63;
    // (the launcher keeps images * waves_per_image below 2^31: 32-bit quotients, one per wave)
    const unsigned wid = stage_wave();
    const unsigned image = wid / (unsigned)p.waves_per_image;
    if (image >= (unsigned)p.images) return;                       // whole waves
    const int chunk = (int)(wid - image * (unsigned)p.waves_per_image);
    const int nt = p.n_mels * p.T;
    const E* s = static_cast<const E*>(p.s) + (long long)image * nt;
    E* y = static_cast<E*>(p.y) + (long long)image * nt;
    const int shift = (int)(((unsigned long long)y & 15) / sizeof(E));     // y's elements in front of the image inside its first granule
    const bool alike = ((((unsigned long long)s) ^ ((unsigned long long)y)) & 15) == 0;
    int e0[kSmIter];
    bool whole[kSmIter], plain = true;
#pragma unroll
    for (int it = 0; it < kSmIter; ++it) {
        e0[it] = ((chunk * kSmIter + it) * 64 + lane) * VE - shift;
        whole[it] = alike && e0[it] >= 0 && e0[it] + VE <= nt;
        plain = plain && (whole[it] || e0[it] >= nt);
    }
    if (__all(plain)) sm_apply_body<E, VE, false>(p, image, s, y, nt, e0, whole);
    else sm_apply_body<E, VE, true>(p, image, s, y, nt, e0, whole);
}

long long specmask_waves_per_image(int n_mels, int T, int elem_bytes)
{
    const long long ve = 16 / elem_bytes, per_wave = 64LL * ve * kSmIter;
    return ((long long)n_mels * T + (ve - 1) + per_wave - 1) / per_wave;      // (up to ve - 1 elements of shift in front)
}

hipError_t launch_specmask_draw(const SpecMaskDrawParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(dmel_specmask_draw_kernel, dim3(1), dim3(1024), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_specmask_apply(SpecMaskParams p, int elem_bytes, hipStream_t s)
{
    p.waves_per_image = specmask_waves_per_image(p.n_mels, p.T, elem_bytes);
    // floor(e / T) = (e * t_magic) >> t_shift for 0 <= e < 2^30: t_magic = ceil(2^(30 + l) / T), l = ceil(log2 T) (Granlund and Montgomery)
    int l = 0;
    while ((1LL << l) < p.T) ++l;
    p.t_shift = 30 + l;
    p.t_magic = (unsigned)(((1ULL << p.t_shift) + (unsigned long long)p.T - 1) / (unsigned long long)p.T);
    const long long blocks = (p.images * p.waves_per_image + 3) / 4;
    if (elem_bytes == 4) hipLaunchKernelGGL((dmel_specmask_apply_kernel<unsigned, 4>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((dmel_specmask_apply_kernel<unsigned short, 8>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace dmel
