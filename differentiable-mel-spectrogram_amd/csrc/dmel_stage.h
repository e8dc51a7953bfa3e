// dmel_stage.h -- what the stages behind the mel layers (dmel_pcen.hip, dmel_bandnorm.hip, dmel_specmask.hip, dmel_deltas.hip,
// dmel_statspool.hip, dmel_attnpool.hip) share; included after dmel_kernels.h.  A row is T frames of one (clip[, channel], band) triple,
// clip = row / rows_per_clip, and its valid frames are t < lengths[clip].
//   geometry   frames one per lane; rows of up to 32 frames are packed 64 / W to a wave, W = 1 << logw the next power of two >= T; longer
//              rows get a wave each (logw = 6).  Workgroups of 4 waves.
//   lengths    lengths[clip] (nullptr: T), through the constant address space where the clip is the wave's; a length outside 1 ... T is
//              invalid: such a clip has no valid frame and its outputs are NaN.
// The per-lane row descriptors (bn_row, dl_lane, sp_row, ap_row) stay in their files and are built from these pieces.
//   sums       the W lanes of a row meet through a fixed butterfly in registers: no LDS, no barrier, the same bits every run.
#pragma once

namespace dmel {

// nothing writes these buffers while a kernel reads them: a uniform address in the constant address space is a scalar load
typedef const int __attribute__((address_space(4))) * stage_const_ints;
typedef const float __attribute__((address_space(4))) * stage_const_floats;
typedef const double __attribute__((address_space(4))) * stage_const_doubles;

// log2 of the lanes a row of T frames takes
inline int stage_logw(int T)
{
    int logw = 6;
    if (T <= 32) {
        logw = 0;
        while ((1 << logw) < T) ++logw;
    }
    return logw;
}

// workgroups of a launch with one segment of lanes per row
inline long long stage_row_blocks(long long rows, int T)
{
    const long long per_block = 4LL * (64 >> stage_logw(T));
    return (rows + per_block - 1) / per_block;
}

// the wave's number in a launch of 4-wave workgroups, in a scalar register
__device__ __forceinline__ unsigned stage_wave()
{
    return blockIdx.x * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// lengths[clip], or T without lengths, for a clip that is a 64-bit value per lane.  Where the clip is the same in every lane of a wave the
// load is spelled in place through stage_const_ints: ((stage_const_ints)(unsigned long long)lengths)[clip]
__device__ __forceinline__ int stage_length(const int* lengths, long long clip, int T)
{
    return lengths ? lengths[clip] : T;
}

// the invalid-length rule: a length outside 1 ... T is bad, and a clip with a bad length has no valid frame
__device__ __forceinline__ bool stage_bad(int tc, int T)
{
    return tc < 1 || tc > T;
}
__device__ __forceinline__ int stage_valid(int tc, int T, bool& bad)
{
    bad = stage_bad(tc, T);
    return bad ? 0 : tc;
}

// sum over the W lanes of a segment in fp64, the same order every run; every lane of the segment ends with the sum
__device__ __forceinline__ double stage_seg_sum(double v, int W)
{
    for (int d = W >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace dmel
