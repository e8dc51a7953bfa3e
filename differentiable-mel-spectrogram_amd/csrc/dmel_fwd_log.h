// dmel_fwd_log.h -- the fused epilogue's logarithm, included inside namespace dmel by dmel_fwd.hip and dmel_fwd_len.hip (one translation unit
// each: the two copies of slow_log live in different code objects).

// log(me), me = mel + eps, for the fused epilogue (models.py:73).  With the reference's eps (1e-10, any eps >= 1e-30) the argument is a
// normal number: v_log_f32 (log2, 1 ulp) times ln 2 -- 2 instructions against ~12 of logf(), whose extra work is the scaling of
// denormal arguments; absolute error <= 3e-6 at |log| = 23 (the 1e-4 bar of the path is absolute in the log domain).  eps below
// that (or negative): logf().  The choice is uniform over the launch.
__device__ __attribute__((noinline)) float slow_log(float me) { return logf(me); }   // (a call: the compiler does not fold the two paths into a select)
__device__ __forceinline__ float fast_log(float me, float eps)
{
    if (eps >= 1e-30f) return __builtin_amdgcn_logf(me) * 0.69314718055994530942f;
    return slow_log(me);
}
