// dmel_fwd_len.hip -- the fused forward over clips of per-clip lengths (MelSpectrogramLayer.forward(x, lengths), dmel_forward_*lengths).
//
// dmel_fwd_len_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_LEN = 1: every sample-space bound of the clip (the buffer resource,
// the interior / edge test, the load clamps, the window-multiply masks, the three clip sums and their quotient) is the clip's own length
// Lc = lengths[b] instead of n_points; the frames at or past Tc = Lc / hop + 1 are pad frames (zero mel power: 0, or the epilogue's own
// log(0 + eps); tangent 0), and a tile whose first frame is a pad frame writes its rows and skips the transform and the contraction.
// Built for the modes of the HTK layer (kTrain, kTrainW, kInfer), n_fft 32 ... 16384, in a translation unit of its own (four parts, split
// as dmel_fwd.hip's): dmel_fwd_kernel and dmel_fwd_multi_kernel are compiled exactly as before.
#include "dmel_kernels.h"
#include "dmel_wavefft.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_LEN 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_LEN

template <int N, int MODE, int TPW> static hipError_t launch_len_one(const FwdLenParams& p, int grid, hipStream_t s)
{
    constexpr FftGeom g = geom_mode<N, MODE>();
    hipLaunchKernelGGL((dmel_fwd_len_kernel<N, MODE, TPW>), dim3(grid), dim3(g.THREADS), g.LDS_BYTES, s, p);
    return hipGetLastError();
}

// one tile per workgroup only: the two-tile variants of dmel_fwd.hip spill here (<512, kTrain, 2>: 3 registers, 16 bytes of scratch)
template <int N, int MODE> static hipError_t launch_len_mode(int tpw, const FwdLenParams& p, int grid, hipStream_t s)
{
    if (tpw != 1) return hipErrorInvalidValue;
    if constexpr (MODE == kTrainW && !wlc_size(N)) return hipErrorInvalidValue;
    else return launch_len_one<N, MODE, 1>(p, grid, s);
}

template <int N, int MODE> static hipError_t set_len_attr_mode()
{
    if constexpr (MODE == kTrainW && !wlc_size(N)) return hipSuccess;
    else return hipFuncSetAttribute(reinterpret_cast<const void*>(&dmel_fwd_len_kernel<N, MODE, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    geom_mode<N, MODE>().LDS_BYTES);
}

// -DDMEL_FWD_SPLIT -DDMEL_FWD_PART=<k>: build.py compiles this file four times, the sizes dealt as in dmel_fwd.hip
#ifndef DMEL_FWD_PART
#define DMEL_FWD_PART 0
#endif
constexpr int len_part_of(int n) { return n <= 512 ? 0 : n == 1024 ? 1 : (n == 2048 || n == 16384) ? 2 : 3; }
#if defined(DMEL_FWD_SPLIT)
#define DMEL_LEN_HERE(n) (len_part_of(n) == DMEL_FWD_PART)
#else
#define DMEL_LEN_HERE(n) true
#endif

template <int N> static hipError_t launch_len_size(int mode, int tpw, const FwdLenParams& p, int grid, hipStream_t s)
{
    if constexpr (!DMEL_LEN_HERE(N)) return hipErrorInvalidValue;
    else {
        switch (mode) {
            case kTrain: return launch_len_mode<N, kTrain>(tpw, p, grid, s);
            case kTrainW: return launch_len_mode<N, kTrainW>(tpw, p, grid, s);
            case kInfer: return launch_len_mode<N, kInfer>(tpw, p, grid, s);
        }
        return hipErrorInvalidValue;
    }
}

template <int N> static hipError_t set_len_attr_n()
{
    if constexpr (!DMEL_LEN_HERE(N)) return hipSuccess;
    else {
        hipError_t e;
        if ((e = set_len_attr_mode<N, kTrain>()) != hipSuccess) return e;
        if ((e = set_len_attr_mode<N, kTrainW>()) != hipSuccess) return e;
        return set_len_attr_mode<N, kInfer>();
    }
}

#define DMEL_LEN_CAT2(a, b) a##b
#define DMEL_LEN_CAT(a, b) DMEL_LEN_CAT2(a, b)
hipError_t DMEL_LEN_CAT(launch_forward_len_part, DMEL_FWD_PART)(int n_fft, int mode, int tpw, const FwdLenParams& p, int grid, hipStream_t s)
{
    switch (n_fft) {
        case 32: return launch_len_size<32>(mode, tpw, p, grid, s);
        case 64: return launch_len_size<64>(mode, tpw, p, grid, s);
        case 128: return launch_len_size<128>(mode, tpw, p, grid, s);
        case 256: return launch_len_size<256>(mode, tpw, p, grid, s);
        case 512: return launch_len_size<512>(mode, tpw, p, grid, s);
        case 1024: return launch_len_size<1024>(mode, tpw, p, grid, s);
        case 2048: return launch_len_size<2048>(mode, tpw, p, grid, s);
        case 4096: return launch_len_size<4096>(mode, tpw, p, grid, s);
        case 8192: return launch_len_size<8192>(mode, tpw, p, grid, s);
        case 16384: return launch_len_size<16384>(mode, tpw, p, grid, s);
    }
    return hipErrorInvalidValue;
}

hipError_t DMEL_LEN_CAT(forward_len_prepare_attributes_part, DMEL_FWD_PART)()
{
    hipError_t e;
    if ((e = set_len_attr_n<32>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<64>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<128>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<256>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<512>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<1024>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<2048>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<4096>()) != hipSuccess) return e;
    if ((e = set_len_attr_n<8192>()) != hipSuccess) return e;
    return set_len_attr_n<16384>();
}

#if DMEL_FWD_PART == 0
#if defined(DMEL_FWD_SPLIT)
hipError_t launch_forward_len_part1(int, int, int, const FwdLenParams&, int, hipStream_t);
hipError_t launch_forward_len_part2(int, int, int, const FwdLenParams&, int, hipStream_t);
hipError_t launch_forward_len_part3(int, int, int, const FwdLenParams&, int, hipStream_t);
hipError_t forward_len_prepare_attributes_part1();
hipError_t forward_len_prepare_attributes_part2();
hipError_t forward_len_prepare_attributes_part3();
#endif
hipError_t launch_forward_len(int n_fft, int mode, int tpw, const FwdLenParams& p, int grid, hipStream_t s)
{
#if defined(DMEL_FWD_SPLIT)
    switch (len_part_of(n_fft)) {
        case 1: return launch_forward_len_part1(n_fft, mode, tpw, p, grid, s);
        case 2: return launch_forward_len_part2(n_fft, mode, tpw, p, grid, s);
        case 3: return launch_forward_len_part3(n_fft, mode, tpw, p, grid, s);
    }
#endif
    return launch_forward_len_part0(n_fft, mode, tpw, p, grid, s);
}

hipError_t forward_len_prepare_attributes()
{
    hipError_t e;
    if ((e = forward_len_prepare_attributes_part0()) != hipSuccess) return e;
#if defined(DMEL_FWD_SPLIT)
    if ((e = forward_len_prepare_attributes_part1()) != hipSuccess) return e;
    if ((e = forward_len_prepare_attributes_part2()) != hipSuccess) return e;
    if ((e = forward_len_prepare_attributes_part3()) != hipSuccess) return e;
#endif
    return hipSuccess;
}
#endif

}  // namespace dmel
