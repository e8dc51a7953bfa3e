// dmel_fwd_band.hip -- the fused forward of BandSplitMelSpectrogram (dmel_forward_band*): K window widths inside ONE (B, 1, M, T) image.
//
// dmel_fwd_band_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_MULTI = 1 and DMEL_FWD_BAND = 1: the multi-window kernel's channel
// addressing (channel slot from the relabelled workgroup index, lam_for_channel, the channel's window table and lambd words), but the clip's
// output base is the one-channel image's and channel c produces rows [e_c, e_c+1) only (FwdBandParams::band_edges).  The rows' values are the
// scalar kernel's to the bit: a row's products are accumulated exactly as there; what changes is which tiles / phases run and which rows are
// stored -- a banded 16 x 16 x 4 tile (or a piece of one) none of whose bands is the channel's is not contracted, a wave-local phase none of
// whose quads holds one runs no steps, and the result rows, the staged rows, the NaN rows of an uncovered channel and the bf16 stores are
// confined to the range.  Built for kTrain, kTrainW, kInfer, n_fft 32 ... 16384, one tile per workgroup, in a translation unit of its own
// (four parts, split as dmel_fwd.hip's): the existing kernels are compiled exactly as before.
#include "dmel_kernels.h"
#include "dmel_wavefft.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_MULTI 1
#define DMEL_FWD_BAND 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_BAND
#undef DMEL_FWD_MULTI

template <int N, int MODE, int TPW> static hipError_t launch_band_one(const FwdBandParams& p, int grid, hipStream_t s)
{
    constexpr FftGeom g = geom_mode<N, MODE>();
    hipLaunchKernelGGL((dmel_fwd_band_kernel<N, MODE, TPW>), dim3(grid), dim3(g.THREADS), g.LDS_BYTES, s, p);
    return hipGetLastError();
}

// one tile per workgroup only (as dmel_fwd_len.hip)
template <int N, int MODE> static hipError_t launch_band_mode(int tpw, const FwdBandParams& p, int grid, hipStream_t s)
{
    if (tpw != 1) return hipErrorInvalidValue;
    if constexpr (MODE == kTrainW && !wlc_size(N)) return hipErrorInvalidValue;
    else return launch_band_one<N, MODE, 1>(p, grid, s);
}

template <int N, int MODE> static hipError_t set_band_attr_mode()
{
    if constexpr (MODE == kTrainW && !wlc_size(N)) return hipSuccess;
    else return hipFuncSetAttribute(reinterpret_cast<const void*>(&dmel_fwd_band_kernel<N, MODE, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    geom_mode<N, MODE>().LDS_BYTES);
}

// -DDMEL_FWD_SPLIT -DDMEL_FWD_PART=<k>: build.py compiles this file four times, the sizes dealt as in dmel_fwd.hip
#ifndef DMEL_FWD_PART
#define DMEL_FWD_PART 0
#endif
constexpr int band_part_of(int n) { return n <= 512 ? 0 : n == 1024 ? 1 : (n == 2048 || n == 16384) ? 2 : 3; }
#if defined(DMEL_FWD_SPLIT)
#define DMEL_BAND_HERE(n) (band_part_of(n) == DMEL_FWD_PART)
#else
#define DMEL_BAND_HERE(n) true
#endif

template <int N> static hipError_t launch_band_size(int mode, int tpw, const FwdBandParams& p, int grid, hipStream_t s)
{
    if constexpr (!DMEL_BAND_HERE(N)) return hipErrorInvalidValue;
    else {
        switch (mode) {
            case kTrain: return launch_band_mode<N, kTrain>(tpw, p, grid, s);
            case kTrainW: return launch_band_mode<N, kTrainW>(tpw, p, grid, s);
            case kInfer: return launch_band_mode<N, kInfer>(tpw, p, grid, s);
        }
        return hipErrorInvalidValue;
    }
}

template <int N> static hipError_t set_band_attr_n()
{
    if constexpr (!DMEL_BAND_HERE(N)) return hipSuccess;
    else {
        hipError_t e;
        if ((e = set_band_attr_mode<N, kTrain>()) != hipSuccess) return e;
        if ((e = set_band_attr_mode<N, kTrainW>()) != hipSuccess) return e;
        return set_band_attr_mode<N, kInfer>();
    }
}

#define DMEL_BAND_CAT2(a, b) a##b
#define DMEL_BAND_CAT(a, b) DMEL_BAND_CAT2(a, b)
hipError_t DMEL_BAND_CAT(launch_forward_band_part, DMEL_FWD_PART)(int n_fft, int mode, int tpw, const FwdBandParams& p, int grid, hipStream_t s)
{
    switch (n_fft) {
        case 32: return launch_band_size<32>(mode, tpw, p, grid, s);
        case 64: return launch_band_size<64>(mode, tpw, p, grid, s);
        case 128: return launch_band_size<128>(mode, tpw, p, grid, s);
        case 256: return launch_band_size<256>(mode, tpw, p, grid, s);
        case 512: return launch_band_size<512>(mode, tpw, p, grid, s);
        case 1024: return launch_band_size<1024>(mode, tpw, p, grid, s);
        case 2048: return launch_band_size<2048>(mode, tpw, p, grid, s);
        case 4096: return launch_band_size<4096>(mode, tpw, p, grid, s);
        case 8192: return launch_band_size<8192>(mode, tpw, p, grid, s);
        case 16384: return launch_band_size<16384>(mode, tpw, p, grid, s);
    }
    return hipErrorInvalidValue;
}

hipError_t DMEL_BAND_CAT(forward_band_prepare_attributes_part, DMEL_FWD_PART)()
{
    hipError_t e;
    if ((e = set_band_attr_n<32>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<64>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<128>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<256>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<512>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<1024>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<2048>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<4096>()) != hipSuccess) return e;
    if ((e = set_band_attr_n<8192>()) != hipSuccess) return e;
    return set_band_attr_n<16384>();
}

#if DMEL_FWD_PART == 0
#if defined(DMEL_FWD_SPLIT)
hipError_t launch_forward_band_part1(int, int, int, const FwdBandParams&, int, hipStream_t);
hipError_t launch_forward_band_part2(int, int, int, const FwdBandParams&, int, hipStream_t);
hipError_t launch_forward_band_part3(int, int, int, const FwdBandParams&, int, hipStream_t);
hipError_t forward_band_prepare_attributes_part1();
hipError_t forward_band_prepare_attributes_part2();
hipError_t forward_band_prepare_attributes_part3();
#endif
hipError_t launch_forward_band(int n_fft, int mode, int tpw, const FwdBandParams& p, int grid, hipStream_t s)
{
#if defined(DMEL_FWD_SPLIT)
    switch (band_part_of(n_fft)) {
        case 1: return launch_forward_band_part1(n_fft, mode, tpw, p, grid, s);
        case 2: return launch_forward_band_part2(n_fft, mode, tpw, p, grid, s);
        case 3: return launch_forward_band_part3(n_fft, mode, tpw, p, grid, s);
    }
#endif
    return launch_forward_band_part0(n_fft, mode, tpw, p, grid, s);
}

hipError_t forward_band_prepare_attributes()
{
    hipError_t e;
    if ((e = forward_band_prepare_attributes_part0()) != hipSuccess) return e;
#if defined(DMEL_FWD_SPLIT)
    if ((e = forward_band_prepare_attributes_part1()) != hipSuccess) return e;
    if ((e = forward_band_prepare_attributes_part2()) != hipSuccess) return e;
    if ((e = forward_band_prepare_attributes_part3()) != hipSuccess) return e;
#endif
    return hipSuccess;
}
#endif

}  // namespace dmel
