// dmel_fwd_dispatch.h -- the launch and attribute scaffolding the builds of the fused forward share: dmel_fwd.hip (dmel_fwd_kernel,
// dmel_fwd_multi_kernel), dmel_fwd_len.hip (dmel_fwd_len_kernel), dmel_fwd_band.hip (dmel_fwd_band_kernel), dmel_fwd_multi_len.hip
// (dmel_fwd_multi_len_kernel) and dmel_fwd_band_len.hip (dmel_fwd_band_len_kernel).  Each of them describes itself in a variant V:
//
//   using Params                                       FwdParams or what derives from it
//   using Modes = FwdModes<...>                        the modes it is built for
//   template <int N, int MODE, int TPW> exists()       the instantiations <N, MODE, TPW> it holds
//   template <int N, int MODE, int TPW> kernels[]      the kernel (or kernels) of one instantiation
//   static int pick(const Params&)                     which of them a launch takes
//
// and ends with DMEL_FWD_PARTS_OF(V).  Everything else -- the split into parts, the entry points -- is here; the map from n_fft to N is with_nfft (dmel_kernels.h).
#pragma once
#include "dmel_kernels.h"
#include "dmel_wavefft.h"

namespace dmel {

// -DDMEL_FWD_SPLIT -DDMEL_FWD_PART=<k>, k = 0..3: build.py compiles each of these files four times for libdmel_hip.so so that the
// instantiations of the large transforms -- minutes of compile time each -- build in parallel: part 0 holds everything that is not a template
// instantiation plus the sizes up to 512, parts 1-3 hold 1024 / 2048 + 16384 / 4096 + 8192 and nothing else.  Without DMEL_FWD_SPLIT (the
// tools' one-command builds) everything is in one translation unit, part 0.
// -DDMEL_ONLY_NFFT=<n>: development builds that instantiate one transform size only (tools/build_variant.sh), unsplit.  Never defined for
// libdmel_hip.so.
#ifndef DMEL_FWD_PART
#define DMEL_FWD_PART 0
#endif
#if defined(DMEL_FWD_SPLIT) && !defined(DMEL_ONLY_NFFT)
constexpr bool kFwdSplit = true;
#else
constexpr bool kFwdSplit = false;
#endif
constexpr int fwd_part_of(int n) { return n <= 512 ? 0 : n == 1024 ? 1 : (n == 2048 || n == 16384) ? 2 : 3; }
template <int PART> constexpr bool fwd_here(int n)      // size n is instantiated in part PART of this build
{
#if defined(DMEL_ONLY_NFFT)
    return n == DMEL_ONLY_NFFT;
#else
    return !kFwdSplit || fwd_part_of(n) == PART;
#endif
}

template <int... MODES> struct FwdModes {};

template <class V, int N, int MODE, int TPW> static hipError_t fwd_launch_one(const typename V::Params& p, int grid, hipStream_t s)
{
    constexpr FftGeom g = geom_mode<N, MODE>();
    const auto kernel = V::template kernels<N, MODE, TPW>[V::pick(p)];
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(g.THREADS), g.LDS_BYTES, s, p);
    return hipGetLastError();
}

template <class V, int N, int MODE> static hipError_t fwd_launch_mode(int tpw, const typename V::Params& p, int grid, hipStream_t s)
{
    if constexpr (V::template exists<N, MODE, 2>()) { if (tpw == 2) return fwd_launch_one<V, N, MODE, 2>(p, grid, s); }
    if constexpr (V::template exists<N, MODE, 1>()) { if (tpw == 1) return fwd_launch_one<V, N, MODE, 1>(p, grid, s); }
    return hipErrorInvalidValue;
}

template <class V, int N, int... MODES> static hipError_t fwd_launch_n(FwdModes<MODES...>, int mode, int tpw, const typename V::Params& p, int grid, hipStream_t s)
{
    hipError_t e = hipErrorInvalidValue;
    ((mode == MODES ? (void)(e = fwd_launch_mode<V, N, MODES>(tpw, p, grid, s)) : (void)0), ...);
    return e;
}

// raises the dynamic-LDS limit of every kernel of the instantiations <N, MODE, *>
template <class V, int N, int MODE> static hipError_t fwd_set_attr_mode()
{
    hipError_t e = hipSuccess;
    auto set = [&](auto tt) {
        constexpr int TPW = decltype(tt)::value;
        if constexpr (V::template exists<N, MODE, TPW>())
            for (auto kernel : V::template kernels<N, MODE, TPW>)
                if (e == hipSuccess)
                    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, geom_mode<N, MODE>().LDS_BYTES);
    };
    set(IC<1>{});
    set(IC<2>{});
    return e;
}

template <class V, int N, int... MODES> static hipError_t fwd_set_attr_n(FwdModes<MODES...>)
{
    static_assert(geom<N, true>().WAVES == geom<N, false>().WAVES && geom<N, true>().NBPRE == geom<N, false>().NBPRE,
                  "both plans of a size share the filterbank fragment layout");
    hipError_t e = hipSuccess;
    ((e == hipSuccess ? (void)(e = fwd_set_attr_mode<V, N, MODES>()) : (void)0), ...);
    return e;
}

// ---- the parts: every part instantiates these two for its own number (DMEL_FWD_PARTS_OF), part 0 reaches the others' through fwd_launch /
// fwd_set_attr
template <class V, int PART> hipError_t fwd_launch_part(int n_fft, int mode, int tpw, const typename V::Params& p, int grid, hipStream_t s)
{
    hipError_t e = hipErrorInvalidValue;
    with_nfft(n_fft, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        if constexpr (fwd_here<PART>(N)) e = fwd_launch_n<V, N>(typename V::Modes{}, mode, tpw, p, grid, s);
    });
    return e;
}

template <class V, int PART> hipError_t fwd_set_attr_part()
{
    hipError_t e = hipSuccess;
    for (int n = kMinFastNfft; n <= kMaxFastNfft && e == hipSuccess; n *= 2)
        with_nfft(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            if constexpr (fwd_here<PART>(N)) e = fwd_set_attr_n<V, N>(typename V::Modes{});
        });
    return e;
}

template <class V> static hipError_t fwd_launch(int n_fft, int mode, int tpw, const typename V::Params& p, int grid, hipStream_t s)
{
    if constexpr (kFwdSplit) {
        switch (fwd_part_of(n_fft)) {
            case 1: return fwd_launch_part<V, 1>(n_fft, mode, tpw, p, grid, s);
            case 2: return fwd_launch_part<V, 2>(n_fft, mode, tpw, p, grid, s);
            case 3: return fwd_launch_part<V, 3>(n_fft, mode, tpw, p, grid, s);
        }
    }
    return fwd_launch_part<V, 0>(n_fft, mode, tpw, p, grid, s);
}

template <class V> static hipError_t fwd_set_attr()
{
    hipError_t e = fwd_set_attr_part<V, 0>();
    if constexpr (kFwdSplit) {
        if (e == hipSuccess) e = fwd_set_attr_part<V, 1>();
        if (e == hipSuccess) e = fwd_set_attr_part<V, 2>();
        if (e == hipSuccess) e = fwd_set_attr_part<V, 3>();
    }
    return e;
}

#define DMEL_FWD_PART_OF(LINKAGE, V, K) \
    LINKAGE template hipError_t fwd_launch_part<V, K>(int, int, int, const V::Params&, int, hipStream_t); \
    LINKAGE template hipError_t fwd_set_attr_part<V, K>();
// this part's two functions are instantiated here; in part 0 of a split build, those of parts 1 to 3 are declared as instantiated elsewhere
#if DMEL_FWD_PART != 0
#define DMEL_FWD_PARTS_OF(V) DMEL_FWD_PART_OF(, V, DMEL_FWD_PART)
#elif defined(DMEL_FWD_SPLIT) && !defined(DMEL_ONLY_NFFT)
#define DMEL_FWD_PARTS_OF(V) DMEL_FWD_PART_OF(, V, 0) DMEL_FWD_PART_OF(extern, V, 1) DMEL_FWD_PART_OF(extern, V, 2) DMEL_FWD_PART_OF(extern, V, 3)
#else
#define DMEL_FWD_PARTS_OF(V) DMEL_FWD_PART_OF(, V, 0)
#endif

}  // namespace dmel
