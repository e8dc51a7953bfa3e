// dmel_fwd_band_len.hip -- the fused forward of BandSplitMelSpectrogram over clips of per-clip lengths (dmel_forward_band*_lengths).
//
// dmel_fwd_band_len_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_MULTI = 1, DMEL_FWD_BAND = 1 and DMEL_FWD_LEN = 1:
// dmel_fwd_band_kernel's one (B, 1, M, T) image, channel c producing rows [e_c, e_c+1) only, over dmel_fwd_len_kernel's clips.  The pad rows of a
// tile past the clip and the NaN rows of an invalid length are confined to the channel's rows like every other store site; a pad tile returns
// before the contraction, so the band build's skipping of tiles / phases is untouched.  The rows' values are dmel_fwd_len_kernel's at lambd[c] to
// the bit.  Built for kTrain, kTrainW, kInfer, n_fft 32 ... 16384, one tile per workgroup, in a translation unit of its own (four parts, split as
// dmel_fwd.hip's: dmel_fwd_dispatch.h).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_MULTI 1
#define DMEL_FWD_BAND 1
#define DMEL_FWD_LEN 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_LEN
#undef DMEL_FWD_BAND
#undef DMEL_FWD_MULTI

// this file's variant (dmel_fwd_dispatch.h).  One tile per workgroup only (as dmel_fwd_len.hip)
struct FwdBandLenVariant {
    using Params = FwdBandLenParams;
    using Modes = FwdModes<kTrain, kTrainW, kInfer>;
    template <int N, int MODE, int TPW> static constexpr bool exists() { return TPW == 1 && (MODE != kTrainW || wlc_size(N)); }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdBandLenParams) = {dmel_fwd_band_len_kernel<N, MODE, TPW>};
    static int pick(const FwdBandLenParams&) { return 0; }
};
DMEL_FWD_PARTS_OF(FwdBandLenVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdBandLenParams& p, int grid, hipStream_t s) { return fwd_launch<FwdBandLenVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_band_len_prepare_attributes() { return fwd_set_attr<FwdBandLenVariant>(); }
#endif

}  // namespace dmel
