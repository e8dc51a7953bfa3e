// dmel_fwd_band.hip -- the fused forward of BandSplitMelSpectrogram (dmel_forward_band*): K window widths inside ONE (B, 1, M, T) image.
//
// dmel_fwd_band_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_MULTI = 1 and DMEL_FWD_BAND = 1: the multi-window kernel's channel
// addressing (channel slot from the relabelled workgroup index, lam_for_channel, the channel's window table and lambd words), but the clip's
// output base is the one-channel image's and channel c produces rows [e_c, e_c+1) only (FwdBandParams::band_edges).  The rows' values are the
// scalar kernel's to the bit: a row's products are accumulated exactly as there; what changes is which tiles / phases run and which rows are
// stored -- a banded 16 x 16 x 4 tile (or a piece of one) none of whose bands is the channel's is not contracted, a wave-local phase none of
// whose quads holds one runs no steps, and the result rows, the staged rows, the NaN rows of an uncovered channel and the bf16 stores are
// confined to the range.  Built for kTrain, kTrainW, kInfer, n_fft 32 ... 16384, one tile per workgroup, in a translation unit of its own
// (four parts, split as dmel_fwd.hip's: dmel_fwd_dispatch.h).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_MULTI 1
#define DMEL_FWD_BAND 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_BAND
#undef DMEL_FWD_MULTI

// this file's variant (dmel_fwd_dispatch.h).  One tile per workgroup only (as dmel_fwd_len.hip)
struct FwdBandVariant {
    using Params = FwdBandParams;
    using Modes = FwdModes<kTrain, kTrainW, kInfer>;
    template <int N, int MODE, int TPW> static constexpr bool exists() { return TPW == 1 && (MODE != kTrainW || wlc_size(N)); }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdBandParams) = {dmel_fwd_band_kernel<N, MODE, TPW>};
    static int pick(const FwdBandParams&) { return 0; }
};
DMEL_FWD_PARTS_OF(FwdBandVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdBandParams& p, int grid, hipStream_t s) { return fwd_launch<FwdBandVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_band_prepare_attributes() { return fwd_set_attr<FwdBandVariant>(); }
#endif

}  // namespace dmel
