// dmel_fwd_multi_len.hip -- the fused forward of MultiWindowMelSpectrogram over clips of per-clip lengths (dmel_forward_multi*_lengths).
//
// dmel_fwd_multi_len_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_MULTI = 1 and DMEL_FWD_LEN = 1: the multi-window kernel's channel
// addressing (channel slot from the relabelled workgroup index, lam_for_channel, the channel's window table, lambd words and output rows) over
// dmel_fwd_len_kernel's clips -- every sample-space bound is the clip's own length Lc = lengths[b], the frames from Tc = Lc / hop + 1 on are pad
// frames, and a tile whose first frame is one writes the CHANNEL's rows of it and transforms nothing.  Channel k of the output is
// dmel_fwd_len_kernel's image at lambd[k] to the bit.  Built for kTrain, kTrainW, kInfer, n_fft 32 ... 16384, one tile per workgroup, in a
// translation unit of its own (four parts, split as dmel_fwd.hip's: dmel_fwd_dispatch.h).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_MULTI 1
#define DMEL_FWD_LEN 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_LEN
#undef DMEL_FWD_MULTI

// this file's variant (dmel_fwd_dispatch.h).  One tile per workgroup only (as dmel_fwd_len.hip)
struct FwdMultiLenVariant {
    using Params = FwdMultiLenParams;
    using Modes = FwdModes<kTrain, kTrainW, kInfer>;
    template <int N, int MODE, int TPW> static constexpr bool exists() { return TPW == 1 && (MODE != kTrainW || wlc_size(N)); }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdMultiLenParams) = {dmel_fwd_multi_len_kernel<N, MODE, TPW>};
    static int pick(const FwdMultiLenParams&) { return 0; }
};
DMEL_FWD_PARTS_OF(FwdMultiLenVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdMultiLenParams& p, int grid, hipStream_t s) { return fwd_launch<FwdMultiLenVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_multi_len_prepare_attributes() { return fwd_set_attr<FwdMultiLenVariant>(); }
#endif

}  // namespace dmel
