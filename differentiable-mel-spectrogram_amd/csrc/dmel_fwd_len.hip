// dmel_fwd_len.hip -- the fused forward over clips of per-clip lengths (MelSpectrogramLayer.forward(x, lengths), dmel_forward_*lengths).
//
// dmel_fwd_len_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_LEN = 1: every sample-space bound of the clip (the buffer resource,
// the interior / edge test, the load clamps, the window-multiply masks, the three clip sums and their quotient) is the clip's own length
// Lc = lengths[b] instead of n_points; the frames at or past Tc = Lc / hop + 1 are pad frames (zero mel power: 0, or the epilogue's own
// log(0 + eps); tangent 0), and a tile whose first frame is a pad frame writes its rows and skips the transform and the contraction.
// Built for the modes of the HTK layer (kTrain, kTrainW, kInfer), n_fft 32 ... 16384, in a translation unit of its own (four parts, split
// as dmel_fwd.hip's: dmel_fwd_dispatch.h).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_LEN 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_LEN

// this file's variant (dmel_fwd_dispatch.h).  One tile per workgroup only: the two-tile variants of dmel_fwd.hip spill here (<512, kTrain, 2>: 3 registers,
// 16 bytes of scratch)
struct FwdLenVariant {
    using Params = FwdLenParams;
    using Modes = FwdModes<kTrain, kTrainW, kInfer>;
    template <int N, int MODE, int TPW> static constexpr bool exists() { return TPW == 1 && (MODE != kTrainW || wlc_size(N)); }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdLenParams) = {dmel_fwd_len_kernel<N, MODE, TPW>};
    static int pick(const FwdLenParams&) { return 0; }
};
DMEL_FWD_PARTS_OF(FwdLenVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdLenParams& p, int grid, hipStream_t s) { return fwd_launch<FwdLenVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_len_prepare_attributes() { return fwd_set_attr<FwdLenVariant>(); }
#endif

}  // namespace dmel
