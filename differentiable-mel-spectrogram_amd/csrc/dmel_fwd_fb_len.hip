// dmel_fwd_fb_len.hip -- the fused forward over clips of per-clip lengths for a TRAINED filterbank (MelSpectrogramLayer(learnable_fb=True,
// lengths_learnable_fb=True).forward(x, lengths): dmel_forward_dev_fixed_lengths, dmel_backward_fb_dev_lengths).
//
// dmel_fwd_fb_len_kernel is csrc/dmel_fwd_body.inc compiled with DMEL_FWD_LEN = 1 (the clip bounds Lc / Tc of dmel_fwd_len.hip) and
// DMEL_FWD_FB = 1, in the three modes the HTK layer's length build does not have or cannot serve:
//   kTrainH   the dense contraction on the bf16 matrix pipe (DMEL_FLAG_MFMA_BF16X3), n_fft 64 ... 4096
//   kSpec     the recompute pass of the filterbank gradient: the power spectrogram (B, F, T) of clips of Lc samples, DC removed over the
//             clip (models.py:38), n_fft 32 ... 16384
//   kTrain    the exact contraction, also with FwdParams::spec_out (the spectrogram saved for the filterbank gradient), n_fft 32 ... 16384
// What DMEL_FWD_FB changes: for a length outside 1 ... L the clip's whole (F, T) spectrogram -- kSpec's output, kTrain / kTrainH's spec_out
// -- is NaN, and kSpec writes nothing in a pad tile (the gradient's GEMM never loads a column at or past Tc).  One tile per workgroup, four
// parts (dmel_fwd_dispatch.h).
#include "dmel_fwd_dispatch.h"

namespace dmel {

#include "dmel_fwd_log.h"
#define STAMP(i) do {} while (0)
#define STAMP_PLACE() do {} while (0)

#define DMEL_FWD_LEN 1
#define DMEL_FWD_FB 1
#include "dmel_fwd_body.inc"
#undef DMEL_FWD_FB
#undef DMEL_FWD_LEN

struct FwdFbLenVariant {
    using Params = FwdFbLenParams;
    using Modes = FwdModes<kTrain, kTrainH, kSpec>;
    template <int N, int MODE, int TPW> static constexpr bool exists() { return TPW == 1 && (MODE != kTrainH || (N >= kHsplitMinNfft && N <= kHsplitMaxNfft)); }
    template <int N, int MODE, int TPW> static constexpr void (*kernels[])(FwdFbLenParams) = {dmel_fwd_fb_len_kernel<N, MODE, TPW>};
    static int pick(const FwdFbLenParams&) { return 0; }
};
DMEL_FWD_PARTS_OF(FwdFbLenVariant)

#if DMEL_FWD_PART == 0
hipError_t launch_forward(int n_fft, int mode, int tpw, const FwdFbLenParams& p, int grid, hipStream_t s) { return fwd_launch<FwdFbLenVariant>(n_fft, mode, tpw, p, grid, s); }
hipError_t forward_fb_len_prepare_attributes() { return fwd_set_attr<FwdFbLenVariant>(); }
#endif

}  // namespace dmel
