"""The scalar forward's lambd tracking is the K = 1 case of the multi-window forward's: two plans, one driven through dmel_forward_dev, the other
through dmel_forward_multi_dev with one channel, follow the same lambd trajectory with the device synchronised after every call (each report has
landed before the host looks).  After every call dmel_plan_lambd_status and dmel_plan_lambd_status_channel(0) agree field by field and the two
outputs are equal bit for bit; an uncovered jump then fails loudly once on both, and both recover through a cold start.  No field differs
between the two forms on this trajectory (the differences the two keep -- a forced launch, the range a channel's guards are cut to -- lie
outside it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L, M, HOP, SR = 2, 2000, 16, 100, 16000
T = L // HOP + 1
FIELDS = ("known", "lambd_seen", "n_fft_seen", "seq_issued", "seq_seen", "rate", "guards", "next_n_fft", "next_guards", "error")


def test_scalar_and_one_channel_tracking_agree_call_by_call():
    from dmel_amd import capi
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    scalar, multi = capi.Plan(L, HOP, M, SR), capi.Plan(L, HOP, M, SR)
    try:                                                  # (the plans are released here, not by a later garbage collection inside another test's capture)
        lam = torch.zeros(1, dtype=torch.float32, device=DEV)
        out_s, out_m = torch.empty((B, 1, M, T), device=DEV), torch.empty((B, 1, M, T), device=DEV)
        scr_s = torch.zeros(scalar.scratch_bytes(B), dtype=torch.uint8, device=DEV)
        scr_m = torch.zeros(multi.scratch_bytes_multi(B, 1), dtype=torch.uint8, device=DEV)

        def call():
            out_s.fill_(7.0)
            out_m.fill_(9.0)
            scalar.forward_dev(x.data_ptr(), B, lam.data_ptr(), out_s.data_ptr(), None, True, 1e-10, s, scratch_ptr=scr_s.data_ptr())
            multi.forward_multi_dev(x.data_ptr(), B, lam.data_ptr(), 1, out_m.data_ptr(), None, True, 1e-10, s, scr_m.data_ptr())
            torch.cuda.synchronize()

        def statuses():
            a, b = scalar.lambd_status(), multi.lambd_status_channel(0)
            for k in FIELDS:
                assert a[k] == b[k], (k, a, b)
            return a

        # 12 calls from 10.0 rising by 0.08: 6 lambd crosses 64 and reaches 65 at the last, n_fft 64 -> 128, and the guard launch must cover it
        traj = (np.float32(10.0) + np.float32(0.08) * np.arange(12, dtype=np.float32)).astype(np.float32)
        seen_n = []
        for i, v in enumerate(traj):
            lam.fill_(float(v))
            call()
            st = statuses()
            assert st["known"] == 1 and st["error"] == 0 and st["seq_seen"] == i + 1 and st["seq_issued"] == i + 1, st
            assert st["lambd_seen"] == float(v) and st["n_fft_seen"] == capi.n_fft(float(v)), st
            assert torch.isfinite(out_s).all() and torch.equal(out_s, out_m), i
            seen_n.append(st["n_fft_seen"])
        assert seen_n[0] == 64 and seen_n[-1] == 128 and sorted(seen_n) == seen_n
        assert abs(statuses()["rate"] - 0.08) < 1e-4

        # one uncovered jump with the guards switched off on both plans: NaN by design and a host-visible word, no fault
        scalar.set_tracking(8, 2)
        multi.set_tracking(8, 2)
        lam.fill_(40.0)                                       # n_fft 256: no launch of the next call covers it
        call()
        assert torch.isnan(out_s).all() and torch.isnan(out_m).all()
        assert statuses()["error"] == 1
        for plan, fn in ((scalar, lambda: scalar.forward_dev(x.data_ptr(), B, lam.data_ptr(), out_s.data_ptr(), None, True, 1e-10, s, scratch_ptr=scr_s.data_ptr())),
                         (multi, lambda: multi.forward_multi_dev(x.data_ptr(), B, lam.data_ptr(), 1, out_m.data_ptr(), None, True, 1e-10, s, scr_m.data_ptr()))):
            with pytest.raises(capi.DmelError, match=r"status 6: .*lambd moved from"):
                fn()
        st = statuses()
        assert st["known"] == 0 and st["error"] == 0, st
        call()                                                # once only: this call goes through, by a cold start
        st = statuses()
        assert st["known"] == 1 and st["error"] == 0 and st["lambd_seen"] == 40.0 and st["n_fft_seen"] == 256, st
        assert torch.isfinite(out_s).all() and torch.equal(out_s, out_m)
    finally:
        scalar.close()
        multi.close()
