"""ctypes binding of libdmel_hip.so (include/dmel.h).

This is the only way the Python layer reaches the kernels: raw device pointers, sizes and a
stream handle go through the C ABI.  There is no CPU fallback: if the shared object is missing or
no gfx950 device is visible, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DMEL_LIB") or os.path.join(_PKG_DIR, "libdmel_hip.so")   # DMEL_LIB: diagnostic builds (tools/stamps.py)

DMEL_OK = 0
DMEL_ERR_INVALID_ARGUMENT = 1
DMEL_ERR_UNSUPPORTED = 2
DMEL_ERR_HIP = 3
DMEL_ERR_NO_DEVICE = 4
DMEL_ERR_OUT_OF_MEMORY = 5
DMEL_ERR_LAMBD_TRACKING = 6
DMEL_ERR_MAILBOX_TIMEOUT = 7
DMEL_FLAG_MFMA_BF16X3 = 8
DMEL_FLAG_CHECK_NFFT = 16
DMEL_FLAG_X_INDIRECT = 32
DMEL_FLAG_LOG = 1
DMEL_FLAG_FULL_WINDOW = 2
DMEL_FLAG_OUT_BF16 = 4
DMEL_DTYPE_F32, DMEL_DTYPE_BF16 = 0, 1
MAX_NFFT = 16384          # largest transform of the HIP kernels (kMaxNfft in csrc/dmel_kernels.h)
MIN_FAST_NFFT = 32        # smallest transform of the fused kernel (kMinFastNfft); the multi-window layer serves MIN_FAST_NFFT ... MAX_NFFT

TORCH_LIB_PATH = os.path.join(_PKG_DIR, "libdmel_torch.so")


class DmelConfig(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("hop_length", C.c_int32), ("n_mels", C.c_int32),
                ("sample_rate", C.c_int32), ("f_min", C.c_double), ("f_max", C.c_double),
                ("normalize_window", C.c_int32), ("max_batch", C.c_int32)]


class DmelPlanInfo(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("n_freqs", C.c_int32), ("n_time", C.c_int32),
                ("frames_per_tile", C.c_int32), ("grid_fwd", C.c_int32), ("fb_blocks", C.c_int32),
                ("fb_blocks_dense", C.c_int32), ("lds_bytes", C.c_int32), ("kernel_path", C.c_int32),
                ("contraction", C.c_int32), ("wl_steps", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class DmelLambdStatus(C.Structure):
    _fields_ = [("known", C.c_int32), ("lambd_seen", C.c_float), ("n_fft_seen", C.c_int32), ("seq_issued", C.c_uint32),
                ("seq_seen", C.c_uint32), ("rate", C.c_float), ("guards", C.c_int32), ("error", C.c_int32),
                ("error_seq", C.c_uint32), ("error_lambd", C.c_float), ("next_n_fft", C.c_int32), ("next_guards", C.c_int32),
                ("calls", C.c_uint32)]


class DmelProfile(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("fwd_ms", C.c_double), ("bwd_ms", C.c_double),
                ("prep_launches", C.c_int32), ("fwd_launches", C.c_int32), ("bwd_launches", C.c_int32)]


class DmelError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libdmel_hip: status {status}: {message}")
        self.status = status


# name -> (restype, argtypes) of every function include/dmel.h declares, in the header's order.  The header is the authority: tests compare the
# names and the parameter counts with it and the library's exports with the names.  ``vp`` is any device or opaque pointer (an int, None or a
# ctypes array), the typed pointers are host arrays and out-parameters, ``buf`` a byte buffer (uint8_t[]), ``status`` the dmel_status enum.
P = C.POINTER
vp, vpp, fp, i32p, u32p, buf = C.c_void_p, P(C.c_void_p), P(C.c_float), P(C.c_int32), P(C.c_uint32), C.c_char_p
status, i32, u32, i64, u64, f32, f64 = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
_SIGNATURES = {
    "dmel_abi_version": (i32, []),
    "dmel_n_fft": (i32, [f32]),
    "dmel_window_host": (status, [f32, i32, i32, fp, fp]),
    "dmel_mel_fbanks_host": (status, [i32, f64, f64, i32, i32, fp]),
    "dmel_contraction_partition_host": (status, [i32p, i32, i32, i32p, i32p, i32p, i32p, i32p, i32p]),
    "dmel_last_error": (C.c_char_p, []),
    "dmel_device_count": (i32, []),
    "dmel_plan_create": (status, [P(DmelConfig), vpp]),
    "dmel_plan_destroy": (status, [vp]),
    "dmel_plan_retain": (status, [vp]),
    "dmel_plan_release": (status, [vp]),
    "dmel_plan_is_live": (i32, [vp]),
    "dmel_lambd_ring_size": (i32, []),
    "dmel_plan_get_config": (status, [vp, P(DmelConfig)]),
    "dmel_plan_set_filterbank": (status, [vp, i32, fp]),
    "dmel_plan_set_filterbank_dev": (status, [vp, i32, vp, vp]),
    "dmel_forward": (status, [vp, vp, i32, f32, u32, f64, vp, vp, vp]),
    "dmel_scratch_bytes": (C.c_size_t, [vp, i32]),
    "dmel_forward_scratch": (status, [vp, vp, i32, f32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_dev": (status, [vp, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_dev_fixed": (status, [vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_dev_fixed_spec": (status, [vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp, vp]),
    "dmel_forward_lengths": (status, [vp, vp, vp, i32, f32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_dev_lengths": (status, [vp, vp, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_dev_fixed_lengths": (status, [vp, vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp, vp]),
    "dmel_plan_lambd_status": (status, [vp, P(DmelLambdStatus)]),
    "dmel_plan_lambd_report": (status, [vp, u32, fp, i32p]),
    "dmel_decide_launch": (status, [f32, f32, f32, i32p, i32p]),
    "dmel_plan_force_launch": (status, [vp, i32, i32]),
    "dmel_plan_set_tracking": (status, [vp, i32, i32]),
    "dmel_plan_lambd_reset": (status, [vp]),
    "dmel_backward": (status, [vp, vp, vp, i64, i32, vp, vp]),
    "dmel_backward_ex": (status, [vp, vp, i32, vp, i64, i32, vp, vp]),
    "dmel_backward_scratch": (status, [vp, vp, i32, vp, i64, i32, vp, vp, vp]),
    "dmel_backward_fb": (status, [vp, vp, i32, f32, u32, vp, vp, vp, vp]),
    "dmel_backward_fb_dev": (status, [vp, vp, i32, vp, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_fb_saved": (status, [vp, vp, i32, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_fb_saved_dl": (status, [vp, vp, i32, i32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "dmel_backward_fb_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_fb_saved_lengths": (status, [vp, vp, vp, i32, i32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "dmel_backward_x": (status, [vp, vp, i32, f32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_spec": (status, [vp, vp, i32, f32, i32, u32, vp, vp, vp]),
    "dmel_backward_x_dev": (status, [vp, vp, i32, vp, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_spec_dev": (status, [vp, vp, i32, vp, i32, u32, vp, vp, vp]),
    "dmel_backward_x_lengths": (status, [vp, vp, vp, i32, f32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, u32, vp, vp, vp, vp]),
    "dmel_spectrogram": (status, [vp, vp, i32, f32, i32, vp, vp]),
    "dmel_spectrogram_ex": (status, [vp, vp, i32, f32, i32, u32, vp, vp, vp]),
    "dmel_spectrogram_ex_dev": (status, [vp, vp, i32, vp, i32, u32, vp, vp, vp]),
    "dmel_comm_unique_id": (status, [buf]),
    "dmel_comm_create": (status, [buf, i32, i32, vpp]),
    "dmel_comm_destroy": (status, [vp]),
    "dmel_comm_allreduce_async": (status, [vp, vp, i32, vp, i32p]),
    "dmel_comm_allreduce": (status, [vp, vp, i32, vp]),
    "dmel_comm_wait": (status, [vp, i32, vp]),
    "dmel_mailbox_create": (status, [i32, i32, vpp, buf]),
    "dmel_mailbox_connect": (status, [vp, buf]),
    "dmel_mailbox_destroy": (status, [vp]),
    "dmel_mailbox_allreduce": (status, [vp, vp, vp]),
    "dmel_mailbox_error": (status, [vp, i32p, u32p, i32p]),
    "dmel_mailbox_set_spin_limit": (status, [vp, u32]),
    "dmel_mailbox_set_timeout_ms": (status, [vp, u64]),
    "dmel_plan_attach_mailbox": (status, [vp, vp]),
    "dmel_adam_step": (status, [vp, vp, vp, vp, vp, vp, i64, f64, f64, f64, f64, f64, i32, vp]),
    "dmel_plan_attach_adam": (status, [vp, vp, vp, vp, vp, f64, f64, f64, f64, f64, i32]),
    "dmel_pcen_scratch_bytes": (C.c_size_t, [i64]),
    "dmel_pcen_forward": (status, [vp, i64, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp]),
    "dmel_pcen_backward": (status, [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp]),
    "dmel_bandnorm_scratch_bytes": (C.c_size_t, [i64, i32]),
    "dmel_bandnorm_forward": (status, [vp, i64, i32, i64, i32, vp, vp, vp, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, vp]),
    "dmel_bandnorm_backward": (status, [vp, vp, vp, i64, i32, i64, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "dmel_specmask_draw": (status, [i64, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp]),
    "dmel_specmask_apply": (status, [vp, i64, i32, i64, i32, vp, vp, i32, i32, i32, f32, vp, vp]),
    "dmel_deltas_forward": (status, [vp, i64, i64, i32, vp, i32, i32, i32, vp, vp]),
    "dmel_deltas_backward": (status, [vp, i64, i64, i32, vp, i32, i32, i32, vp, vp]),
    "dmel_statspool_forward": (status, [vp, i64, i64, i32, vp, i32, f64, vp, vp, vp, vp]),
    "dmel_statspool_backward": (status, [vp, vp, vp, vp, i64, i64, i32, vp, i32, vp, vp]),
    "dmel_attnpool_forward": (status, [vp, vp, i64, i64, i64, i32, vp, i32, f64, vp, vp, vp, vp]),
    "dmel_attnpool_backward": (status, [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp, i32, f64, vp, vp, vp]),
    "dmel_scratch_bytes_multi": (C.c_size_t, [vp, i32, i32]),
    "dmel_forward_multi": (status, [vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_multi_dev": (status, [vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_multi_lengths": (status, [vp, vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_multi_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, u32, f64, vp, vp, vp, vp]),
    "dmel_backward_multi": (status, [vp, vp, i32, vp, i32, i32, i32, vp, vp, vp]),
    "dmel_plan_lambd_status_channel": (status, [vp, i32, P(DmelLambdStatus)]),
    "dmel_decide_launch_multi": (status, [fp, fp, i32, f32, i32p, u32p, i32p]),
    "dmel_backward_x_multi": (status, [vp, vp, i32, fp, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_multi_dev": (status, [vp, vp, i32, vp, i32, i32p, u32p, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_multi_lengths": (status, [vp, vp, vp, i32, fp, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_multi_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, i32p, u32p, i32, u32, vp, vp, vp, vp]),
    "dmel_plan_last_multi_launch": (status, [vp, i32p, u32p, i32p]),
    "dmel_forward_band": (status, [vp, vp, i32, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_band_dev": (status, [vp, vp, i32, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_band_lengths": (status, [vp, vp, vp, i32, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_forward_band_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, vp, u32, f64, vp, vp, vp, vp]),
    "dmel_backward_band": (status, [vp, vp, i32, vp, i32, i32, vp, i32, vp, vp, vp]),
    "dmel_backward_x_band": (status, [vp, vp, i32, fp, i32, vp, u32, vp, vp, vp, vp]),
    "dmel_backward_x_band_dev": (status, [vp, vp, i32, vp, i32, vp, i32p, u32p, i32, u32, vp, vp, vp, vp]),
    "dmel_backward_x_band_lengths": (status, [vp, vp, vp, i32, fp, i32, vp, u32, vp, vp, vp, vp]),
    "dmel_backward_x_band_dev_lengths": (status, [vp, vp, vp, i32, vp, i32, vp, i32p, u32p, i32, u32, vp, vp, vp, vp]),
    "dmel_plan_get_info": (status, [vp, P(DmelPlanInfo)]),
    "dmel_plan_set_profiling": (status, [vp, i32]),
    "dmel_plan_get_profile": (status, [vp, P(DmelProfile)]),
}
SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load():
    """dlopen libdmel_hip.so.  Raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python differentiable-mel-spectrogram_amd/build.py). "
            "There is no CPU fallback for the DMEL layer.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


_torch_ops = None


def torch_ops():
    """The torch-registered ops (TORCH_LIBRARY(dmel, ...), csrc/dmel_torch.cpp): ``torch.ops.dmel``.  Loads libdmel_torch.so
    (and through it libdmel_hip.so) on first use; raises if it has not been built."""
    global _torch_ops
    if _torch_ops is None:
        import torch
        load()
        if not os.path.exists(TORCH_LIB_PATH):
            raise RuntimeError(f"{TORCH_LIB_PATH} is missing: build it first (python differentiable-mel-spectrogram_amd/build.py). "
                               "There is no CPU fallback for the DMEL layer.")
        torch.ops.load_library(TORCH_LIB_PATH)
        _torch_ops = torch.ops.dmel
    return _torch_ops


def _check(status: int):
    if status != DMEL_OK:
        raise DmelError(status, (load().dmel_last_error() or b"").decode("utf-8", "replace"))


def release_handle(handle: int) -> None:
    """dmel_plan_release of a handle obtained from ``Plan.retain``"""
    if handle:
        load().dmel_plan_release(C.c_void_p(int(handle)))


def lambd_ring_size() -> int:
    return int(load().dmel_lambd_ring_size())


def n_fft(lambd: float) -> int:
    return int(load().dmel_n_fft(C.c_float(float(lambd))))


def decide_launch(lambd: float, rate: float, stale_forwards: float) -> tuple[int, int]:
    """(n_fft, guards) a forward must be launched for when lambd may move by ``rate`` per forward for ``stale_forwards`` forwards
    unobserved (dmel_decide_launch: a pure function, no device)."""
    n, g = C.c_int32(0), C.c_int32(0)
    _check(load().dmel_decide_launch(C.c_float(float(lambd)), C.c_float(float(rate)), C.c_float(float(stale_forwards)), C.byref(n), C.byref(g)))
    return int(n.value), int(g.value)


def decide_launch_multi(lambds, rates, stale_forwards: float) -> list[tuple[int, int]]:
    """[(n_fft, channel mask), ...] in ascending n_fft: the union over channels of decide_launch (dmel_decide_launch_multi)."""
    k = len(lambds)
    lam = (C.c_float * max(k, 1))(*[float(v) for v in lambds])
    rate = (C.c_float * max(k, 1))(*[float(v) for v in rates])
    ns, masks, cnt = (C.c_int32 * (3 * max(k, 1)))(), (C.c_uint32 * (3 * max(k, 1)))(), C.c_int32(0)
    _check(load().dmel_decide_launch_multi(lam, rate, k, C.c_float(float(stale_forwards)), ns, masks, C.byref(cnt)))
    return [(int(ns[i]), int(masks[i])) for i in range(cnt.value)]


def adam_step(param_ptr: int, grad_ptr: int, exp_avg_ptr: int, exp_avg_sq_ptr: int, step_ptr: int, ticket_ptr: int, n: int, lr: float,
              beta1: float, beta2: float, eps: float, weight_decay: float, maximize: bool, stream: int) -> None:
    """dmel_adam_step: torch.optim.Adam's update of an fp32 parameter as one launch on ``stream`` (device pointers; ``ticket_ptr``
    = one zeroed device word, may be 0 up to 1024 elements)."""
    _check(load().dmel_adam_step(param_ptr, grad_ptr, exp_avg_ptr, exp_avg_sq_ptr, step_ptr, ticket_ptr or None, int(n), C.c_double(float(lr)),
                                 C.c_double(float(beta1)), C.c_double(float(beta2)), C.c_double(float(eps)), C.c_double(float(weight_decay)),
                                 1 if maximize else 0, stream))


def pcen_scratch_bytes(rows: int) -> int:
    """dmel_pcen_scratch_bytes: what pcen_backward needs for the parameter gradients (a pure function, no device)"""
    return int(load().dmel_pcen_scratch_bytes(int(rows)))


def pcen_forward(e_ptr: int, rows: int, n_mels: int, n_time: int, alpha_ptr: int, delta_ptr: int, r_ptr: int, s_ptr: int, eps: float,
                 y_ptr: int, m_ptr: int | None, stream: int) -> None:
    """dmel_pcen_forward: y (and the smoother M, when ``m_ptr`` is given) of ``rows`` x ``n_time`` fp32 linear mel power, band = row % n_mels"""
    _check(load().dmel_pcen_forward(e_ptr, int(rows), int(n_mels), int(n_time), alpha_ptr, delta_ptr, r_ptr, s_ptr, C.c_float(float(eps)),
                                    y_ptr, m_ptr or None, stream))


def pcen_backward(g_ptr: int, e_ptr: int, m_ptr: int, rows: int, n_mels: int, n_time: int, alpha_ptr: int, delta_ptr: int, r_ptr: int, s_ptr: int,
                  eps: float, de_ptr: int | None, dparams_ptr: int | None, scratch_ptr: int | None, stream: int) -> None:
    """dmel_pcen_backward: dE and / or the (4, n_mels) gradients of alpha, delta, r, s (``scratch_ptr``: pcen_scratch_bytes(rows) bytes)"""
    _check(load().dmel_pcen_backward(g_ptr, e_ptr, m_ptr, int(rows), int(n_mels), int(n_time), alpha_ptr, delta_ptr, r_ptr, s_ptr,
                                     C.c_float(float(eps)), de_ptr or None, dparams_ptr or None, scratch_ptr or None, stream))


def bandnorm_scratch_bytes(rows: int, n_mels: int) -> int:
    """dmel_bandnorm_scratch_bytes: what bandnorm_backward (and the training forward of the batch statistics) needs (a pure function, no device)"""
    return int(load().dmel_bandnorm_scratch_bytes(int(rows), int(n_mels)))


def bandnorm_forward(s_ptr: int, rows: int, n_mels: int, rows_per_clip: int, n_time: int, lengths_ptr: int | None, weight_ptr: int | None,
                     bias_ptr: int | None, batch_stats: bool, training: bool, eps: float, momentum: float, running_mean_ptr: int | None,
                     running_var_ptr: int | None, num_batches_tracked_ptr: int | None, y_ptr: int, stats_ptr: int, scratch_ptr: int | None,
                     stream: int) -> None:
    """dmel_bandnorm_forward: y and the fp64 (mu, rstd) pairs of ``rows`` x ``n_time`` fp32 frames, band = row % n_mels,
    clip = row // rows_per_clip, valid frames t < lengths[clip] (int32 on the device; None: all)"""
    _check(load().dmel_bandnorm_forward(s_ptr, int(rows), int(n_mels), int(rows_per_clip), int(n_time), lengths_ptr or None, weight_ptr or None,
                                        bias_ptr or None, int(bool(batch_stats)), int(bool(training)), C.c_double(float(eps)),
                                        C.c_double(float(momentum)), running_mean_ptr or None, running_var_ptr or None,
                                        num_batches_tracked_ptr or None, y_ptr, stats_ptr, scratch_ptr or None, stream))


def bandnorm_backward(g_ptr: int, s_ptr: int, stats_ptr: int, rows: int, n_mels: int, rows_per_clip: int, n_time: int, lengths_ptr: int | None,
                      weight_ptr: int | None, batch_stats: bool, training: bool, ds_ptr: int | None, dweight_ptr: int | None,
                      dbias_ptr: int | None, scratch_ptr: int, stream: int) -> None:
    """dmel_bandnorm_backward: ds and / or the (n_mels,) gradients of weight and bias (``scratch_ptr``: bandnorm_scratch_bytes(rows, n_mels) bytes)"""
    _check(load().dmel_bandnorm_backward(g_ptr, s_ptr, stats_ptr, int(rows), int(n_mels), int(rows_per_clip), int(n_time), lengths_ptr or None,
                                         weight_ptr or None, int(bool(batch_stats)), int(bool(training)), ds_ptr or None, dweight_ptr or None,
                                         dbias_ptr or None, scratch_ptr, stream))


def specmask_draw(images: int, channels: int, n_mels: int, n_time_frames: int, lengths_ptr: int | None, time_param: int, time_permille: int,
                  n_time: int, freq_param: int, n_freq: int, rng_state_ptr: int, advance: bool, stripes_ptr: int | None, stream: int) -> None:
    """dmel_specmask_draw: the (images, n_time + n_freq, 2) int32 table of [lo, hi) stripe pairs from the device words
    ``rng_state`` = (seed, calls); ``advance`` stores calls + 1 behind the draw"""
    _check(load().dmel_specmask_draw(int(images), int(channels), int(n_mels), int(n_time_frames), lengths_ptr or None, int(time_param),
                                     int(time_permille), int(n_time), int(freq_param), int(n_freq), rng_state_ptr or None, int(bool(advance)),
                                     stripes_ptr or None, stream))


def specmask_apply(s_ptr: int, rows: int, n_mels: int, rows_per_clip: int, n_time_frames: int, lengths_ptr: int | None, stripes_ptr: int | None,
                   n_time: int, n_freq: int, elem_bf16: bool, fill: float, y_ptr: int, stream: int) -> None:
    """dmel_specmask_apply: y = fill under the table's stripes on valid frames, s's bits elsewhere (``rows`` x ``n_time_frames`` fp32 or bf16
    elements); the backward is the same call on the cotangent with fill 0"""
    _check(load().dmel_specmask_apply(s_ptr or None, int(rows), int(n_mels), int(rows_per_clip), int(n_time_frames), lengths_ptr or None,
                                      stripes_ptr or None, int(n_time), int(n_freq), int(bool(elem_bf16)), C.c_float(float(fill)), y_ptr or None,
                                      stream))


def deltas_forward(s_ptr: int, rows: int, rows_per_clip: int, n_time_frames: int, lengths_ptr: int | None, win_length: int, order: int,
                   include_static: bool, y_ptr: int, stream: int) -> None:
    """dmel_deltas_forward: y = the groups [s,] d[, dd] of ``rows`` x ``n_time_frames`` fp32 values, the stencil's edge at each clip's own
    last valid frame"""
    _check(load().dmel_deltas_forward(s_ptr or None, int(rows), int(rows_per_clip), int(n_time_frames), lengths_ptr or None, int(win_length),
                                      int(order), int(bool(include_static)), y_ptr or None, stream))


def deltas_backward(g_ptr: int, rows: int, rows_per_clip: int, n_time_frames: int, lengths_ptr: int | None, win_length: int, order: int,
                    include_static: bool, ds_ptr: int, stream: int) -> None:
    """dmel_deltas_backward: ds = g_static + D^T (g_d + D^T g_dd) from the cotangent of dmel_deltas_forward's y"""
    _check(load().dmel_deltas_backward(g_ptr or None, int(rows), int(rows_per_clip), int(n_time_frames), lengths_ptr or None, int(win_length),
                                       int(order), int(bool(include_static)), ds_ptr or None, stream))


STATSPOOL_MEAN, STATSPOOL_STD, STATSPOOL_MAX = 1, 2, 4


def statspool_forward(s_ptr: int, rows: int, rows_per_clip: int, n_time_frames: int, lengths_ptr: int | None, which: int, eps: float,
                      y_ptr: int, stats_ptr: int | None, argmax_ptr: int | None, stream: int) -> None:
    """dmel_statspool_forward: y = the groups [mean][, std][, max] (``which``: bits 1, 2, 4) of ``rows`` x ``n_time_frames`` fp32 values over
    each clip's own valid frames; ``stats_ptr`` (2 * rows doubles) and ``argmax_ptr`` (rows int32) are what the backward reads"""
    _check(load().dmel_statspool_forward(s_ptr or None, int(rows), int(rows_per_clip), int(n_time_frames), lengths_ptr or None, int(which),
                                         C.c_double(float(eps)), y_ptr or None, stats_ptr or None, argmax_ptr or None, stream))


def statspool_backward(g_ptr: int, s_ptr: int | None, stats_ptr: int | None, argmax_ptr: int | None, rows: int, rows_per_clip: int,
                       n_time_frames: int, lengths_ptr: int | None, which: int, ds_ptr: int, stream: int) -> None:
    """dmel_statspool_backward: ds = g_mean / Tc + g_std (s - mu) / (Tc sd) + [t == am] g_max from the cotangent of dmel_statspool_forward's y"""
    _check(load().dmel_statspool_backward(g_ptr or None, s_ptr or None, stats_ptr or None, argmax_ptr or None, int(rows), int(rows_per_clip),
                                          int(n_time_frames), lengths_ptr or None, int(which), ds_ptr or None, stream))


ATTNPOOL_MEAN, ATTNPOOL_STD = 1, 2


def attnpool_forward(s_ptr: int, a_ptr: int, rows: int, rows_per_clip: int, logit_rows_per_clip: int, n_time_frames: int,
                     lengths_ptr: int | None, which: int, eps: float, y_ptr: int, stats_ptr: int | None, norm_ptr: int | None, stream: int) -> None:
    """dmel_attnpool_forward: y = the groups [mean][, std] (``which``: bits 1, 2) of ``rows`` x ``n_time_frames`` fp32 values under the softmax
    of each clip's ``logit_rows_per_clip`` logit rows over its own valid frames; ``stats_ptr`` (2 * rows doubles: mu, var) and ``norm_ptr``
    (2 doubles per logit row: m, Z) are what the backward reads"""
    _check(load().dmel_attnpool_forward(s_ptr or None, a_ptr or None, int(rows), int(rows_per_clip), int(logit_rows_per_clip), int(n_time_frames),
                                        lengths_ptr or None, int(which), C.c_double(float(eps)), y_ptr or None, stats_ptr or None,
                                        norm_ptr or None, stream))


def attnpool_backward(g_ptr: int, s_ptr: int, a_ptr: int, stats_ptr: int, norm_ptr: int, rows: int, rows_per_clip: int,
                      logit_rows_per_clip: int, n_time_frames: int, lengths_ptr: int | None, which: int, eps: float, ds_ptr: int, da_ptr: int,
                      stream: int) -> None:
    """dmel_attnpool_backward: ds = w (g_mean + g_std d / sd) and da = w sum_r (g_mean d + g_std (d^2 - var) / (2 sd)), d = s - mu, from the
    cotangent of dmel_attnpool_forward's y and the pairs it stored (``eps``: the forward's)"""
    _check(load().dmel_attnpool_backward(g_ptr or None, s_ptr or None, a_ptr or None, stats_ptr or None, norm_ptr or None, int(rows),
                                         int(rows_per_clip), int(logit_rows_per_clip), int(n_time_frames), lengths_ptr or None, int(which),
                                         C.c_double(float(eps)), ds_ptr or None, da_ptr or None, stream))


def device_count() -> int:
    return int(load().dmel_device_count())


def window_host(lambd: float, n: int, normalize: bool = False):
    import numpy as np
    w = np.empty(n, np.float32)
    dw = np.empty(n, np.float32)
    _check(load().dmel_window_host(float(lambd), n, int(normalize), w.ctypes.data_as(C.POINTER(C.c_float)),
                                   dw.ctypes.data_as(C.POINTER(C.c_float))))
    return w, dw


def contraction_partition(units, waves: int = 8):
    """dmel_contraction_partition_host: (own[waves], [(wave, tile, first, units), ...]) for one group of mel tiles"""
    L = load()
    i32 = C.c_int32
    n = len(units)
    u = (i32 * 8)(*([int(v) for v in units] + [0] * (8 - n)))
    own, npc = (i32 * 8)(), i32(0)
    pw, pt, pf, pu = (i32 * 8)(), (i32 * 8)(), (i32 * 8)(), (i32 * 8)()
    _check(L.dmel_contraction_partition_host(u, n, int(waves), own, C.byref(npc), pw, pt, pf, pu))
    return list(own)[:waves], [(pw[i], pt[i], pf[i], pu[i]) for i in range(npc.value)]


def mel_fbanks_host(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int):
    import numpy as np
    fb = np.empty((n_freqs, n_mels), np.float32)
    _check(load().dmel_mel_fbanks_host(n_freqs, float(f_min), float(f_max), n_mels, sample_rate,
                                       fb.ctypes.data_as(C.POINTER(C.c_float))))
    return fb


def _floats(values):
    """a host array of C floats (the K window widths passed by value)"""
    return (C.c_float * len(values))(*[float(v) for v in values])


def _ints(values):
    """a host array of int32 (the K + 1 band edges)"""
    return (C.c_int32 * len(values))(*[int(v) for v in values])


class Plan:
    """Owner of a dmel_plan handle (MelSpectrogramLayer.__init__ state, models.py:15-30)."""

    def __init__(self, n_points: int, hop_length: int, n_mels: int, sample_rate: int, f_min: float = 0.0,
                 f_max: float | None = None, normalize_window: bool = False, max_batch: int = 0):
        self._h = C.c_void_p()
        cfg = DmelConfig(int(n_points), int(hop_length), int(n_mels), int(sample_rate), float(f_min),
                         -1.0 if f_max is None else float(f_max), int(bool(normalize_window)), int(max_batch))
        _check(load().dmel_plan_create(C.byref(cfg), C.byref(self._h)))
        self.n_time = int(n_points) // int(hop_length) + 1
        self.n_mels = int(n_mels)
        self.n_points = int(n_points)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().dmel_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def retain(self) -> int:
        """dmel_plan_retain: one more reference; returns the raw handle to give to ``release_handle`` later (it stays valid after
        this wrapper is gone: what a captured HIP graph needs)"""
        _check(load().dmel_plan_retain(self._h))
        return int(self._h.value)

    def is_live(self) -> bool:
        return bool(self._h.value) and bool(load().dmel_plan_is_live(self._h))

    def __deepcopy__(self, memo):
        raise TypeError("a dmel plan is a cache of device tables bound to one GPU: copy the layer, not the plan")

    def __reduce__(self):
        raise TypeError("a dmel plan is a cache of device tables bound to one GPU and cannot be pickled; the layers drop "
                        "their plans when copied or pickled and rebuild them on first use")

    def forward(self, x_ptr: int, batch: int, lambd: float, out_ptr: int, tangent_ptr: int | None,
                log: bool, eps: float, stream: int, extra_flags: int = 0):
        _check(load().dmel_forward(self._h, x_ptr, batch, C.c_float(float(lambd)),
                                   (DMEL_FLAG_LOG if log else 0) | int(extra_flags), float(eps), out_ptr, tangent_ptr, stream))

    @property
    def handle(self) -> int:
        """The dmel_plan* as an integer (what the torch ops take)."""
        return int(self._h.value or 0)

    def scratch_bytes(self, batch: int) -> int:
        return int(load().dmel_scratch_bytes(self._h, int(batch)))

    def forward_dev(self, x_ptr: int, batch: int, lambd_ptr: int, out_ptr: int, tangent_ptr: int | None, log: bool, eps: float,
                    stream: int, scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_dev: lambd stays on the device (no host read)."""
        _check(load().dmel_forward_dev(self._h, x_ptr, batch, lambd_ptr, (DMEL_FLAG_LOG if log else 0) | int(extra_flags), float(eps),
                                       out_ptr, tangent_ptr, scratch_ptr, stream))

    def forward_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd: float, out_ptr: int, tangent_ptr: int | None, log: bool,
                        eps: float, stream: int, scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_lengths: clips ``x[b, :lengths[b]]`` (int32 lengths on the device), lambd by value."""
        _check(load().dmel_forward_lengths(self._h, x_ptr, lengths_ptr, batch, C.c_float(float(lambd)),
                                           (DMEL_FLAG_LOG if log else 0) | int(extra_flags), float(eps), out_ptr, tangent_ptr, scratch_ptr, stream))

    def forward_dev_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd_ptr: int, out_ptr: int, tangent_ptr: int | None, log: bool,
                            eps: float, stream: int, scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_dev_lengths: clips ``x[b, :lengths[b]]`` with lambd left on the device (no host read)."""
        _check(load().dmel_forward_dev_lengths(self._h, x_ptr, lengths_ptr, batch, lambd_ptr, (DMEL_FLAG_LOG if log else 0) | int(extra_flags),
                                               float(eps), out_ptr, tangent_ptr, scratch_ptr, stream))

    def backward_x_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd: float, grad_ptr: int, out_ptr: int | None, grad_x_ptr: int,
                           log: bool, stream: int):
        """dmel_backward_x_lengths: the waveform gradient of clips ``x[b, :lengths[b]]`` (zero past a clip, NaN for an invalid length)."""
        _check(load().dmel_backward_x_lengths(self._h, x_ptr, lengths_ptr, batch, C.c_float(float(lambd)), DMEL_FLAG_LOG if log else 0, grad_ptr,
                                              out_ptr if log else None, grad_x_ptr, stream))

    def backward_x_dev_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, grad_ptr: int, out_ptr: int | None,
                               grad_x_ptr: int, log: bool, stream: int, extra_flags: int = 0):
        """dmel_backward_x_dev_lengths: the same with lambd read on the device (n_fft_: what this step's forward launched for)."""
        _check(load().dmel_backward_x_dev_lengths(self._h, x_ptr, lengths_ptr, batch, lambd_ptr, int(n_fft_),
                                                  (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr, out_ptr if log else None, grad_x_ptr,
                                                  stream))

    def forward_dev_fixed(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, out_ptr: int, tangent_ptr: int | None, log: bool,
                          eps: float, stream: int, scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_dev_fixed: one launch for ``n_fft_``, lambd read and checked on the device (trainable filterbank)."""
        _check(load().dmel_forward_dev_fixed(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags),
                                             float(eps), out_ptr, tangent_ptr, scratch_ptr, stream))

    def forward_dev_fixed_spec(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, out_ptr: int, tangent_ptr: int, spec_ptr: int,
                               log: bool, eps: float, stream: int, scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_dev_fixed_spec: the training forward that also writes the (B, F, T) power spectrogram for backward_fb_saved."""
        _check(load().dmel_forward_dev_fixed_spec(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags),
                                                  float(eps), out_ptr, tangent_ptr, spec_ptr, scratch_ptr, stream))

    def backward_fb_saved(self, spec_ptr: int, batch: int, n_fft_: int, grad_ptr: int, out_ptr: int | None, grad_fb_ptr: int, log: bool,
                          stream: int, extra_flags: int = 0):
        _check(load().dmel_backward_fb_saved(self._h, spec_ptr, batch, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr,
                                             out_ptr if log else None, grad_fb_ptr, stream))

    def backward_fb_saved_dl(self, spec_ptr: int, batch: int, n_fft_: int, grad_ptr: int, out_ptr: int | None, tangent_ptr: int, grad_fb_ptr: int,
                             dlambd_ptr: int, scratch_ptr: int | None, log: bool, stream: int, extra_flags: int = 0):
        """dmel_backward_fb_saved_dl: the filterbank gradient on the saved spectrogram and d lambd in one launch (fp32 grad_out)."""
        _check(load().dmel_backward_fb_saved_dl(self._h, spec_ptr, batch, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr,
                                                out_ptr if log else None, tangent_ptr, grad_fb_ptr, dlambd_ptr, scratch_ptr, stream))

    def backward_fb_dev(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, grad_ptr: int, out_ptr: int | None, grad_fb_ptr: int,
                        log: bool, stream: int, extra_flags: int = 0):
        """dmel_backward_fb_dev: dmel_backward_fb with lambd read on the device."""
        _check(load().dmel_backward_fb_dev(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr,
                                           out_ptr if log else None, grad_fb_ptr, stream))

    def forward_dev_fixed_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, out_ptr: int,
                                  tangent_ptr: int | None, spec_ptr: int | None, log: bool, eps: float, stream: int,
                                  scratch_ptr: int | None = None, extra_flags: int = 0):
        """dmel_forward_dev_fixed_lengths: forward_dev_fixed(_spec) over clips of per-clip lengths (a trained filterbank on a zero-padded batch)."""
        _check(load().dmel_forward_dev_fixed_lengths(self._h, x_ptr, lengths_ptr, batch, lambd_ptr, int(n_fft_),
                                                     (DMEL_FLAG_LOG if log else 0) | int(extra_flags), float(eps), out_ptr, tangent_ptr, spec_ptr,
                                                     scratch_ptr, stream))

    def backward_fb_dev_lengths(self, x_ptr: int, lengths_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, grad_ptr: int, out_ptr: int | None,
                                grad_fb_ptr: int, log: bool, stream: int, extra_flags: int = 0):
        """dmel_backward_fb_dev_lengths: the filterbank gradient of clips of per-clip lengths, spectrogram recomputed."""
        _check(load().dmel_backward_fb_dev_lengths(self._h, x_ptr, lengths_ptr, batch, lambd_ptr, int(n_fft_),
                                                   (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr, out_ptr if log else None, grad_fb_ptr,
                                                   stream))

    def backward_fb_saved_lengths(self, spec_ptr: int, lengths_ptr: int, batch: int, n_fft_: int, grad_ptr: int, out_ptr: int | None,
                                  tangent_ptr: int | None, grad_fb_ptr: int, dlambd_ptr: int | None, scratch_ptr: int | None, log: bool,
                                  stream: int, extra_flags: int = 0):
        """dmel_backward_fb_saved_lengths: ... on the saved spectrogram; with tangent_ptr and dlambd_ptr, d lambd in the same launch."""
        _check(load().dmel_backward_fb_saved_lengths(self._h, spec_ptr, lengths_ptr, batch, int(n_fft_),
                                                     (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr, out_ptr if log else None,
                                                     tangent_ptr, grad_fb_ptr, dlambd_ptr, scratch_ptr, stream))

    def backward_x_dev(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, grad_ptr: int, out_ptr: int | None, grad_x_ptr: int,
                       log: bool, stream: int, extra_flags: int = 0):
        """dmel_backward_x_dev: dmel_backward_x with lambd read on the device (n_fft_: what this step's forward ran)."""
        _check(load().dmel_backward_x_dev(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr,
                                          out_ptr if log else None, grad_x_ptr, stream))

    def backward_x_spec_dev(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, grad_spec_ptr: int, grad_x_ptr: int, stream: int,
                            half_window: bool = False):
        _check(load().dmel_backward_x_spec_dev(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), 1 | (2 if half_window else 0),
                                               grad_spec_ptr, grad_x_ptr, stream))

    def spectrogram_ex_dev(self, x_ptr: int, batch: int, lambd_ptr: int, n_fft_: int, spec_ptr: int, tangent_ptr, stream: int,
                           remove_dc: bool = True, half_window: bool = False):
        flags = (1 if remove_dc else 0) | (2 if half_window else 0)
        _check(load().dmel_spectrogram_ex_dev(self._h, x_ptr, batch, lambd_ptr, int(n_fft_), flags, spec_ptr, tangent_ptr, stream))

    def backward_scratch(self, grad_ptr: int, tangent_ptr: int, count: int, dlambd_ptr: int, stream: int, scratch_ptr: int | None,
                         accumulate: bool = False, grad_bf16: bool = False):
        _check(load().dmel_backward_scratch(self._h, grad_ptr, DMEL_DTYPE_BF16 if grad_bf16 else DMEL_DTYPE_F32, tangent_ptr,
                                            int(count), int(accumulate), dlambd_ptr, scratch_ptr, stream))

    def lambd_status(self) -> dict:
        st = DmelLambdStatus()
        _check(load().dmel_plan_lambd_status(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def set_tracking(self, max_ahead: int = 8, guard_mode: int = 0):
        _check(load().dmel_plan_set_tracking(self._h, int(max_ahead), int(guard_mode)))

    def lambd_reset(self):
        _check(load().dmel_plan_lambd_reset(self._h))

    # -- the multi-window layer (dmel_forward_multi*, dmel_backward_multi) --
    def scratch_bytes_multi(self, batch: int, channels: int) -> int:
        return int(load().dmel_scratch_bytes_multi(self._h, int(batch), int(channels)))

    # (``lengths_ptr``: int32 per-clip lengths on the device -- the *_lengths entry points; None: the whole rows)
    def forward_multi(self, x_ptr: int, batch: int, lambd, out_ptr: int, tangent_ptr: int | None, log: bool, eps: float, stream: int,
                      scratch_ptr: int, out_bf16: bool = False, lengths_ptr: int | None = None):
        """lambd: the K host values (a sequence of floats)"""
        lam = _floats(lambd)
        flags = (DMEL_FLAG_LOG if log else 0) | (DMEL_FLAG_OUT_BF16 if out_bf16 else 0)
        tail = (batch, lam, len(lambd), flags, float(eps), out_ptr, tangent_ptr, scratch_ptr, stream)
        if lengths_ptr is None:
            _check(load().dmel_forward_multi(self._h, x_ptr, *tail))
        else:
            _check(load().dmel_forward_multi_lengths(self._h, x_ptr, lengths_ptr, *tail))

    def forward_multi_dev(self, x_ptr: int, batch: int, lambd_ptr: int, channels: int, out_ptr: int, tangent_ptr: int | None, log: bool,
                          eps: float, stream: int, scratch_ptr: int, out_bf16: bool = False, lengths_ptr: int | None = None):
        flags = (DMEL_FLAG_LOG if log else 0) | (DMEL_FLAG_OUT_BF16 if out_bf16 else 0)
        tail = (batch, lambd_ptr, int(channels), flags, float(eps), out_ptr, tangent_ptr, scratch_ptr, stream)
        if lengths_ptr is None:
            _check(load().dmel_forward_multi_dev(self._h, x_ptr, *tail))
        else:
            _check(load().dmel_forward_multi_dev_lengths(self._h, x_ptr, lengths_ptr, *tail))

    def backward_multi(self, grad_ptr: int, tangent_ptr: int, batch: int, channels: int, dlambd_ptr: int, stream: int, scratch_ptr: int,
                       accumulate: bool = False, grad_bf16: bool = False):
        _check(load().dmel_backward_multi(self._h, grad_ptr, DMEL_DTYPE_BF16 if grad_bf16 else DMEL_DTYPE_F32, tangent_ptr, int(batch),
                                          int(channels), int(accumulate), dlambd_ptr, scratch_ptr, stream))

    # -- the band-split layer (dmel_forward_band*, dmel_backward_band): one (B, 1, M, T) image, channel k owns rows edges[k] ... edges[k + 1] - 1 --
    def forward_band(self, x_ptr: int, batch: int, lambd, edges, out_ptr: int, tangent_ptr: int | None, log: bool, eps: float, stream: int,
                     scratch_ptr: int, out_bf16: bool = False, lengths_ptr: int | None = None):
        """lambd: the K host values; edges: K + 1 host integers"""
        lam = _floats(lambd)
        ed = _ints(edges)
        flags = (DMEL_FLAG_LOG if log else 0) | (DMEL_FLAG_OUT_BF16 if out_bf16 else 0)
        tail = (batch, lam, len(lambd), ed, flags, float(eps), out_ptr, tangent_ptr, scratch_ptr, stream)
        if lengths_ptr is None:
            _check(load().dmel_forward_band(self._h, x_ptr, *tail))
        else:
            _check(load().dmel_forward_band_lengths(self._h, x_ptr, lengths_ptr, *tail))

    def forward_band_dev(self, x_ptr: int, batch: int, lambd_ptr: int, edges, out_ptr: int, tangent_ptr: int | None, log: bool,
                         eps: float, stream: int, scratch_ptr: int, out_bf16: bool = False, lengths_ptr: int | None = None):
        ed = _ints(edges)
        flags = (DMEL_FLAG_LOG if log else 0) | (DMEL_FLAG_OUT_BF16 if out_bf16 else 0)
        tail = (batch, lambd_ptr, len(edges) - 1, ed, flags, float(eps), out_ptr, tangent_ptr, scratch_ptr, stream)
        if lengths_ptr is None:
            _check(load().dmel_forward_band_dev(self._h, x_ptr, *tail))
        else:
            _check(load().dmel_forward_band_dev_lengths(self._h, x_ptr, lengths_ptr, *tail))

    def backward_band(self, grad_ptr: int, tangent_ptr: int, batch: int, edges, dlambd_ptr: int, stream: int, scratch_ptr: int,
                      accumulate: bool = False, grad_bf16: bool = False):
        ed = _ints(edges)
        _check(load().dmel_backward_band(self._h, grad_ptr, DMEL_DTYPE_BF16 if grad_bf16 else DMEL_DTYPE_F32, tangent_ptr, int(batch),
                                         len(edges) - 1, ed, int(accumulate), dlambd_ptr, scratch_ptr, stream))

    def backward_x_multi(self, x_ptr: int, batch: int, lambd, grad_ptr: int, out_ptr: int | None, grad_x_ptr: int, log: bool, stream: int,
                         edges=None, lengths_ptr: int | None = None):
        """dmel_backward_x_multi: grad_x = sum over channels (ascending) of the scalar layer's waveform gradient; lambd: the K host values;
        grad_ptr / out_ptr: (B, K, M, T) fp32.  With ``edges`` (K + 1 host integers) dmel_backward_x_band: grad_ptr / out_ptr are ONE
        (B, 1, M, T) image and channel k's cotangent is its rows edges[k] ... edges[k + 1] - 1, +0.0 elsewhere.  With ``lengths_ptr`` the
        *_lengths entry points (see forward_multi)."""
        lam = _floats(lambd)
        flags = DMEL_FLAG_LOG if log else 0
        head = (self._h, x_ptr) if lengths_ptr is None else (self._h, x_ptr, lengths_ptr)
        tail = (flags, grad_ptr, out_ptr, grad_x_ptr, stream)
        if edges is None:
            fn = load().dmel_backward_x_multi if lengths_ptr is None else load().dmel_backward_x_multi_lengths
            _check(fn(*head, batch, lam, len(lambd), *tail))
        else:
            fn = load().dmel_backward_x_band if lengths_ptr is None else load().dmel_backward_x_band_lengths
            _check(fn(*head, batch, lam, len(lambd), _ints(edges), *tail))

    def backward_x_multi_dev(self, x_ptr: int, batch: int, lambd_ptr: int, channels: int, launches, grad_ptr: int, out_ptr: int | None,
                             grad_x_ptr: int, log: bool, stream: int, edges=None, lengths_ptr: int | None = None):
        """dmel_backward_x_multi_dev: lambd read on the device; launches: [(n_fft, channel mask), ...] of the forward whose gradient
        this is (last_multi_launch() right after it).  With ``edges``: dmel_backward_x_band_dev (see backward_x_multi)."""
        k = max(len(launches), 1)
        ns = (C.c_int32 * k)(*[int(n) for n, _ in launches])
        masks = (C.c_uint32 * k)(*[int(m) for _, m in launches])
        flags = DMEL_FLAG_LOG if log else 0
        head = (self._h, x_ptr) if lengths_ptr is None else (self._h, x_ptr, lengths_ptr)
        tail = (ns, masks, len(launches), flags, grad_ptr, out_ptr, grad_x_ptr, stream)
        if edges is None:
            fn = load().dmel_backward_x_multi_dev if lengths_ptr is None else load().dmel_backward_x_multi_dev_lengths
            _check(fn(*head, batch, lambd_ptr, int(channels), *tail))
        else:
            fn = load().dmel_backward_x_band_dev if lengths_ptr is None else load().dmel_backward_x_band_dev_lengths
            _check(fn(*head, batch, lambd_ptr, int(channels), _ints(edges), *tail))

    def backward_x_band(self, x_ptr: int, batch: int, lambd, edges, grad_ptr: int, out_ptr: int | None, grad_x_ptr: int, log: bool, stream: int,
                        lengths_ptr: int | None = None):
        """dmel_backward_x_band(_lengths): the band-split layer's waveform gradient, lambd as K host values"""
        self.backward_x_multi(x_ptr, batch, lambd, grad_ptr, out_ptr, grad_x_ptr, log, stream, edges=edges, lengths_ptr=lengths_ptr)

    def backward_x_band_dev(self, x_ptr: int, batch: int, lambd_ptr: int, edges, launches, grad_ptr: int, out_ptr: int | None,
                            grad_x_ptr: int, log: bool, stream: int, lengths_ptr: int | None = None):
        """dmel_backward_x_band_dev(_lengths): lambd read on the device; launches: last_multi_launch() right after the forward_band_dev
        whose gradient this is"""
        self.backward_x_multi_dev(x_ptr, batch, lambd_ptr, len(edges) - 1, launches, grad_ptr, out_ptr, grad_x_ptr, log, stream, edges=edges,
                                  lengths_ptr=lengths_ptr)

    def last_multi_launch(self) -> list[tuple[int, int]]:
        """[(n_fft, channel mask), ...] in ascending n_fft: what the most recent forward_multi(_dev) / forward_band(_dev) on this plan issued
        (host bookkeeping)"""
        ns, masks, cnt = (C.c_int32 * 24)(), (C.c_uint32 * 24)(), C.c_int32(0)
        _check(load().dmel_plan_last_multi_launch(self._h, ns, masks, C.byref(cnt)))
        return [(int(ns[i]), int(masks[i])) for i in range(cnt.value)]

    def lambd_status_channel(self, channel: int) -> dict:
        st = DmelLambdStatus()
        _check(load().dmel_plan_lambd_status_channel(self._h, int(channel), C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def lambd_report(self, number: int):
        """lambd as read by execution ``number`` (None if its report has left the ring): timing-independent, see include/dmel.h."""
        lam, found = C.c_float(0.0), C.c_int32(0)
        _check(load().dmel_plan_lambd_report(self._h, C.c_uint32(int(number) & 0xFFFFFFFF), C.cast(C.byref(lam), C.POINTER(C.c_float)), C.byref(found)))
        return float(lam.value) if found.value else None

    def attach_mailbox(self, mailbox):
        """dmel_plan_attach_mailbox: backward() on this plan returns the sum over the mailbox's ranks (None detaches)."""
        _check(load().dmel_plan_attach_mailbox(self._h, mailbox._h if mailbox is not None else None))
        self._mailbox = mailbox                       # keep it alive as long as the plan points at it

    def attach_adam(self, param_ptr, exp_avg_ptr=0, exp_avg_sq_ptr=0, step_ptr=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                    weight_decay=0.0, maximize=False, keep=None):
        """dmel_plan_attach_adam: every backward() on this plan ends with Adam's update of the fp32 device scalar at ``param_ptr`` by the
        gradient it has just written (``param_ptr`` = 0 / None detaches).  ``keep``: the objects that own the four addresses -- referenced
        from the plan for as long as it carries them (the caching allocator must not hand that memory to anyone else meanwhile)."""
        self._adam_keep = keep if param_ptr else None
        _check(load().dmel_plan_attach_adam(self._h, param_ptr or None, exp_avg_ptr or None, exp_avg_sq_ptr or None, step_ptr or None,
                                            C.c_double(float(lr)), C.c_double(float(beta1)), C.c_double(float(beta2)), C.c_double(float(eps)),
                                            C.c_double(float(weight_decay)), 1 if maximize else 0))

    def force_launch(self, n_fft_: int = 0, guards: int = 0):
        """dmel_plan_force_launch: the caller chooses the launches of dmel_forward_dev (n_fft_ = 0: automatic again)."""
        _check(load().dmel_plan_force_launch(self._h, int(n_fft_), int(guards)))

    def backward(self, grad_ptr: int, tangent_ptr: int, count: int, dlambd_ptr: int, stream: int, accumulate: bool = False,
                 grad_bf16: bool = False):
        if grad_bf16:
            _check(load().dmel_backward_ex(self._h, grad_ptr, DMEL_DTYPE_BF16, tangent_ptr, int(count), int(accumulate), dlambd_ptr, stream))
        else:
            _check(load().dmel_backward(self._h, grad_ptr, tangent_ptr, int(count), int(accumulate), dlambd_ptr, stream))

    def backward_fb(self, x_ptr: int, batch: int, lambd: float, grad_ptr: int, out_ptr: int | None, grad_fb_ptr: int,
                    log: bool, stream: int, extra_flags: int = 0):
        """grad of the loss w.r.t. the (n_fft/2+1, n_mels) filterbank (adjoint of models.py:53)."""
        _check(load().dmel_backward_fb(self._h, x_ptr, batch, C.c_float(float(lambd)),
                                       (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr, out_ptr if log else None,
                                       grad_fb_ptr, stream))

    def backward_x(self, x_ptr: int, batch: int, lambd: float, grad_ptr: int, out_ptr: int | None, grad_x_ptr: int,
                   log: bool, stream: int, extra_flags: int = 0):
        """grad of the loss w.r.t. the waveform (adjoint of models.py:38-53)."""
        _check(load().dmel_backward_x(self._h, x_ptr, batch, C.c_float(float(lambd)), (DMEL_FLAG_LOG if log else 0) | int(extra_flags), grad_ptr,
                                      out_ptr if log else None, grad_x_ptr, stream))

    def backward_x_spec(self, x_ptr: int, batch: int, lambd: float, n_fft_: int, grad_spec_ptr: int, grad_x_ptr: int, stream: int,
                        half_window: bool = False):
        """grad of the loss w.r.t. the waveform through the spectrogram layer (models.py:171-200)."""
        _check(load().dmel_backward_x_spec(self._h, x_ptr, batch, C.c_float(float(lambd)), int(n_fft_), 1 | (2 if half_window else 0),
                                           grad_spec_ptr, grad_x_ptr, stream))

    def spectrogram(self, x_ptr: int, batch: int, lambd: float, spec_ptr: int, stream: int, remove_dc: bool = False):
        _check(load().dmel_spectrogram(self._h, x_ptr, batch, C.c_float(float(lambd)), int(remove_dc), spec_ptr, stream))

    def spectrogram_ex(self, x_ptr: int, batch: int, lambd: float, n_fft_: int, spec_ptr: int, tangent_ptr, stream: int,
                       remove_dc: bool = True, half_window: bool = False):
        flags = (1 if remove_dc else 0) | (2 if half_window else 0)
        _check(load().dmel_spectrogram_ex(self._h, x_ptr, batch, C.c_float(float(lambd)), int(n_fft_), flags, spec_ptr,
                                          tangent_ptr, stream))

    def set_filterbank(self, n_fft_: int, fb):
        import numpy as np
        if fb is None:
            _check(load().dmel_plan_set_filterbank(self._h, int(n_fft_), None))
            return
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        if fb.shape != (n_fft_ // 2 + 1, self.n_mels):
            raise ValueError(f"filterbank must be ({n_fft_ // 2 + 1}, {self.n_mels}), got {fb.shape}")
        _check(load().dmel_plan_set_filterbank(self._h, int(n_fft_), fb.ctypes.data_as(C.POINTER(C.c_float))))

    def set_filterbank_dev(self, n_fft_: int, fb_ptr: int, stream: int):
        """(n_fft/2+1, n_mels) fp32 row-major DEVICE matrix -> the plan's tables, on ``stream`` (no host copy, no sync)."""
        _check(load().dmel_plan_set_filterbank_dev(self._h, int(n_fft_), fb_ptr, stream))

    def set_profiling(self, enable: bool):
        _check(load().dmel_plan_set_profiling(self._h, int(bool(enable))))

    def get_profile(self) -> dict:
        pr = DmelProfile()
        _check(load().dmel_plan_get_profile(self._h, C.byref(pr)))
        return {k: getattr(pr, k) for k, _ in pr._fields_}

    def info(self) -> dict:
        inf = DmelPlanInfo()
        _check(load().dmel_plan_get_info(self._h, C.byref(inf)))
        return inf.as_dict()


class Comm:
    """Owner of a dmel_comm handle: native RCCL all-reduce of the scalar gradient (include/dmel.h)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        _check(load().dmel_comm_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == Comm.ID_BYTES
        self._h = C.c_void_p()
        _check(load().dmel_comm_create(C.create_string_buffer(unique_id, Comm.ID_BYTES), int(rank), int(world), C.byref(self._h)))

    def allreduce_async(self, buf_ptr: int, count: int, stream: int) -> int:
        t = C.c_int32(-1)
        _check(load().dmel_comm_allreduce_async(self._h, buf_ptr, int(count), stream, C.byref(t)))
        return int(t.value)

    def allreduce(self, buf_ptr: int, count: int, stream: int) -> None:
        """In-stream SUM all-reduce (ordered like a kernel launch on ``stream``)."""
        _check(load().dmel_comm_allreduce(self._h, buf_ptr, int(count), stream))

    def wait(self, ticket: int, stream: int) -> None:
        _check(load().dmel_comm_wait(self._h, int(ticket), stream))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().dmel_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mailbox:
    """Owner of a dmel_mailbox handle: the peer-to-peer all-reduce of lambd.grad folded into the backward's kernel (include/dmel.h)."""

    HANDLE_BYTES = 64

    def __init__(self, rank: int, world: int):
        self._h = C.c_void_p()
        buf = C.create_string_buffer(Mailbox.HANDLE_BYTES)
        _check(load().dmel_mailbox_create(int(rank), int(world), C.byref(self._h), buf))
        self.rank, self.world, self.handle = int(rank), int(world), buf.raw

    def connect(self, handles):
        """``handles``: the 64-byte handles of all ranks in rank order (this rank's own entry is not opened)."""
        blob = b"".join(handles)
        assert len(blob) == self.world * Mailbox.HANDLE_BYTES
        _check(load().dmel_mailbox_connect(self._h, C.create_string_buffer(blob, len(blob))))

    def allreduce(self, buf_ptr: int, stream: int) -> None:
        """buf[0] = sum over ranks of buf[0], one tiny launch on ``stream``."""
        _check(load().dmel_mailbox_allreduce(self._h, buf_ptr, stream))

    def error(self):
        """None, or (step, missing_rank) of the first exchange that timed out since the last call."""
        failed, step, miss = C.c_int32(0), C.c_uint32(0), C.c_int32(0)
        _check(load().dmel_mailbox_error(self._h, C.byref(failed), C.byref(step), C.byref(miss)))
        return (int(step.value), int(miss.value)) if failed.value else None

    def set_spin_limit(self, polls: int) -> None:
        """polls per source rank before an exchange gives up; 0 = no limit on the count (the wall-clock bound holds)"""
        _check(load().dmel_mailbox_set_spin_limit(self._h, int(polls)))

    def set_timeout_ms(self, ms: int) -> None:
        """wall-clock bound of one exchange (default 120 000 ms; 0 = wait for ever)"""
        _check(load().dmel_mailbox_set_timeout_ms(self._h, C.c_uint64(int(ms))))

    def close(self):
        """raises while a plan still holds the mailbox (detach or release the plans first: MailboxAllReduce.close does)"""
        if getattr(self, "_h", None) is not None and self._h.value:
            _check(load().dmel_mailbox_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
