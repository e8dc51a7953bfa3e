/*
 * dmel.h -- C ABI of libdmel_hip.so: the MI355X (gfx950) implementation of the DMEL hot path.
 *
 * The reference (johnmartinsson/differentiable-mel-spectrogram) is pure Python and has no FFI;
 * its boundary for this path is the nn.Module `MelSpectrogramLayer` (models.py:14-56) plus the
 * `torch.log(s + 1e-10)` line of the nets that wrap it (models.py:73).  Each entry point below
 * names the reference code it replaces.  Signatures carry plain pointers and sizes only (device
 * pointers are HIP device addresses, `stream` is a hipStream_t passed as void*); no torch types.
 *
 * Conventions
 *   - every function returns a dmel_status (0 = DMEL_OK); dmel_last_error() gives the message of
 *     the calling thread's last failure.
 *   - waveforms  x        : (batch, n_points) fp32, row-major, device      models.py:33
 *   - outputs    out      : (batch, 1, n_mels, n_points / hop + 1) fp32    models.py:30,36
 *   - tangent             : same shape as out, d out / d lambd (raw, signed parameter)
 *   - lambd is the trainable window std-dev in samples (models.py:19); the kernels use |lambd|
 *     (models.py:38) and n_fft = next_pow2(int(6*|lambd|)) (time_frequency.py:39,60-65).
 *   - a plan owns its device tables and a default scratch; calls that use the plan's scratch from different streams
 *     are ordered after each other by the library (an event), calls with caller scratch are independent.
 *
 * Alignment
 *   - pointers the library only READS need the alignment of their element and nothing more: x, lengths, lambd_dev, the
 *     filterbank, grad_out (4 bytes for fp32, 2 for bf16), and a tangent, saved output or saved spectrogram handed back to a
 *     backward call.  A contiguous view into a larger buffer, a slice of a concatenated gradient or the address in a
 *     DMEL_FLAG_X_INDIRECT cell is fine at any element offset: the kernels choose their loads by the address they are given.
 *   - pointers the library STORES through must be 16-byte aligned: out, tangent, spec, grad_x, grad_fb and a caller's scratch.
 *     The kernels write them with 8- and 16-byte stores (packed bf16 pairs for DMEL_FLAG_OUT_BF16) that are guarded by shape only.
 *     Every entry point checks this on the host and returns DMEL_ERR_INVALID_ARGUMENT, naming the argument, before it launches
 *     anything.  hipMalloc and every framework allocator return blocks aligned far beyond this; it matters when a caller carves
 *     outputs out of one block.  (dlambd and the optimizer's one-element tensors are stored as single floats: 4 bytes.)
 */
#ifndef DMEL_H
#define DMEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMEL_ABI_VERSION 5   /* round 6: dmel_plan_info.contraction / wl_steps; DMEL_FLAG_X_INDIRECT served by every forward kernel (round 4 = 4: *_dev variants of the fixed-length paths, saved spectrogram, DMEL_FLAG_MFMA_BF16X3, mailbox time-out, plan registry) */

typedef enum dmel_status {
    DMEL_OK = 0,
    DMEL_ERR_INVALID_ARGUMENT = 1,  /* bad shape / null pointer / negative size / an output pointer that is not 16-byte aligned */
    DMEL_ERR_UNSUPPORTED = 2,       /* a transform that needs an FFT of more than 1048576 points (|lambd| > 174762, or an
                                       optimized=False clip longer than 262144 samples) */
    DMEL_ERR_HIP = 3,               /* a HIP runtime call failed (message has the detail) */
    DMEL_ERR_NO_DEVICE = 4,         /* no gfx950 device visible                           */
    DMEL_ERR_OUT_OF_MEMORY = 5,
    DMEL_ERR_LAMBD_TRACKING = 6,    /* dmel_forward_dev: lambd changed n_fft faster than the sync-free path covers   */
    DMEL_ERR_MAILBOX_TIMEOUT = 7    /* an exchange of the plan's mailbox gave up on a rank (the gradient it returned was NaN): reported by
                                       the next forward / backward on the plan, sticky until dmel_mailbox_error reads it */
} dmel_status;

/* Constructor arguments of the layer: models.py:15-30 (MelSpectrogramLayer.__init__). */
typedef struct dmel_config {
    int32_t n_points;          /* clip length L                                   models.py:30 */
    int32_t hop_length;        /*                                                 models.py:18 */
    int32_t n_mels;            /*                                                 models.py:26 */
    int32_t sample_rate;       /*                                                 models.py:27 */
    double f_min;              /*                                                 models.py:24 */
    double f_max;              /* < 0: sample_rate / 2 (integer division)         models.py:25 */
    int32_t normalize_window;  /* time_frequency.py:25-28 (norm=True branch)                   */
    int32_t max_batch;         /* workspace is sized for this many clips (grown on demand)     */
} dmel_config;

typedef struct dmel_plan dmel_plan;

/* Flags for dmel_forward */
#define DMEL_FLAG_LOG 1u       /* fuse out = log(mel + eps)                        models.py:73 */
#define DMEL_FLAG_FULL_WINDOW 2u /* the layer's optimized=False branch: window = whole clip, n_fft = 2*n_points
                                  (time_frequency.py:41,51); any n_points (powers of two up to 8192 on the FFT kernels,
                                  everything else through the global-memory / chirp-z path)                */
#define DMEL_FLAG_OUT_BF16 4u   /* dmel_forward writes `out` as bf16 (round to nearest even of the fp32 result; BASELINE
                                  config 2 "bf16 activations / fp32 grad"): half the output bytes.  The arithmetic, the
                                  tangent and d lambd stay fp32.  The reference's output is fp32 (models.py:36).          */
#define DMEL_FLAG_MFMA_BF16X3 8u /* opt-in: dense contractions (dmel_backward_fb*: the filterbank gradient's GEMM; dmel_forward* with a
                                   caller-supplied DENSE filterbank) run on the bf16 matrix pipe as three split-bf16 products per fp32
                                   product (hi hi + lo hi + hi lo, fp32 accumulate: ~2e-5 relative, inside the 1e-4 bar; 16 x the fp32 MFMA
                                   rate).  Default: exact fp32 MFMA (v_mfma_f32_16x16x4_f32).  The HTK bank's banded contraction ignores it. */
#define DMEL_FLAG_CHECK_NFFT 16u /* dmel_backward_x_dev(_lengths) only: the kernels do their work only if the device value of lambd asks for exactly the
                                   `n_fft` of this call (time_frequency.py:39,60-65 evaluated on the device) and otherwise leave grad_x
                                   untouched.  For the optimized=True layer whose forward (dmel_forward_dev) issued one launch per candidate
                                   n_fft: the caller fills grad_x with NaN and issues one dmel_backward_x_dev per candidate. */
#define DMEL_FLAG_X_INDIRECT 32u /* dmel_forward_dev only (round 5): `x` is a device pointer to ONE device pointer -- the address of the batch, read by
                                   the kernel when it runs.  A step captured into a HIP graph reads static addresses; with this flag the static
                                   address is that of a pointer cell, and handing the step a new batch (train.py:25-49: one per iteration) is an
                                   8-byte write instead of a copy of the batch (dmel_amd.GraphedStep.feed, zero_copy).  Every kernel of the
                                   forward reads the cell (round 6: the direct-DFT kernel below n_fft 32 and the global-memory / chirp-z path beyond
                                   16384 too, so a lambd that drifts out of the fused kernel's range inside a captured loop is served like any
                                   other).  The batch must stay valid until the forward has executed. */
#define DMEL_DTYPE_F32 0
#define DMEL_DTYPE_BF16 1

/* ---- host-side helpers (no device needed) ------------------------------------------------- */

int32_t dmel_abi_version(void);

/* time_frequency.py:60-65 applied as at :39 -- fp32 product 6*|lambd|, int() truncation,
 * 1 << (x-1).bit_length().  Returns n_fft (>= 1). */
int32_t dmel_n_fft(float lambd);

/* time_frequency.py:21-30: Gaussian window of length n_fft centred at n_fft/2 (fp32 arithmetic as
 * the reference), optional L2 normalisation; dwindow (may be NULL) receives d window / d |lambd|. */
dmel_status dmel_window_host(float lambd, int32_t n_fft, int32_t normalize, float* window, float* dwindow);

/* models.py:42-48: torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate)
 * with norm=None, mel_scale="htk".  fb is (n_freqs, n_mels) row-major fp32, host memory. */
dmel_status dmel_mel_fbanks_host(int32_t n_freqs, double f_min, double f_max, int32_t n_mels,
                                 int32_t sample_rate, float* fb);

/* How the fused forward deals the contraction of models.py:53 over the waves of a workgroup (host arithmetic, for tests and tools):
 * `units[t]` = the non-zero extent of mel tile t (16 mels) of one group of `n_tiles` <= `waves` tiles, in units of 16 bins; wave t owns
 * tile t and takes own[t] units from its start, the rest goes in contiguous pieces to other waves -- at most one piece per wave --:
 * piece i = (piece_wave[i], piece_tile[i], piece_first[i], piece_units[i]).  `waves` is 8 or 4; arrays of 8 entries each. */
dmel_status dmel_contraction_partition_host(const int32_t* units, int32_t n_tiles, int32_t waves, int32_t* own, int32_t* n_pieces,
                                            int32_t* piece_wave, int32_t* piece_tile, int32_t* piece_first, int32_t* piece_units);

const char* dmel_last_error(void);

/* ---- device path --------------------------------------------------------------------------- */

/* Number of visible HIP devices whose architecture is gfx950 (0 when none / no driver). */
int32_t dmel_device_count(void);

/* MelSpectrogramLayer.__init__ (models.py:15-30).  Binds to the current HIP device. */
dmel_status dmel_plan_create(const dmel_config* cfg, dmel_plan** plan);
/* A plan is reference counted: dmel_plan_create returns it with one reference, dmel_plan_destroy (= dmel_plan_release) drops one,
 * and the plan is freed -- after the device has finished what was queued on it -- when the last one goes.  Whoever keeps a
 * dmel_plan* beyond the owner's lifetime takes a reference: the autograd node of torch.ops.dmel.mel_spectrogram does, so
 * `y = layer(x); del layer; y.backward(g)` is safe (a plain torch module, models.py:33-56, has no such hazard either).
 * A HIP graph that captured launches of a plan does NOT hold one by itself: keep the layer, or take a reference for the life of the
 * graph (dmel_amd.GraphedStep does: it retains the plans of its layers at every capture and releases them when the graph goes). */
dmel_status dmel_plan_destroy(dmel_plan* plan);
dmel_status dmel_plan_retain(dmel_plan* plan);
dmel_status dmel_plan_release(dmel_plan* plan);
/* 1 while `plan` is a plan of this process between dmel_plan_create and its last release, 0 for anything else (never dereferences
 * the pointer: a registry lookup).  Bindings that pass plans as integers (torch.ops.dmel.*) check this before every use. */
int32_t dmel_plan_is_live(const dmel_plan* plan);
/* depth of the pinned ring the executed forwards of a plan report into (dmel_plan_lambd_report finds execution `number` while fewer
 * than this many later ones have executed): whoever looks reports up late -- dmel_amd.GraphedStep, (max_ahead + 1) replays of
 * `steps_per_replay` forwards behind -- keeps that distance below it */
int32_t dmel_lambd_ring_size(void);
dmel_status dmel_plan_get_config(const dmel_plan* plan, dmel_config* cfg);

/* Replace the mel filterbank of the plan by a caller-supplied (n_freqs, n_mels) fp32 HOST matrix for
 * the given n_fft (n_freqs = n_fft/2+1; 1 or any even length up to 1048576): the contraction of models.py:53 then uses it instead
 * of the HTK table.  Pass fb = NULL to return to the built-in table. */
dmel_status dmel_plan_set_filterbank(dmel_plan* plan, int32_t n_fft, const float* fb);

/* The same from a DEVICE matrix (a trainable filterbank after an optimizer step): the first call for an n_fft rebuilds that
 * n_fft's tables with the dense structure (every 4x16 block multiplied; one device synchronisation), every later call is one
 * small kernel on `stream` that refreshes the values -- no host copy, no synchronisation, capturable.  Return to the built-in
 * table with dmel_plan_set_filterbank(plan, n_fft, NULL). */
dmel_status dmel_plan_set_filterbank_dev(dmel_plan* plan, int32_t n_fft, const float* fb_dev, void* stream);

/*
 * MelSpectrogramLayer.forward (models.py:33-56) [+ models.py:73 when DMEL_FLAG_LOG]:
 * DC removal, Gaussian-windowed STFT (center=True, zero padding), |.|^2, mel contraction.
 *   x        device, (batch, n_points) fp32
 *   lambd    host value of the parameter (the reference reads it to the host too,
 *            time_frequency.py:39); may be negative or zero
 *   out      device, (batch, 1, n_mels, n_time) fp32 (bf16 elements with DMEL_FLAG_OUT_BF16: pass the pointer cast)
 *   tangent  device, same shape, or NULL for inference: receives d out / d lambd so that
 *            the backward is a single dot product (one trainable scalar -> forward mode)
 *   eps      the 1e-10 of models.py:73 (ignored without DMEL_FLAG_LOG)
 * Asynchronous on `stream`.
 */
dmel_status dmel_forward(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                         double eps, float* out, float* tangent, void* stream);

/*
 * The same forward with lambd left ON THE DEVICE: no device->host read, so a training step (forward, backward,
 * optimizer update of lambd) can be queued without the host ever waiting, and captured into a HIP graph.  The
 * reference reads lambd to the host once per sample to derive n_fft (time_frequency.py:39); here every kernel reads
 * the device scalar itself, derives the window from it and checks that next_pow2(int(6|lambd|)) is the n_fft it was
 * launched for.  The host picks that n_fft from what the kernels last reported (a pinned word, no synchronisation)
 * and, while lambd is within reach of a power-of-two boundary (or under graph capture), adds guard launches for the
 * neighbouring n_fft that return at once unless the work is theirs.  A forward that no launch covers (lambd crossed
 * more than the guards allow while the host was running ahead) writes NaN to its outputs and the NEXT call returns
 * DMEL_ERR_LAMBD_TRACKING once; the run-ahead is bounded (dmel_plan_set_tracking) to keep that out of reach.
 *   lambd_dev  device, 1 fp32 (e.g. the nn.Parameter's storage); read by the kernels at execution time
 *   out        device, fp32 (bf16 with DMEL_FLAG_OUT_BF16)
 *   scratch    device, dmel_scratch_bytes(plan, batch) bytes owned by the caller for this call and for the
 *              dmel_backward_scratch that consumes its tangent (no initialisation needed), or NULL to use the plan's
 *              own (then calls on different streams are serialised by the plan)
 * The first call on a plan (and the first after an error or dmel_plan_lambd_reset) reads lambd once, blocking.
 * DMEL_FLAG_FULL_WINDOW is not accepted (its n_fft does not depend on lambd: use dmel_forward_dev_fixed, which needs no tracking).
 */
size_t dmel_scratch_bytes(const dmel_plan* plan, int32_t batch);
/* dmel_forward (lambd by value) with the caller's scratch instead of the plan's */
dmel_status dmel_forward_scratch(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                                 double eps, void* out, float* tangent, void* scratch, void* stream);
dmel_status dmel_forward_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, uint32_t flags,
                             double eps, void* out, float* tangent, void* scratch, void* stream);
/* The same forward for callers whose n_fft is fixed by something else than lambd -- a trainable filterbank matrix
 * (dmel_plan_set_filterbank_dev) has n_fft/2+1 rows: exactly one launch for `n_fft`, lambd read and checked on the device, no
 * guard launches, no host picture of lambd (never blocks, capturable from the first call).  If the device value asks for
 * another n_fft the outputs are NaN and the NEXT call returns DMEL_ERR_LAMBD_TRACKING (models.py:42-48 ties the reference's
 * matrix to the n_fft of the forward in the same way: torch.matmul fails on the shape).
 * With DMEL_FLAG_FULL_WINDOW (the layer's optimized=False branch, time_frequency.py:41,51) the transform is n_fft = 2 n_points
 * whatever lambd is: `n_fft` is ignored, nothing is checked, lambd only shapes the window the kernels build from the device value. */
dmel_status dmel_forward_dev_fixed(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                   uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
/* dmel_forward_dev_fixed that ALSO writes the power spectrogram the contraction consumed -- spec: device, (batch, n_fft/2+1, n_time) fp32,
 * the layout of time_frequency.py:53 -- for dmel_backward_fb_saved: the filterbank gradient then skips its recompute of the spectrogram
 * (16.5 us of 43 at BASELINE config 2, for 16.8 MB more stored here).  Training forward only (tangent != NULL), power-of-two n_fft
 * from 32 to 16384, not with DMEL_FLAG_FULL_WINDOW; spec = NULL is plain dmel_forward_dev_fixed. */
dmel_status dmel_forward_dev_fixed_spec(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                        uint32_t flags, double eps, void* out, float* tangent, float* spec, void* scratch, void* stream);
/* Per-clip lengths (zero-padded batches): dmel_forward_scratch / dmel_forward_dev over clips x[b, :lengths[b]].  lengths: device, `batch`
 * int32 values, read by the kernels when they run (never by the host: a captured forward sees what the buffer holds at replay).  Clip b
 * is computed as a plan with n_points = lengths[b] would compute it (its own mean; the centred frames zero-padded past lengths[b]) for
 * its frames t < lengths[b] / hop_length + 1; the frames after them are pad frames -- the value of a frame of zero mel power (0, or the
 * kernel's log(0 + eps) with DMEL_FLAG_LOG) and a zero tangent -- and tiles of pad frames are not transformed.  x[b, lengths[b]:] is
 * never read.  A length outside 1 ... n_points makes that clip's rows (and its tangent) NaN; the other clips are unaffected.
 * The tangent carries the usual meaning, so dmel_backward_scratch on it gives d loss / d lambd.  Flags: DMEL_FLAG_LOG, DMEL_FLAG_OUT_BF16,
 * DMEL_FLAG_X_INDIRECT.  The HTK bank and n_fft 32 ... 16384 only: dmel_forward_lengths refuses a lambd outside that range
 * (DMEL_ERR_UNSUPPORTED); dmel_forward_dev_lengths clamps its launches to it (a forward no launch covered is NaN and the next call
 * returns DMEL_ERR_LAMBD_TRACKING, as dmel_forward_dev).  Scratch as dmel_forward_scratch / dmel_forward_dev.  NULL handles and pointers:
 * DMEL_ERR_INVALID_ARGUMENT before any device call. */
dmel_status dmel_forward_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, float lambd, uint32_t flags,
                                 double eps, void* out, float* tangent, void* scratch, void* stream);
dmel_status dmel_forward_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                     uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
/* Per-clip lengths through a TRAINED filterbank (dmel_plan_set_filterbank_dev; the reference's AudioMNIST loader pads its clips,
 * datasets.py:175, and a bank trained on them contracts at models.py:53): dmel_forward_dev_fixed / dmel_forward_dev_fixed_spec over clips
 * x[b, :lengths[b]].  Clip b loses its own mean (models.py:38 over lengths[b] samples), its frames t >= lengths[b] / hop_length + 1 are pad
 * frames (0, or the kernel's log(0 + eps); tangent 0; models.py:73), x[b, lengths[b]:] is never read, and a length outside 1 ... n_points makes
 * the clip's rows, its tangent and -- with `spec` -- its whole (n_fft/2+1, n_time) spectrogram NaN.  One launch for `n_fft`, a power of two
 * in 32 ... 16384; lambd is read and checked on the device as dmel_forward_dev_fixed does (no host read of lambd or lengths: capturable).
 * spec: NULL, or (batch, n_fft/2+1, n_time) fp32 for dmel_backward_fb_saved_lengths (then tangent != NULL); its columns of pad frames
 * are not meaningful.  Flags: DMEL_FLAG_LOG, DMEL_FLAG_OUT_BF16, DMEL_FLAG_MFMA_BF16X3 (the dense contraction on the bf16 matrix pipe,
 * n_fft 64 ... 4096).  With every length at n_points the results have the bits of dmel_forward_dev_fixed(_spec).  NULL handles and
 * pointers, a misaligned out / tangent / spec / scratch: DMEL_ERR_INVALID_ARGUMENT before any device call. */
dmel_status dmel_forward_dev_fixed_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                           int32_t n_fft, uint32_t flags, double eps, void* out, float* tangent, float* spec, void* scratch,
                                           void* stream);

/* Every forward that EXECUTES on a plan (an eager dmel_forward_dev, or one replay of a captured one) draws the next
 * EXECUTION NUMBER from a device counter and reports (number, lambd as it read it) into a pinned ring of 64 entries. */
typedef struct dmel_lambd_status {
    int32_t known;            /* 0 until a value has been seen                                             */
    float lambd_seen;         /* lambd as read by the most recent forward that has EXECUTED                */
    int32_t n_fft_seen;
    uint32_t seq_issued;      /* execution number the host expects its most recent eager call to draw (caught up with the
                                 reports: replays of captured forwards execute without the host counting them)            */
    uint32_t seq_seen;        /* execution number lambd_seen belongs to                                    */
    float rate;               /* decayed maximum of |change of lambd| per call                             */
    int32_t guards;           /* most recent call: bit 0 = n_fft/2 guard launched, bit 1 = 2 n_fft guard   */
    int32_t error;            /* 1: a forward was not covered (reported by the next dmel_forward_dev)      */
    uint32_t error_seq;
    float error_lambd;
    int32_t next_n_fft;       /* what a dmel_forward_dev issued now would launch for, and guard (bits as `guards`)        */
    int32_t next_guards;
    uint32_t calls;           /* dmel_forward_dev / _fixed calls on this plan so far, captured ones included               */
} dmel_lambd_status;
dmel_status dmel_plan_lambd_status(dmel_plan* plan, dmel_lambd_status* status);
/* lambd as read by execution `number`, if its report is still in the ring (found = 1).  Unlike dmel_plan_lambd_status, whose
 * picture is "whatever executed last when the host looked", this answer does not depend on timing: ranks of a data-parallel
 * job that issue the same forwards in the same order read the same value for the same number, and can therefore take the
 * same re-capture decision without a collective (dmel_amd.graph.GraphedStep). */
dmel_status dmel_plan_lambd_report(dmel_plan* plan, uint32_t number, float* lambd, int32_t* found);
/* The launch choice as a pure function: n_fft of `lambd` (time_frequency.py:39,60-65) and the neighbouring n_fft a forward
 * must guard (bit 0: n_fft / 2, bit 1: 2 n_fft) when lambd may move by up to `rate` per forward for `stale_forwards` forwards
 * before anybody looks again. */
dmel_status dmel_decide_launch(float lambd, float rate, float stale_forwards, int32_t* n_fft, int32_t* guards);
/* While n_fft > 0, dmel_forward_dev launches exactly for `n_fft` plus the guards given (bits as above) instead of choosing
 * from its own picture; the kernels still check the device value and poison + report a forward nothing covered.  For callers
 * that decide themselves (a captured step that must hold the same launches on every rank).  n_fft = 0: back to automatic. */
dmel_status dmel_plan_force_launch(dmel_plan* plan, int32_t n_fft, int32_t guards);
/* max_ahead: calls the host may be ahead of the last observation before dmel_forward_dev waits (0 = unbounded, default 8);
 * guard_mode: 0 = near boundaries only, and both neighbours whenever the stream is capturing (default: a captured forward
 * is replayed without the host looking); 1 = always both neighbours; 2 = never; 3 = near boundaries only, also under
 * capture -- for callers that watch dmel_plan_lambd_status between replays and re-capture when next_n_fft / next_guards
 * differ from what the graph holds (dmel_amd.graph.GraphedStep does; max_ahead is then the replays it lets queue up) */
dmel_status dmel_plan_set_tracking(dmel_plan* plan, int32_t max_ahead, int32_t guard_mode);
/* forget what was seen (after lambd was rewritten from outside, e.g. load_state_dict): the next call reads it again */
dmel_status dmel_plan_lambd_reset(dmel_plan* plan);

/*
 * Backward to lambd.grad (what loss.backward() reaches through the layer, train.py:47):
 *   dlambd[0] = sum_i grad_out[i] * tangent[i]        (accumulate != 0: += instead of =)
 * grad_out, tangent: device fp32, `count` elements; dlambd: device fp32 scalar.
 * Deterministic (fixed-order two-stage reduction, fp64 accumulation).  Asynchronous on `stream`.
 */
dmel_status dmel_backward(dmel_plan* plan, const float* grad_out, const float* tangent, int64_t count,
                          int32_t accumulate, float* dlambd, void* stream);

/* dmel_backward for a gradient tensor of another element type: grad_dtype = DMEL_DTYPE_F32 or DMEL_DTYPE_BF16 (the
 * gradient of a DMEL_FLAG_OUT_BF16 output; widened exactly, accumulated in fp64 like the fp32 path). */
dmel_status dmel_backward_ex(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int64_t count,
                             int32_t accumulate, float* dlambd, void* stream);
/* dmel_backward_ex with the reduction's partials and ticket in the caller's `scratch` (the block given to the
 * dmel_forward_dev that produced `tangent`, which also zeroed the ticket): nothing plan-owned is touched, so any number of
 * streams may run steps of one plan concurrently.  scratch = NULL: the plan's own. */
dmel_status dmel_backward_scratch(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int64_t count,
                                  int32_t accumulate, float* dlambd, void* scratch, void* stream);

/*
 * Backward to the filterbank matrix ("mel params"): the adjoint of the contraction at models.py:53,
 * `torch.matmul(spectrogram, mel_fb)` with mel_fb (n_freqs, n_mels) from models.py:42-48.  The reference keeps
 * mel_fb constant; this is what torch autograd returns when it is made a leaf:
 *   grad_fb[f][m] = sum_{b,t} spec[b][f][t] * gm[b][m][t]
 *   gm = grad_out                 without DMEL_FLAG_LOG
 *   gm = grad_out * exp(-out)     with DMEL_FLAG_LOG (out = the saved log output of dmel_forward; models.py:73)
 * The spectrogram is recomputed from x (same lambd and flags as the forward), not saved.
 *   x         device, (batch, n_points) fp32       grad_out  device, (batch, 1, n_mels, n_time) fp32
 *   out       device, same shape as grad_out, or NULL without DMEL_FLAG_LOG
 *   grad_fb   device, (n_fft/2+1, n_mels) fp32, overwritten
 * flags: DMEL_FLAG_LOG, DMEL_FLAG_FULL_WINDOW as in dmel_forward; any transform length the forward accepts (the spectrogram pass
 * takes the chirp-z path for lengths that are not powers of two).  Deterministic (fixed-order sum over batch
 * slices, exact-fp32 MFMA).  Asynchronous on `stream`; uses a plan-owned workspace, so calls on one plan must be
 * issued on one stream at a time.
 */
dmel_status dmel_backward_fb(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                             const float* grad_out, const float* out, float* grad_fb, void* stream);
/* dmel_backward_fb with lambd read on the device (the spectrogram recompute checks it against `n_fft`, the one the forward
 * of this step was issued for: dmel_forward_dev_fixed); no host read, capturable.  With DMEL_FLAG_FULL_WINDOW `n_fft` is ignored
 * (2 n_points) and nothing is checked. */
dmel_status dmel_backward_fb_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                 const float* grad_out, const float* out, float* grad_fb, void* stream);
/* dmel_backward_fb on the spectrogram saved by dmel_forward_dev_fixed_spec (same batch, n_fft, plan): the GEMM and the ordered sum of
 * its slices only.  flags: DMEL_FLAG_LOG (then `out` = the saved log output), DMEL_FLAG_MFMA_BF16X3. */
dmel_status dmel_backward_fb_saved(dmel_plan* plan, const float* spec, int32_t batch, int32_t n_fft, uint32_t flags,
                                   const float* grad_out, const float* out, float* grad_fb, void* stream);
/* dmel_backward_fb_saved and dmel_backward_scratch (d lambd = sum(grad_out * tangent), fp32 grad_out, written to `dlambd`, not
 * accumulated) in ONE launch: a few extra workgroups of the gradient's GEMM kernel play the dot kernel's blocks -- the same partition
 * and order of additions, the same bits -- so a trainable-filterbank step (models.py:53 with learnable_fb) issues one kernel less.
 * `scratch`: the dmel_scratch_bytes area the step's forward was given (NULL: the plan's own).  A plan whose reducer lives in the dot
 * kernel (dmel_plan_attach_mailbox), or a launch without room for the extra workgroups, runs the two kernels one after the other:
 * same results. */
dmel_status dmel_backward_fb_saved_dl(dmel_plan* plan, const float* spec, int32_t batch, int32_t n_fft, uint32_t flags,
                                      const float* grad_out, const float* out, const float* tangent, float* grad_fb, float* dlambd,
                                      void* scratch, void* stream);
/* The filterbank gradient of a forward with per-clip lengths (dmel_forward_dev_fixed_lengths; models.py:53 for a batch the loader
 * padded, datasets.py:175):
 *   grad_fb[f][m] = sum_b sum_{t < Tc_b} spec_b[f][t] * gm_b[m][t],   Tc_b = lengths[b] / hop_length + 1,
 * spec_b the spectrogram of x[b, :lengths[b]] (DC removed over the clip, models.py:38), gm as dmel_backward_fb (models.py:73 with
 * DMEL_FLAG_LOG).  grad_out, out and the spectrogram are never loaded at t >= Tc_b: NaN or inf there reaches nothing.  A length
 * outside 1 ... n_points makes every element of grad_fb NaN (that clip is summed over all n_time frames of a NaN spectrogram).  The
 * batch is cut into the slices of dmel_backward_fb whatever the lengths, and K-blocks without a frame are skipped inside them, so with
 * every length at n_points the result has the bits of dmel_backward_fb_dev / dmel_backward_fb_saved(_dl).  lengths: device, `batch`
 * int32 values read by the kernels when they run.  n_fft: a power of two in 32 ... 16384.  flags: DMEL_FLAG_LOG, DMEL_FLAG_MFMA_BF16X3.
 * dmel_backward_fb_dev_lengths recomputes the spectrogram from x (lambd read on the device and checked against n_fft);
 * dmel_backward_fb_saved_lengths contracts the one the forward saved and, when `tangent` and `dlambd` are given (both or neither),
 * carries d lambd = sum(grad_out * tangent) in the same launch as dmel_backward_fb_saved_dl does (over all frames: the tangent of a pad
 * frame is zero).  NULL handles and pointers, a misaligned grad_fb / scratch: DMEL_ERR_INVALID_ARGUMENT before any device call. */
dmel_status dmel_backward_fb_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                         int32_t n_fft, uint32_t flags, const float* grad_out, const float* out, float* grad_fb,
                                         void* stream);
dmel_status dmel_backward_fb_saved_lengths(dmel_plan* plan, const float* spec, const int32_t* lengths, int32_t batch, int32_t n_fft,
                                           uint32_t flags, const float* grad_out, const float* out, const float* tangent, float* grad_fb,
                                           float* dlambd, void* scratch, void* stream);

/*
 * Backward to the waveform: what torch autograd returns for x.requires_grad through models.py:38 (DC removal),
 * time_frequency.py:43-53 (zero padding, framing, window, rfft, |.|^2), models.py:53 (mel contraction) and, with
 * DMEL_FLAG_LOG, models.py:73.  The reference never differentiates the waveform; provided for completeness
 * (adversarial / saliency uses).  Arguments as dmel_backward_fb; grad_x: device, (batch, n_points) fp32, overwritten.
 * Every transform the forward runs: the wave-FFT kernels up to n_fft 2048, LDS transforms up to 16384, and beyond that -- or for
 * lengths that are not powers of two, i.e. the optimized=False branch (DMEL_FLAG_FULL_WINDOW) on arbitrary clips -- the
 * global-memory FFT / chirp-z transforms in both directions (a correctness path: one (batch, n_time, n_fft) fp32 workspace).
 * Deterministic (overlap-add as an ordered gather).  Asynchronous on `stream`; shares the plan-owned workspace with dmel_backward_fb.
 */
dmel_status dmel_backward_x(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                            const float* grad_out, const float* out, float* grad_x, void* stream);
/* The same through SpectrogramLayer.forward (models.py:171-200; dmel_spectrogram_ex with DMEL_SPEC_REMOVE_DC): grad_spec is the
 * gradient of the power spectrogram, device (batch, n_fft/2+1, n_time) fp32; n_fft and flags as in dmel_spectrogram_ex (any
 * even n_fft the forward accepts). */
dmel_status dmel_backward_x_spec(dmel_plan* plan, const float* x, int32_t batch, float lambd, int32_t n_fft, uint32_t flags,
                                 const float* grad_spec, float* grad_x, void* stream);
/* Both with lambd read on the device (no host read, capturable): `n_fft` is the transform length the forward of this step ran --
 * fixed by a trainable filterbank (dmel_forward_dev_fixed), 2 n_points with DMEL_FLAG_FULL_WINDOW (then `n_fft` is ignored), or the
 * spectrogram layer's explicit length.  A lambd that has left `n_fft` made that forward return NaN and raise its error; the
 * gradient computed here for it is not meaningful either.  With DMEL_FLAG_CHECK_NFFT (dmel_backward_x_dev, n_fft <= 16384, not with
 * DMEL_FLAG_FULL_WINDOW) the call is a no-op on the device unless lambd asks for `n_fft`: the sync-free backward of the
 * optimized=True layer, one call per n_fft its forward launched for (dmel_plan_get_info's n_fft and dmel_lambd_status::guards
 * read right after dmel_forward_dev). */
dmel_status dmel_backward_x_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                const float* grad_out, const float* out, float* grad_x, void* stream);
dmel_status dmel_backward_x_spec_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                     const float* grad_spec, float* grad_x, void* stream);
/* dmel_backward_x / dmel_backward_x_dev over clips of per-clip lengths: the backward of dmel_forward_lengths / dmel_forward_dev_lengths
 * (`lengths` as there: device, read by the kernels only).  With Lc = lengths[b] and Tc = Lc / hop_length + 1, grad_x[b, :Lc] is what
 * dmel_backward_x of a plan with n_points = Lc returns for x[b, :Lc] and grad_out[b, :, :Tc] (the clip's own mean, and the mean of its
 * gradient, over Lc samples); grad_x[b, Lc:] = +0.  x[b, Lc:], grad_out[b, :, Tc:] and out[b, :, Tc:] are never read; tiles of pad frames
 * are not transformed.  A length outside 1 ... n_points makes the row grad_x[b, :] NaN and changes no other row.  grad_out, out and
 * grad_x keep their row strides (n_time, n_points).  Flags: DMEL_FLAG_LOG and, for dmel_backward_x_dev_lengths, DMEL_FLAG_CHECK_NFFT
 * (as dmel_backward_x_dev: one call per n_fft the forward launched for, over a NaN-filled grad_x).  The HTK bank and power-of-two n_fft
 * 32 ... 16384 only (otherwise DMEL_ERR_UNSUPPORTED).  With all lengths at n_points the result is dmel_backward_x's, bit for bit. */
dmel_status dmel_backward_x_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, float lambd, uint32_t flags,
                                    const float* grad_out, const float* out, float* grad_x, void* stream);
dmel_status dmel_backward_x_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                        int32_t n_fft, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);

/* Power spectrogram only, (batch, n_fft/2+1, n_time) fp32 = time_frequency.differentiable_spectrogram
 * (time_frequency.py:32-58, optimized branch) applied per clip; remove_dc != 0 adds models.py:38. */
dmel_status dmel_spectrogram(dmel_plan* plan, const float* x, int32_t batch, float lambd,
                             int32_t remove_dc, float* spec, void* stream);

/*
 * SpectrogramLayer.forward (models.py:171-200) = time_frequency.differentiable_spectrogram per clip
 * (time_frequency.py:32-58) with the tangent d spec / d lambd for its backward.
 *   n_fft   0: derive from lambd (optimized branch, :39); otherwise the transform length to use --
 *           the non-optimized branch (:41,:51) is n_fft = 2 * n_points with DMEL_SPEC_HALF_WINDOW
 *           (torch.stft zero-pads the win_length = n_points window to n_fft on both sides).
 *           Any even length (powers of two up to 16384 on the LDS kernels).
 *   spec, tangent   device, (batch, n_fft/2+1, n_time) fp32; tangent may be NULL.
 */
#define DMEL_SPEC_REMOVE_DC 1u      /* models.py:187: x[idx] - mean(x[idx])                          */
#define DMEL_SPEC_HALF_WINDOW 2u    /* window support = middle half of n_fft                          */
dmel_status dmel_spectrogram_ex(dmel_plan* plan, const float* x, int32_t batch, float lambd, int32_t n_fft,
                                uint32_t flags, float* spec, float* tangent, void* stream);
/* the same with lambd read on the device; n_fft must be given (> 0: a length that does not depend on lambd, e.g. the reference's
 * DSPEC configuration optimized=False, search_spaces.py:71-91): no host read, capturable */
dmel_status dmel_spectrogram_ex_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                    uint32_t flags, float* spec, float* tangent, void* stream);

/* ---- the one exchange step: all-reduce of lambd.grad across GPUs (RCCL over xGMI) -------------------
 * The reference has no distributed code; with the batch sharded over one process per GPU the only cross-GPU
 * datum of this path is the scalar gradient.  These calls issue ncclAllReduce natively on the
 * communicator's own stream, ordered against the caller's stream by events (no host blocking, ~5 us of host
 * time), so that the collective of step k overlaps step k+1.  RCCL is dlopen'ed at first use. */
#define DMEL_COMM_ID_BYTES 128
typedef struct dmel_comm dmel_comm;
/* rank 0 creates the id and ships it to the other ranks by any means (dmel_amd.dist uses torch.distributed) */
dmel_status dmel_comm_unique_id(uint8_t id[DMEL_COMM_ID_BYTES]);
/* collective: every rank calls it with the same id; binds to the current HIP device */
dmel_status dmel_comm_create(const uint8_t id[DMEL_COMM_ID_BYTES], int32_t rank, int32_t world, dmel_comm** comm);
dmel_status dmel_comm_destroy(dmel_comm* comm);
/* in-place SUM of `count` fp32 at device address `buf`, after everything already queued on `stream`;
 * `ticket` (0..63, a ring) names the operation for dmel_comm_wait */
dmel_status dmel_comm_allreduce_async(dmel_comm* comm, float* buf, int32_t count, void* stream, int32_t* ticket);
/* the same all-reduce issued IN `stream` (ordered like a kernel launch: what a step needs when the optimizer update that
 * follows consumes the reduced gradient; capturable into a HIP graph together with the step) */
dmel_status dmel_comm_allreduce(dmel_comm* comm, float* buf, int32_t count, void* stream);
/* make `stream` wait for the all-reduce `ticket`; the host does not block */
dmel_status dmel_comm_wait(dmel_comm* comm, int32_t ticket, void* stream);

/* ---- the same exchange without RCCL: a peer-to-peer mailbox folded into the backward's own kernel ---------------------------
 * ncclAllReduce of 4 bytes costs a kernel of its own and the small-message latency of its ring on the critical path of a
 * ~35 us step (the optimizer update needs the reduced gradient).  With a mailbox the workgroup of dmel_backward's dot kernel
 * that finishes last stores (step, local sum) as one 8-byte granule straight into every rank's inbox (peer memory over xGMI,
 * system-scope stores), polls its own inbox for the other ranks' granules of the same step and adds them in rank order: no
 * extra launch, no ring, the same fp32 result on every rank.  Opt-in; RCCL (dmel_comm_*) stays the default.  Every wait is
 * bounded by wall-clock time (default 120 s, dmel_mailbox_set_timeout_ms): an ordinary straggler is waited for; a rank that never
 * arrives makes the result NaN on the ranks that waited and raises a sticky error word, and the NEXT dmel_forward* / dmel_backward*
 * on a plan the mailbox is attached to returns DMEL_ERR_MAILBOX_TIMEOUT (until dmel_mailbox_error has read the word) instead of
 * hanging the device.
 *   1. every rank: dmel_mailbox_create (allocates its inbox on the current device, returns a 64-byte IPC handle)
 *   2. the handles of all ranks, in rank order, travel by any means (dmel_amd.dist uses torch.distributed) to
 *      dmel_mailbox_connect, which maps the peers' inboxes (hipIpcOpenMemHandle; a handle created by THIS process -- several
 *      ranks of one process, one per device -- is looked up in a process-local registry and its pointer used directly, with
 *      peer access enabled between the two devices)
 *   3. dmel_plan_attach_mailbox(plan, mb): from then on dmel_backward / dmel_backward_scratch on that plan return the SUM over
 *      ranks (every rank must call them the same number of times, as with any collective); mb = NULL detaches.  The mailbox
 *      counts the plans it is attached to: dmel_mailbox_destroy refuses while that count is not zero (a plan that is released
 *      detaches itself).
 *      dmel_mailbox_allreduce does the same exchange for a value already in memory (one tiny launch on `stream`). */
#define DMEL_MAILBOX_HANDLE_BYTES 64
#define DMEL_MAILBOX_MAX_WORLD 16
typedef struct dmel_mailbox dmel_mailbox;
dmel_status dmel_mailbox_create(int32_t rank, int32_t world, dmel_mailbox** mb, uint8_t handle[DMEL_MAILBOX_HANDLE_BYTES]);
dmel_status dmel_mailbox_connect(dmel_mailbox* mb, const uint8_t* handles /* world x DMEL_MAILBOX_HANDLE_BYTES, rank order */);
dmel_status dmel_mailbox_destroy(dmel_mailbox* mb);
dmel_status dmel_mailbox_allreduce(dmel_mailbox* mb, float* buf, void* stream);
/* 0 = no exchange has timed out; otherwise *step / *missing_rank name the first one that did (sticky until read) */
dmel_status dmel_mailbox_error(dmel_mailbox* mb, int32_t* failed, uint32_t* step, int32_t* missing_rank);
/* polls per source rank before an exchange gives up; 0 (the default) = no limit on the count, the wall-clock bound holds */
dmel_status dmel_mailbox_set_spin_limit(dmel_mailbox* mb, uint32_t polls);
/* wall-clock bound of one exchange in milliseconds (default 120 000; 0 = wait for ever, as RCCL does) */
dmel_status dmel_mailbox_set_timeout_ms(dmel_mailbox* mb, uint64_t milliseconds);
dmel_status dmel_plan_attach_mailbox(dmel_plan* plan, dmel_mailbox* mb);

/* torch.optim.Adam's update of an fp32 parameter of the layer on the device (main.py:52-53 builds that optimizer; lambd is one
 * scalar, the trainable filterbank a (n_fft/2+1, n_mels) matrix) as ONE launch on `stream`: param, grad, exp_avg, exp_avg_sq are `n`
 * device floats, `step` one device float that counts the updates (starts at 0; torch's capturable Adam keeps it the same way),
 * `ticket` one zero-initialised device word the launch leaves at zero (needed when n > 1024: several workgroups; may be NULL
 * below).  No host synchronisation, capturable.  The hyper-parameters are doubles, as torch hands them to its own kernel
 * (1 - beta is formed in fp64); the state is fp32.  Arithmetic:
 *   step += 1; g = -grad if maximize; g += weight_decay * param; m += (1 - beta1) (g - m); v = beta2 v + (1 - beta2) g^2;
 *   param -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * Opt-in: torch's own optimizer keeps working on the layer's parameters. */
dmel_status dmel_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* step, uint32_t* ticket, int64_t n,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int32_t maximize, void* stream);

/* Adam fused into the backward (round 5; opt-in).  While attached, every dmel_backward / dmel_backward_ex / dmel_backward_scratch on
 * the plan ends with dmel_adam_step's update of ONE fp32 device scalar -- `param`, i.e. lambd -- by the gradient the call has just
 * written to `dlambd` (after the mailbox all-reduce, if one is attached): the workgroup that finishes the dot product applies it, so
 * the step of train.py:47-49 needs no optimizer launch for lambd.  Same arithmetic and state (exp_avg, exp_avg_sq, step: device
 * floats, as dmel_adam_step) bit for bit.  Meant for steps with one backward per update and no other gradient of the layer read
 * after it (no trainable filterbank, no waveform gradient: their kernels read lambd).  param == NULL detaches.  The pointers must
 * stay valid while attached; the hyper-parameters are taken by value at every call (a captured graph holds those of its capture). */
dmel_status dmel_plan_attach_adam(dmel_plan* plan, float* param, float* exp_avg, float* exp_avg_sq, float* step,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int32_t maximize);

/* ---- PCEN: per-channel energy normalisation behind the mel layers (dmel_amd.PCEN; plan-free, as dmel_adam_step) ---------------------
 * The other standard compression of trainable audio front ends (Wang et al. 2017), next to the forward's fused log(s + eps).  Every
 * row is one (clip[, channel], band) pair of T frames of LINEAR mel power E >= 0 (a forward without DMEL_FLAG_LOG); rows % n_mels == 0
 * and the row's band is row % n_mels -- what a contiguous (..., n_mels, T) tensor gives.  alpha, delta, r, s: n_mels device floats each.
 *   M[0] = E[0];  M[t] = (1 - s) M[t-1] + s E[t]  (t >= 1);   D = eps + M;  a = E D^(-alpha);  u = a + delta;  y = u^r - delta^r
 * A frame with E == 0 gives y == +0.0 exactly (silent rows and the pad frames of the *_lengths forwards stay zero).  The kernels do not
 * clamp the parameters: keep 0 <= alpha <= 1, delta > 0, 0 < r <= 1, 0 < s <= 1 (dmel_amd.PCEN.project_) and eps > 0.
 * dmel_pcen_forward writes y and, when M_or_null is given, the smoother M that dmel_pcen_backward reads (rows * T floats each).
 * dmel_pcen_backward takes g = dL/dy and writes dE = dL/dE (rows * T floats) and / or dparams = (4, n_mels): the gradients of alpha,
 * delta, r, s summed over the frames and rows of each band; either may be NULL and is then neither computed nor written.  dparams needs
 * `scratch`: dmel_pcen_scratch_bytes(rows) bytes (rows * 4 floats, 16-byte aligned) owned by the caller for the duration of the call's
 * work on `stream`.  Two launches at most, no atomics: the same inputs give the same bits.  No host read, capturable.  rows == 0 or
 * T == 0: DMEL_OK, nothing is launched or written. */
size_t dmel_pcen_scratch_bytes(int64_t rows);
dmel_status dmel_pcen_forward(const float* E, int64_t rows, int32_t n_mels, int32_t T, const float* alpha, const float* delta,
                              const float* r, const float* s, float eps, float* y, float* M_or_null, void* stream);
dmel_status dmel_pcen_backward(const float* g, const float* E, const float* M, int64_t rows, int32_t n_mels, int32_t T,
                               const float* alpha, const float* delta, const float* r, const float* s, float eps,
                               float* dE_or_null, float* dparams_or_null, float* scratch, void* stream);

/* ---- BandNorm: length-aware per-band standardisation behind the mel layers (dmel_amd.BandNorm; plan-free, as PCEN) ------------------
 * What a consumer applies first to a mel image -- batch normalisation over the mel bins (panns.py:169-172) or per-clip mean / variance
 * normalisation -- with the statistics taken over the VALID frames only.  Every row is one (clip[, channel], band) triple of T fp32 frames:
 * band = row % n_mels, clip = row / rows_per_clip (rows_per_clip = channels * n_mels; rows a multiple of it) -- what a contiguous
 * (B[, C], n_mels, T) tensor gives.  frame_lengths: rows / rows_per_clip device int32 values Tc, read by the kernels only (what
 * layer.frame_lengths(lengths) returns); NULL: every clip has T valid frames.  The valid frames of a clip are t < Tc.
 *   y = (s - mu) rstd weight[band] + bias[band]  on valid frames,  rstd = 1 / sqrt(var + eps), var the biased variance;  +0.0 on pad frames
 * weight / bias: n_mels device floats each, or NULL (1 and 0).  batch_stats = 0: mu and var of each row over its own valid frames
 * (utterance-level CMVN; no buffers, training is ignored).  batch_stats = 1, training = 1: mu and var of band m over every valid frame of
 * every row of that band; running_mean / running_var (n_mels floats each, both or neither) move by nn.BatchNorm2d's rule
 * r = (1 - momentum) r + momentum v with the unbiased variance n / (n - 1) -- running_var left alone when the band has fewer than two valid
 * frames, both when it has none -- and *num_batches_tracked (one int64, may be NULL) advances by one, all on the device.  batch_stats = 1,
 * training = 0: the running buffers are the statistics and nothing is updated.
 * `stats` receives the (mu, rstd) pairs in fp64 that dmel_bandnorm_backward reads: 2 * rows doubles with batch_stats = 0, 2 * n_mels with
 * batch_stats = 1; 16-byte aligned.  `scratch`: dmel_bandnorm_scratch_bytes(rows, n_mels) bytes (16-byte aligned) owned by the caller for
 * the duration of the call's work on `stream`; the forward needs it with batch_stats = 1 and training = 1 only, the backward always.
 * dmel_bandnorm_backward takes g = dL/dy and, with yh = (s - mu) rstd, writes  ds = weight rstd (g - mean(g) - yh mean(g yh))  -- the means
 * over the statistic's own population; with batch_stats = 1 and training = 0  ds = weight rstd g  --, dweight[band] = sum g yh and
 * dbias[band] = sum g over the valid frames; each may be NULL and is then neither computed nor written.  ds is +0.0 on pad frames.
 * s and g are never read at a pad frame.  A frame_lengths[b] outside 1 ... T makes every frame of that clip's rows NaN in y and ds; the clip
 * contributes nothing to batch statistics, running buffers or parameter gradients.  Sums are accumulated in fp64 and combined in a fixed
 * order: no atomics, the same inputs give the same bits.  No host read, capturable.  Three launches at most per call.  rows == 0 or
 * T == 0: DMEL_OK, nothing is launched or written. */
size_t dmel_bandnorm_scratch_bytes(int64_t rows, int32_t n_mels);
dmel_status dmel_bandnorm_forward(const float* s, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T,
                                  const int32_t* frame_lengths_or_null, const float* weight_or_null, const float* bias_or_null,
                                  int32_t batch_stats, int32_t training, double eps, double momentum, float* running_mean,
                                  float* running_var, int64_t* num_batches_tracked_or_null, float* y, double* stats, void* scratch,
                                  void* stream);
dmel_status dmel_bandnorm_backward(const float* g, const float* s, const double* stats, int64_t rows, int32_t n_mels, int64_t rows_per_clip,
                                   int32_t T, const int32_t* frame_lengths_or_null, const float* weight_or_null, int32_t batch_stats,
                                   int32_t training, float* ds_or_null, float* dweight_or_null, float* dbias_or_null, void* scratch,
                                   void* stream);

/* ---- SpecMask: length-aware SpecAugment stripes behind the mel layers (dmel_amd.SpecMask; plan-free, as PCEN and BandNorm) ------------
 * What a training loop applies behind the normalisation (panns.py:141-142, 174-176: time and frequency masking with iid_masks=True), drawn
 * over the VALID frames of a zero-padded batch and pinned to the bit.  An image is one (clip, channel) pair of a contiguous
 * (B[, C], n_mels, T) tensor: image i = clip * channels + channel, n_mels rows of T elements.  Every image draws n_time time stripes, then
 * n_freq frequency stripes, independently of every other image; n_time + n_freq <= 8, either may be 0.  All of it is integer arithmetic.
 *   random words   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key (seed & 0xffffffff,
 *                  seed >> 32), counter (calls & 0xffffffff, calls >> 32, i, j); stripe k of the image (time stripes first) takes block
 *                  j = k / 2 and the word pair (w[2 (k % 2)], w[2 (k % 2) + 1]) = (w_a, w_b).  rng_state = (seed, calls): two int64 on the device.
 *   a stripe       on an axis of `size` positions with cap = min(param, size): width = mulhi32(w_a, cap), lo = mulhi32(w_b, size - width),
 *                  hi = lo + width -- 0 <= lo <= hi <= size - 1, width <= cap - 1 (0 when cap == 0): torchaudio's mask_along_axis_iid support.
 *   time stripes   size = Tc = frame_lengths[clip] (NULL: T), param = min(time_param, Tc * time_permille / 1000) in integer division
 *   freq stripes   size = n_mels, param = freq_param
 * dmel_specmask_draw writes `stripes`: images * (n_time + n_freq) * 2 int32 values, the [lo, hi) pairs; with advance = 1 it then stores
 * calls + 1 (after every draw of the call has read calls; one workgroup, a barrier, a plain store: no atomics, no host read, so a captured
 * call draws fresh stripes on every replay); advance = 0 draws at calls and leaves it.  A frame_lengths[b] outside 1 ... T leaves that clip's
 * table rows zero.  images == 0, T == 0 or n_time + n_freq == 0: DMEL_OK, nothing is launched and calls stays.
 * dmel_specmask_apply moves rows x T elements of 4 bytes (elem_bf16 = 0) or 2 (elem_bf16 = 1) from s to y, never converting them:
 *   y = fill  on a valid frame t < Tc that lies in one of the image's time stripes or whose band lies in one of its frequency stripes
 *       (fill rounded to bf16, to nearest even, for 2-byte elements);  y = s bit for bit elsewhere -- every pad frame t >= Tc included.
 * clip = row / rows_per_clip, rows_per_clip = channels * n_mels, rows a multiple of it.  A frame_lengths[b] outside 1 ... T makes every
 * element of that clip's rows NaN.  The gradient is the same call on the cotangent with fill = +0.0 and the table the forward wrote.
 * s needs its element's alignment only (16-byte accesses are used where s and y sit alike inside a 16-byte granule, chosen per image from
 * the addresses); y must be 16-byte aligned.  One launch; rows == 0 or T == 0: DMEL_OK, nothing is launched.  s and y must not overlap. */
dmel_status dmel_specmask_draw(int64_t images, int32_t channels, int32_t n_mels, int32_t T, const int32_t* frame_lengths_or_null,
                               int32_t time_param, int32_t time_permille, int32_t n_time, int32_t freq_param, int32_t n_freq,
                               int64_t* rng_state, int32_t advance, int32_t* stripes, void* stream);
dmel_status dmel_specmask_apply(const void* s, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T,
                                const int32_t* frame_lengths_or_null, const int32_t* stripes, int32_t n_time, int32_t n_freq,
                                int32_t elem_bf16, float fill, void* y, void* stream);

/* ---- Deltas: length-aware delta and delta-delta channels behind the mel layers (dmel_amd.Deltas; plan-free, as PCEN, BandNorm, SpecMask) --
 * The "velocity" and "acceleration" channels of the mel image, with the stencil's replicate edge at each clip's OWN last valid frame (a
 * stencil over a zero-padded batch reads log(1e-10) = -23.03 behind a short clip's last frame instead).  s is rows x n_time fp32, a row is
 * one (clip, channel, band) triple of a contiguous (B, C, M, T) tensor: rows = B C M, rows_per_clip = C M, clip = row / rows_per_clip,
 * Tc = frame_lengths[clip] (NULL: n_time).  win_length is 3, 5, 7 or 9, n = (win_length - 1) / 2, denom = n (n + 1) (2 n + 1) / 3
 * (2, 10, 28, 60); order is 1 or 2.
 *   for t <  Tc:   d[t]  = ( sum_{j = 1 .. n}  j * ( x[min(t + j, Tc - 1)] - x[max(t - j, 0)] ) ) / denom
 *                  dd[t] = the same formula applied to the STORED fp32 row d[0 .. Tc - 1]
 *   for t >= Tc:   d[t] = dd[t] = +0.0
 * With Tc = n_time this is torchaudio.functional.compute_deltas(win_length, mode="replicate"), applied once and twice.  The antisymmetric
 * form -- a difference first, j times it second -- is part of the specification: a constant row, Tc = 1 and a row of silent frames give
 * +0.0 bit for bit in both channels.  Sums are fp32 or wider in a fixed order (here: fp64, scaled by 1 / denom, rounded to fp32 once); dd is
 * formed from d as rounded to fp32, so dd is the call applied to its own d bit for bit.
 * y has G = include_static + order groups per clip, in torch.cat([s, d, dd], dim=1) order: the output row of input row r in group o is
 * (r / rows_per_clip) * G * rows_per_clip + o * rows_per_clip + r % rows_per_clip.  Group 0 is s moved as words when include_static = 1:
 * every frame, pad frames, NaN payloads and -0.0 included; then d; then dd (order = 2).  s is never loaded at a pad frame for d and dd.
 * A frame_lengths[b] outside 1 ... n_time makes every output row of clip b NaN, the static group included; other clips are untouched.
 * dmel_deltas_backward: g is the cotangent of y (G rows x n_time per input row, the same layout), ds is rows x n_time.  With D the Tc x Tc
 * matrix of the clamped stencil (out-of-range taps fold onto frames 0 and Tc - 1):  ds = g_static + D^T (g_d + D^T g_dd)  on t < Tc
 * (g_static = 0 without include_static, g_dd = 0 with order = 1); on pad frames ds = g_static bit for bit, +0.0 without the static group;
 * g_d and g_dd are never loaded at a pad frame; an invalid length gives a NaN clip.  Every ds[t] is gathered by its own lane: no atomics, two
 * runs give the same bits.  The stage is linear: the backward needs frame_lengths only.
 * s and g need their element's alignment only; y and ds must be 16-byte aligned.  One launch each, no host read, capturable; rows == 0 or
 * n_time == 0: DMEL_OK, nothing is launched.  Refused with DMEL_ERR_INVALID_ARGUMENT before any device is touched: a NULL s, g, y or ds,
 * rows_per_clip that does not divide rows, another win_length or order, a misaligned output.  Input and output must not overlap. */
dmel_status dmel_deltas_forward(const float* s, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                int32_t win_length, int32_t order, int32_t include_static, float* y, void* stream);
dmel_status dmel_deltas_backward(const float* g, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                 int32_t win_length, int32_t order, int32_t include_static, float* ds, void* stream);

/* ---- StatsPool: length-aware mean / std / max pooling over time behind the mel layers (dmel_amd.StatsPool; plan-free, as Deltas) ----------
 * The stage that ends the length-aware chain: (B, C, M, T) plus frame lengths become a fixed-size (B, S C, M) -- the "statistics pooling"
 * of x-vector style heads -- from each row's own VALID frames only.  s is rows x n_time fp32, a row is one (clip, channel, band) triple of
 * a contiguous (B, C, M, T) tensor: rows = B C M, rows_per_clip = C M, clip = row / rows_per_clip, Tc = frame_lengths[clip] (NULL: n_time).
 * `which` selects the statistics: bit 0 mean, bit 1 std, bit 2 max; 1 ... 7; S = popcount(which).  For 1 <= Tc <= n_time:
 *   mean   mu = (sum_{t < Tc} s[t]) / Tc, the sum and the quotient in fp64, rounded to fp32 once for y
 *   std    sd = sqrt(m2 / Tc + eps),  m2 = sum_{t < Tc} (s[t] - mu)^2: the mean first, the squared deviations from the UNROUNDED fp64 mu
 *          second (never E[x^2] - mu^2); the biased variance, as in BandNorm; all in fp64, rounded once.  eps > 0 keeps the gradient finite
 *          on a constant row.  A constant row and Tc = 1 give exactly (float)sqrt((double)eps): the fp64 sum of Tc equal fp32 values and
 *          its quotient by Tc are exact
 *   max    s[am] moved as a word, am chosen by an order that is associative and commutative (the reduction tree cannot change it): a NaN
 *          beats a non-NaN; then the larger value wins; then the lower t wins -- -0.0 and +0.0 tie, so the lower t's bits are stored
 * y has S groups per clip in the fixed order mean, std, max -- torch.cat([mean, std, max], dim=1) of three (B, C, M) tensors: the element of
 * input row r in group o is (r / rows_per_clip) * S * rows_per_clip + o * rows_per_clip + r % rows_per_clip (Deltas' group layout).
 * stats_or_null: 2 * rows doubles, the unrounded pairs (mu, sd), 16-byte aligned; argmax_or_null: rows int32 values am (-1 for a clip with
 * an invalid length); each is written when it is not NULL, whatever `which` selects (without std, sd is formed with eps where eps > 0, else 0).
 * s is never loaded at a pad frame, and a 64-frame chunk without a valid frame is not visited.  A frame_lengths[b] outside 1 ... n_time makes
 * every output element of clip b NaN; other clips are untouched.  Sums run in a fixed order, no atomics: the same inputs give the same bits,
 * and a row's result depends on its own Tc values and (n_time, Tc) only, not on where the row sits in the launch.
 * dmel_statspool_backward: g has y's layout, ds is rows x n_time.  On t < Tc
 *   ds[t] = g_mean / Tc + g_std (s[t] - mu) / (Tc sd) + [t == am] g_max
 * in fp64 from the stored (mu, sd) and am, rounded once; a group that is not selected contributes nothing; ds = +0.0 on pad frames; an
 * invalid length gives a NaN clip.  s is read only when std is selected and never at a pad frame.  With std alone a constant row gives
 * ds == 0 everywhere.  Element-wise: no reduction.
 * s, g, y and ds need their element's alignment only.  One launch each, no host read, capturable; rows == 0 or n_time == 0: DMEL_OK,
 * nothing is launched.  Refused with DMEL_ERR_INVALID_ARGUMENT before any device is touched: a NULL s, g, y or ds, rows_per_clip that does
 * not divide rows, `which` outside 1 ... 7, eps <= 0 or NaN when std is selected, a misaligned stats, a backward that selects std without
 * s and stats or max without argmax. */
dmel_status dmel_statspool_forward(const float* s, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                   int32_t which, double eps, float* y, double* stats_or_null, int32_t* argmax_or_null, void* stream);
dmel_status dmel_statspool_backward(const float* g, const float* s_or_null, const double* stats_or_null, const int32_t* argmax_or_null,
                                    int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null, int32_t which,
                                    float* ds, void* stream);

/* ---- AttentivePool: length-aware attentive statistics pooling over time behind the mel layers (dmel_amd.AttentivePool; plan-free) ---------
 * The x-vector / ECAPA "attentive statistics pooling" with a softmax that knows the lengths: a scorer of the caller's gives every frame a
 * logit, a softmax over the clip's VALID frames turns logits into weights, and the clip vector is the weighted mean and the weighted standard
 * deviation.  (torch.softmax(a, -1) over a zero-padded batch hands every pad frame a share of the weight.)
 * Inputs   s: contiguous (B, C, M, T) fp32 seen as rows = B C M rows of n_time frames, R = rows_per_clip = C M rows per clip;
 *          a: contiguous (B, A, T) fp32 logits, A = logit_rows_per_clip >= 1 divides R, and row r of a clip reads logit row r / (R / A):
 *             A = 1 one attention for the whole clip, A = C one per channel, A = R one per band (ECAPA's channel-dependent form);
 *          Tc = frame_lengths[clip] (NULL: n_time), clip = row / R;
 *          which: bit 0 mean, bit 1 std; 1 ... 3; S = popcount(which);  eps finite and > 0, asked for only when std is selected.
 * Per (clip, logit row), over t < Tc only:
 *          m = max a[t];  p[t] = exp((double)a[t] - (double)m);  Z = sum p[t];  w[t] = p[t] / Z
 * Per row: mu  = (sum p[t] s[t]) / Z            evaluated around the row's first frame, s[0] + (sum p[t] (s[t] - s[0])) / Z: the same
 *                                              number, and a constant row has mu == c and var == 0 exactly in fp64 as well
 *          var = (sum p[t] (s[t] - mu)^2) / Z      the mean first, the deviations from the UNROUNDED fp64 mu second
 *          sd  = sqrt(var + eps)
 * Sums are in fp64; each of mean and std is rounded to fp32 once.
 * Output   y is (B, S C, M) in torch.cat([mean, std], dim=1) order: the element of input row r in group o is
 *          (r / R) * S * R + o * R + r % R (StatsPool's group layout).
 * Optional outputs, needed only when a backward will run, both given or both NULL, both 16-byte aligned:
 *          stats: (rows, 2) fp64, the pairs (mu, var) -- var, not sd: the backward needs var, and sd^2 - eps cancels;
 *          norm:  (B A, 2) fp64, the pairs (m, Z).
 * dmel_attnpool_backward, from g (y's layout), s, a, stats and norm; with d = s[t] - mu, on t < Tc:
 *          ds[r, t] = w[t] (g_mean[r] + g_std[r] d / sd[r])
 *          da[t]    = w[t] sum_{r in the logit row's group} (g_mean[r] d + g_std[r] (d^2 - var[r]) / (2 sd[r]))
 * da is the softmax Jacobian with its mean term sum_u w[u] q[u] taken in closed form from the stored pairs (sum_u w[u] d[u] = 0 and
 * sum_u w[u] d[u]^2 = var): no second reduction over frames.  Both in fp64, rounded once; w[t] is recomputed as exp(a[t] - m) / Z;
 * sd = sqrt(var + eps) from the stored var and the eps of the forward, which the backward therefore takes as well; the g of a statistic
 * that is not selected is not read.
 * Rules shared with the stages in front: s, a and g are never loaded at a pad frame; ds and da are +0.0 on every pad frame; a 64-frame chunk
 * without a valid frame is not visited; a frame_lengths[b] outside 1 ... n_time makes every element of clip b NaN in y, ds, da, stats and
 * norm, and other clips keep their bits; lengths are read on the device only; no host read, no atomics; two runs give the same bits; a
 * clip's bits do not depend on what it is batched with; rows are limited to 2^31 - 1 per launch.  A row that is a constant c over its
 * valid frames gives mean == c and std == (float)sqrt((double)eps) bit for bit.  A valid frame whose logit is -inf, next to finite logits,
 * has weight exactly 0 and ds, da of exactly zero there; other non-finite logits follow IEEE through the formulas and are not specified.
 * s, a, g, y, ds and da need their element's alignment only.  One launch each, capturable; rows == 0 or n_time == 0: DMEL_OK, nothing is
 * launched.  Refused with DMEL_ERR_INVALID_ARGUMENT before any device is touched: a NULL or misaligned s, a, g, y, ds or da,
 * rows_per_clip that does not divide rows, logit_rows_per_clip that does not divide rows_per_clip, `which` outside 1 ... 3, eps <= 0 or
 * NaN when std is selected, a misaligned stats or norm, one of the two without the other, a backward without them. */
dmel_status dmel_attnpool_forward(const float* s, const float* a, int64_t rows, int64_t rows_per_clip, int64_t logit_rows_per_clip,
                                  int32_t n_time, const int32_t* frame_lengths_or_null, int32_t which, double eps, float* y,
                                  double* stats_or_null, double* norm_or_null, void* stream);
dmel_status dmel_attnpool_backward(const float* g, const float* s, const float* a, const double* stats, const double* norm, int64_t rows,
                                   int64_t rows_per_clip, int64_t logit_rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                   int32_t which, double eps, float* ds, float* da, void* stream);

/* ---- the multi-window layer: K trainable window widths as K output channels (dmel_amd.MultiWindowMelSpectrogram) ------------------
 * Channel k of (batch, K, n_mels, n_time) is what dmel_forward* computes for lambd[k], bit for bit; 1 <= K <= 8, every channel's n_fft in
 * 32 ... 16384 (the fused kernel).  One launch per DISTINCT n_fft covers all the channels that need it.  out and tangent are (batch, K, M, T);
 * flags: DMEL_FLAG_LOG, DMEL_FLAG_OUT_BF16.  scratch: dmel_scratch_bytes_multi(plan, batch, K) bytes owned by the caller for the forward and
 * the dmel_backward_multi that consumes its tangent (required).
 * dmel_forward_multi takes the K values from the host (channels grouped by n_fft; a value outside the range: DMEL_ERR_UNSUPPORTED).
 * dmel_forward_multi_dev reads them on the device as dmel_forward_dev does, with one host picture per channel: each channel's launches and
 * guards are chosen as dmel_forward_dev would, and their union is issued.  A channel that no launch covered is NaN (the others are
 * untouched) and the next call returns DMEL_ERR_LAMBD_TRACKING naming it.  The first call (and the first after a reset) reads the K values
 * once, blocking.  dmel_plan_lambd_reset forgets every channel. */
size_t dmel_scratch_bytes_multi(const dmel_plan* plan, int32_t batch, int32_t channels);
dmel_status dmel_forward_multi(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels, uint32_t flags,
                               double eps, void* out, float* tangent, void* scratch, void* stream);
dmel_status dmel_forward_multi_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels, uint32_t flags,
                                   double eps, void* out, float* tangent, void* scratch, void* stream);
/* dmel_forward_multi(_dev) over clips of per-clip lengths (zero-padded batches): lengths as dmel_forward_lengths takes them (device, `batch`
 * int32 values, read by the kernels only), and that function's semantics per channel -- channel k is what dmel_forward_lengths computes for
 * lambd[k], bit for bit: the clip's own mean, pad frames (0, or log(0 + eps); zero tangent) from lengths[b] / hop_length + 1 on, tiles of pad
 * frames not transformed, x[b, lengths[b]:] never read, a length outside 1 ... n_points NaN in every channel of that clip.  A channel that no
 * launch covered is NaN whatever the lengths are.  Flags, scratch, launch choice, guards, per-channel pictures, DMEL_ERR_LAMBD_TRACKING and
 * dmel_plan_last_multi_launch are dmel_forward_multi(_dev)'s; dmel_backward_multi consumes the tangent.  NULL handles and pointers:
 * DMEL_ERR_INVALID_ARGUMENT before any device call. */
dmel_status dmel_forward_multi_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                       int32_t channels, uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
dmel_status dmel_forward_multi_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                           int32_t channels, uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
/* dlambd[k] (= or += with accumulate) sum over clips of grad_out[:, k] . tangent[:, k], K values in ONE deterministic launch (fp64
 * accumulation, fixed-order combine; bf16 gradients widened exactly).  Not with an attached mailbox or fused Adam. */
dmel_status dmel_backward_multi(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int32_t batch, int32_t channels,
                                int32_t accumulate, float* dlambd, void* scratch, void* stream);
/* dmel_plan_lambd_status for channel `channel` of the multi-window forward (calls counts every dmel_forward_dev* / _multi_dev call) */
dmel_status dmel_plan_lambd_status_channel(dmel_plan* plan, int32_t channel, dmel_lambd_status* status);
/* The launch choice of dmel_forward_multi_dev as a pure function: the union over channels of dmel_decide_launch(lambd[k], rate[k],
 * stale_forwards), `count` entries in ascending n_fft, channel_masks[i] bit k = channel k needs n_ffts[i].  Arrays of 3 x channels entries. */
dmel_status dmel_decide_launch_multi(const float* lambd, const float* rate, int32_t channels, float stale_forwards, int32_t* n_ffts,
                                     uint32_t* channel_masks, int32_t* count);
/* Gradient w.r.t. the waveform of the multi-window layer: grad_x (batch, n_points) = the sum, in ascending channel order from 0, of what
 * dmel_backward_x(_dev) gives for each channel, bit for bit.  grad_out and out are (batch, K, M, T) fp32; flags: DMEL_FLAG_LOG only (it
 * needs out, the saved fp32 log output).  One wave-FFT launch per distinct n_fft <= 2048 for all the channels that need it, per-channel
 * launches on the LDS path (n_fft 4096 ... 16384, or a shape the wave kernel does not fit), then ONE deterministic combine launch.
 * dmel_backward_x_multi takes the K values from the host.  dmel_backward_x_multi_dev reads them on the device and takes the launch list
 * of the forward whose gradient this is, (n_ffts, channel_masks, count) as dmel_plan_last_multi_launch returned it right after that
 * forward: ascending powers of two in 32 ... 16384, every channel in some mask, no bit at or above `channels`.  Every launch of a channel
 * returns at once unless lambd[k] asks for its n_fft; a channel that none matches makes grad_x NaN (its forward output is NaN too).
 * The workspace is plan-owned; an eager call sizes it for every channel's n_fft / 2, n_fft and 2 n_fft, so that a later capture near an
 * n_fft boundary needs no growth (a capture that would need some: DMEL_ERR_INVALID_ARGUMENT, run once eagerly). */
dmel_status dmel_backward_x_multi(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels,
                                  uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);
dmel_status dmel_backward_x_multi_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels,
                                      const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count, uint32_t flags,
                                      const float* grad_out, const float* out, float* grad_x, void* stream);
/* dmel_backward_x_multi(_dev) over clips of per-clip lengths, the backward of dmel_forward_multi(_dev)_lengths: gx_k is what
 * dmel_backward_x(_dev)_lengths gives for lambd[k], bit for bit.  lengths: `batch` device integers, read when the kernels run (a captured call
 * takes new values on replay).  grad_x[b, lengths[b]:] = +0.0; a length outside 1 ... n_points makes row b NaN and changes no other row;
 * samples past a clip, and grad_out / out of its pad frames, are never read; pad tiles and pad pairs are not transformed and the combine
 * (dmel_xgrad_combine_multi_len_kernel) reads nothing of them from the plan-owned workspace.  lengths == NULL: DMEL_ERR_INVALID_ARGUMENT;
 * every other rule is dmel_backward_x_multi(_dev)'s. */
dmel_status dmel_backward_x_multi_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                          int32_t channels, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);
dmel_status dmel_backward_x_multi_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                              int32_t channels, const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count,
                                              uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);
/* What the most recent dmel_forward_multi(_dev), dmel_forward_band(_dev) or their _lengths forms on this plan issued (host bookkeeping, captured calls included):
 * count entries in ascending n_fft with their channel masks; arrays of 24 (3 x 8) entries.  count = 0 before the first such call. */
dmel_status dmel_plan_last_multi_launch(dmel_plan* plan, int32_t* n_ffts, uint32_t* channel_masks, int32_t* count);

/* ---- the band-split layer: a trainable window width per GROUP OF MEL BANDS inside one image (dmel_amd.BandSplitMelSpectrogram) ----------
 * out and tangent are (batch, 1, n_mels, n_time), the scalar layer's shape.  band_edges: K + 1 HOST integers 0 = e_0 < e_1 < ... < e_K =
 * n_mels (validated, taken by value: the array may be reused at once); rows e_k ... e_{k+1} - 1 are what dmel_forward* computes for
 * lambd[k], bit for bit, and no other row is computed into memory.  Everything else -- K, the n_fft range, flags, scratch
 * (dmel_scratch_bytes_multi(plan, batch, K), required), one launch per DISTINCT n_fft, host values (dmel_forward_band) or device values with
 * one host picture per channel, guards, dmel_plan_lambd_status_channel, DMEL_ERR_LAMBD_TRACKING -- is dmel_forward_multi(_dev)'s.  A channel no
 * launch covered makes ITS rows NaN and leaves the other groups' rows untouched.  A plan serves one of the two layers: they share the per-channel
 * lambd pictures.  NULL / invalid band_edges, K outside 1 ... 8: DMEL_ERR_INVALID_ARGUMENT before any device work. */
dmel_status dmel_forward_band(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels, const int32_t* band_edges,
                              uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
dmel_status dmel_forward_band_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels, const int32_t* band_edges,
                                  uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream);
/* dmel_forward_band(_dev) over clips of per-clip lengths: rows e_k ... e_{k+1} - 1 are those rows of what dmel_forward_lengths computes for
 * lambd[k], bit for bit; pad rows and the NaN rows of an invalid length are written by each channel into its own rows only.  Everything else as
 * dmel_forward_multi(_dev)_lengths and dmel_forward_band(_dev). */
dmel_status dmel_forward_band_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                      int32_t channels, const int32_t* band_edges, uint32_t flags, double eps, void* out, float* tangent,
                                      void* scratch, void* stream);
dmel_status dmel_forward_band_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                          int32_t channels, const int32_t* band_edges, uint32_t flags, double eps, void* out, float* tangent,
                                          void* scratch, void* stream);
/* dlambd[k] (= or += with accumulate) sum over clips and rows e_k ... e_{k+1} - 1 of grad_out . tangent, both (batch, 1, n_mels, n_time): K
 * values in ONE deterministic launch (fp64 accumulation, workgroups dealt to the groups in proportion to their rows, fixed-order combine; bf16
 * gradients widened exactly).  Not with an attached mailbox or fused Adam. */
dmel_status dmel_backward_band(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int32_t batch, int32_t channels,
                               const int32_t* band_edges, int32_t accumulate, float* dlambd, void* scratch, void* stream);
/* Gradient w.r.t. the waveform of the band-split layer.  grad_out and out are ONE (batch, 1, n_mels, n_time) fp32 image; with G_k = grad_out
 * whose rows outside e_k ... e_{k+1} - 1 are +0.0, grad_x (batch, n_points, 16-byte aligned) = 0 + gx_0 + ... + gx_{K-1} in ascending
 * channel order, gx_k what dmel_backward_x(_dev) gives for lambd[k] and G_k, bit for bit -- dmel_backward_x_multi(_dev) for the
 * (batch, K, M, T) cotangent whose channel k is G_k, without that tensor: a channel loads only its own rows (dmel_xgrad_wave_band_kernel; on
 * the LDS path, n_fft 4096 ... 16384, dmel_xgrad_band_stage_kernel writes the masked rows out for the scalar frames kernel).  Rows outside a
 * channel's range are never read: in log mode they hold other channels' output.  Arguments, launch list (dmel_plan_last_multi_launch right
 * after the dmel_forward_band_dev whose gradient this is), NaN for a channel no launch matched, plan-owned workspace and the capture rule are
 * dmel_backward_x_multi(_dev)'s; band_edges as dmel_forward_band's.  NULL / invalid arguments: DMEL_ERR_INVALID_ARGUMENT before any device work. */
dmel_status dmel_backward_x_band(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels,
                                 const int32_t* band_edges, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);
dmel_status dmel_backward_x_band_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels,
                                     const int32_t* band_edges, const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count,
                                     uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);
/* dmel_backward_x_band(_dev) over clips of per-clip lengths, the backward of dmel_forward_band(_dev)_lengths: gx_k is what
 * dmel_backward_x(_dev)_lengths gives for lambd[k] and G_k, bit for bit (dmel_xgrad_wave_band_len_kernel: a channel's own rows, the clip's own
 * frames).  lengths and the clip rules as dmel_backward_x_multi(_dev)_lengths; everything else as dmel_backward_x_band(_dev). */
dmel_status dmel_backward_x_band_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                         int32_t channels, const int32_t* band_edges, uint32_t flags, const float* grad_out, const float* out,
                                         float* grad_x, void* stream);
dmel_status dmel_backward_x_band_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                             int32_t channels, const int32_t* band_edges, const int32_t* n_ffts, const uint32_t* channel_masks,
                                             int32_t count, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream);

/* Introspection for tests / benchmarks */
typedef struct dmel_plan_info {
    int32_t n_fft;             /* of the most recent forward                                */
    int32_t n_freqs;
    int32_t n_time;
    int32_t frames_per_tile;   /* frames one workgroup of the fused kernel produces         */
    int32_t grid_fwd;          /* workgroups of the fused forward kernel                    */
    int32_t fb_blocks;         /* non-zero 4x16 filterbank blocks fed to the MFMA loop      */
    int32_t fb_blocks_dense;   /* the same count for a dense matrix                         */
    int32_t lds_bytes;         /* dynamic LDS of the fused kernel                           */
    int32_t kernel_path;       /* 0 = wave-FFT + MFMA kernel (32 <= n_fft <= 16384), 1 = direct-DFT kernel (n_fft < 32), 3 = global-memory FFT / chirp-z (dmel_big.hip) */
    /* ABI 5 (round 6): which contraction the most recent fused forward ran, and its size -- what an MFMA-flop count has to be taken from */
    int32_t contraction;       /* 0 = banded / dense 16x16x4 fp32 tiles (fb_blocks of them per 16-row tile), 1 = wave-local 4x4x1 fp32 (kTrainW:
                                  wl_steps instructions per wave, 16 blocks of 4 x 4 each), 2 = dense bf16x3 (kTrainH), -1 = no MFMA stage */
    int32_t wl_steps;          /* contraction 1: v_mfma_f32_4x4x1 instructions every wave issues per tile (all phases)     */
} dmel_plan_info;
dmel_status dmel_plan_get_info(const dmel_plan* plan, dmel_plan_info* info);

/* Per-kernel device timing with HIP events recorded on the caller's stream around each launch
 * (bench.py's roofline line).  Off by default; recording stops silently after 16384 launches. */
typedef struct dmel_profile {
    double prep_ms;            /* sum over launches: partial sums + window tables kernel    */
    double fwd_ms;             /* fused forward kernel                                      */
    double bwd_ms;             /* both kernels of dmel_backward                             */
    int32_t prep_launches, fwd_launches, bwd_launches;
} dmel_profile;
dmel_status dmel_plan_set_profiling(dmel_plan* plan, int32_t enable);
/* Waits for the recorded events, returns the sums since the last call and resets them. */
dmel_status dmel_plan_get_profile(dmel_plan* plan, dmel_profile* profile);

#ifdef __cplusplus
}
#endif
#endif /* DMEL_H */
