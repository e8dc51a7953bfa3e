// dmel_api.cpp -- host side of libdmel_hip.so: the C ABI of include/dmel.h.
//
// Owns everything that is not a kernel or table arithmetic: per-plan workspace, argument checking and kernel dispatch.  No torch types, no oracle
// code.  In order: tables (the builders of dmel_tables.h compute them on the host -- the HTK mel filterbank of models.py:42-48, its packing into
// non-zero MFMA B-fragments, twiddles, the wave-local schedule --; upload() is the one place that allocates their device copies and records them with
// their owner; build_tables chooses the bank, calls, uploads); scratch and workspaces; the forward
// (FwdCall describes a call, launch_forward_n issues it for one n_fft through forward_big / _naive / _fused); the host steps of the sync-free lambd
// tracking around dmel_lamtrack.h, once for K tracked values; the extern "C" entry points, which check, fill a call description by name and hand it on.
#include "../../include/dmel.h"
#include "dmel_kernels.h"
#include "dmel_lamtrack.h"
#include "dmel_stage.h"
#include "dmel_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

thread_local std::string g_err;

dmel_status fail(dmel_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}
}  // namespace

namespace dmel {
dmel_status set_error(dmel_status st, const std::string& msg) { return fail(st, msg); }   // for dmel_comm.cpp
bool mailbox_args(const dmel_mailbox* mb, MailboxArgs* out);                              // dmel_comm.cpp
int mailbox_device(const dmel_mailbox* mb);
void mailbox_attach_count(dmel_mailbox* mb, int delta);
unsigned long long mailbox_peek_error(const dmel_mailbox* mb);
}

namespace {

#define DMEL_HIP(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(DMEL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// Device copies of host tables.  upload() is the one place that allocates them: it records every allocation with its owner, which
// frees what was uploaded into it.  A second pointer to an uploaded table (tw1p == tw1) is an alias, not an owner.
struct DeviceTables {
    std::vector<void*> owned;
    void release() { for (void* q : owned) (void)hipFree(q); owned.clear(); }
};

// *dev = a device copy of `host`, at least min_elems elements long (elements beyond host.size() are left unwritten)
template <class T, class D> dmel_status upload(DeviceTables* owner, const std::vector<T>& host, D** dev, size_t min_elems = 0)
{
    if (host.empty() && min_elems == 0) return DMEL_OK;       // no such table: the pointer stays as it is
    void* d = nullptr;
    DMEL_HIP(hipMalloc(&d, std::max(host.size(), min_elems) * sizeof(T)));
    owner->owned.push_back(d);
    *dev = static_cast<D*>(d);
    if (!host.empty()) DMEL_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return DMEL_OK;
}

struct NfftTables {
    int n_fft = 0, F = 0, KS = 0, NT = 0, groups = 0;
    int n_entries = 0, n_dense = 0;
    float2* tw1 = nullptr;       // twiddles of the plan of the training modes ...
    float2* tw2 = nullptr;
    float2* tw1p = nullptr;      // ... and of the modes that pack two frames per FFT, where that plan differs (else the same pointers)
    float2* tw2p = nullptr;
    float* ent_b = nullptr;
    float* ent_pre = nullptr;
    int pre_groups[16] = {};     // per (wave, run) of group 0: real groups of 4 k-steps inside ent_pre
    unsigned xch_groups = 0;     // FwdParams::xch_groups
    int ent_b_floats = 0;
    int4* tile_ranges = nullptr;
    float* fb_dense = nullptr;   // (F, M) for the direct-DFT kernel
    float2* tw_long = nullptr;   // (N/2) twiddles exp(-2 pi i k / N): LDS radix-2 kernels (long transforms, dL/dx)
    float* fbT = nullptr;        // long transforms: (M, F) transposed bank, (M) bands
    int2* band = nullptr;
    int2* rowband = nullptr;     // (F): non-zero column range of every filterbank row (dL/dx)
    float4* rowpk = nullptr;     // (F): (first two non-zero coefficients, first column, columns) of every row (dL/dx, wave-FFT kernel)
    bool long_rows = false;      // some row has more than two columns
    uint4* ent_h = nullptr;      // caller-supplied (dense) banks, n_fft 64 .. 4096: B fragments of the split-bf16 contraction (FwdParams::ent_h)
    float* fb_nyq = nullptr;     // ... and the row of bin n_fft/2 (n_mels)
    float4* wl_b4 = nullptr;     // kTrainW (wave-local contraction, FwdParams::wl_*): B operands, lane table, phase lengths
    int2* wl_lane = nullptr;
    int* wl_merge = nullptr;      // [phase * 64 + lane]: partner lane of merge round 1 | round 2 << 8 | receives in round 1 << 16 | in round 2 << 17
    int wl_phases = 0, wl_total4 = 0;
    int wl_len4[dmel::kWlMaxPhases] = {};
    int wl_mg[dmel::kWlMaxPhases] = {};   // per phase: bit 0 / 1 = merge round 1 / 2 is needed
    DeviceTables dev;            // what was uploaded into these tables
    void release() { dev.release(); *this = NfftTables(); }
};

}  // namespace

struct dmel_plan {
    dmel_config cfg{};
    int device = 0;
    int T = 0;
    int nchunks = 1, chunk = 0;
    double f_max = 0;
    std::map<int, NfftTables> tables;
    std::map<int, std::vector<float>> custom_fb;
    std::map<int, bool> dense_dev;     // n_fft whose tables have the dense structure and get their values from the device
    // Plan-owned scratch of the entry points that take none from the caller (layout: dmel_scratch_bytes).  Calls that use it
    // are ordered across streams by `xev` (see order_after_last_stream): two streams through one plan serialise, never race.
    unsigned char* own_scratch = nullptr;
    int own_scratch_clips = 0;
    // transforms beyond the LDS kernels (dmel_big.hip): chirp / filter tables per DFT length, twiddles per FFT length, the
    // window table and the per-workgroup sequences in global memory
    struct BigTab { int M = 0, logM = 0; float2* chirp = nullptr; float2* hbr = nullptr; };
    std::map<int, float2*> big_wodd;   // per even N: exp(-2 pi i n / N), n < N/2 (split mode of the big kernel)
    std::map<int, BigTab> big_tabs;
    std::map<int, float2*> big_tw;
    DeviceTables big_dev;              // owner of the three maps' tables
    float2* big_win = nullptr; size_t big_win_n = 0;
    float2* big_z = nullptr; size_t big_z_n = 0;
    float* fbw = nullptr;          // workspace of dmel_backward_fb (spectrogram (B, F, T) + slice partials) and dmel_backward_x
    size_t fbw_floats = 0;         // (frame gradients (B, T, N)); grown on demand
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t xev = nullptr;
    // device-resident lambd (dmel_forward_dev): what the kernels report back and what the host has concluded from it.
    // Every forward that executes draws an execution number from `exec_counter` (device) and reports under it (dmel_kernels.h).
    unsigned long long* host_words = nullptr;   // pinned, device-visible: [0..kLamRing) reports (number << 32) | bits(lambd), [kLamRing] sticky error
    unsigned* exec_counter = nullptr;           // device: executions so far
    dmel::LamTrack track;          // the host's picture of the scalar layer's lambd (dmel_lamtrack.h)
    unsigned calls = 0;            // dmel_forward_dev / _fixed calls, captured ones included; never adjusted
    int max_ahead = 8;             // forwards the host may run ahead of the last observation (0: unbounded)
    int guard_mode = 0;            // 0 auto, 1 always both neighbours, 2 never, 3 auto also under capture
    int forced_n_fft = 0, forced_guards = 0;    // dmel_plan_force_launch: the caller chooses the launches (0: the library does)
    // the multi-window layer (dmel_forward_multi_dev): one picture of lambd per channel, and its own words on the device side (made at
    // the first multi-window call): channel c reports into multi_words + c kLamMultiStride and counts on multi_exec[c]
    dmel::LamTrack multi[dmel::kMaxChannels];
    unsigned long long* multi_words = nullptr;
    unsigned* multi_exec = nullptr;
    // what the most recent dmel_forward_multi(_dev) issued (dmel_plan_last_multi_launch), and the workspace of dmel_backward_x_multi(_dev)
    // (per channel: segments or frame rows + fp64 sums; window tables; staged grad_out / out rows of the LDS path), grown on demand
    int last_multi_ns[3 * dmel::kMaxChannels] = {};
    uint32_t last_multi_mask[3 * dmel::kMaxChannels] = {};
    int last_multi_nl = 0;
    float* xmw = nullptr;
    size_t xmw_floats = 0;
    int refs = 1;                  // dmel_plan_retain / dmel_plan_release (guarded by g_plans_mu)
    dmel_mailbox* mailbox = nullptr;    // dmel_plan_attach_mailbox: the backward's result is the sum over the mailbox's ranks
    dmel::AdamParams fused_adam{};      // dmel_plan_attach_adam: param != nullptr -> the backward's dot kernel applies this update
    std::mutex mu;
    dmel_plan_info info{};
    // optional event timing
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct Span { size_t a, b; int kind; };
    std::vector<Span> spans;
};

namespace {

constexpr int kMaxPartials = 1024;
constexpr size_t kMaxSpans = 16384;

// returns an event index recorded on s, or (size_t)-1 when profiling is off / full
size_t prof_mark(dmel_plan* pl, hipStream_t s)
{
    if (!pl->profiling || pl->spans.size() >= kMaxSpans) return (size_t)-1;
    if (pl->ev_used == pl->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return (size_t)-1;
        pl->ev_pool.push_back(e);
    }
    const size_t i = pl->ev_used++;
    if (hipEventRecord(pl->ev_pool[i], s) != hipSuccess) return (size_t)-1;
    return i;
}
void prof_span(dmel_plan* pl, size_t a, size_t b, int kind)
{
    if (a != (size_t)-1 && b != (size_t)-1) pl->spans.push_back({a, b, kind});
}

// the tables of one n_fft: look up the cache, choose the bank, call the builders (dmel_tables.h), upload, insert
dmel_status build_tables(dmel_plan* pl, int N, NfftTables** out)
{
    auto it = pl->tables.find(N);
    if (it != pl->tables.end()) { *out = &it->second; return DMEL_OK; }
    NfftTables tb;
    struct Guard {          // a failed allocation half-way must not leak the tables made so far
        NfftTables* t; bool keep = false;
        ~Guard() { if (!keep) t->release(); }
    } guard{&tb};
    tb.n_fft = N;
    tb.F = N / 2 + 1;
    const int F = tb.F, M = pl->cfg.n_mels;
    dmel_status st = DMEL_OK;
#define DMEL_UP(...) do { if ((st = upload(&tb.dev, __VA_ARGS__)) != DMEL_OK) return st; } while (0)
    std::vector<float> fb((size_t)F * M);
    auto cit = pl->custom_fb.find(N);
    const bool dense_dev = pl->dense_dev.count(N) != 0, custom = cit != pl->custom_fb.end();
    if (dense_dev) std::fill(fb.begin(), fb.end(), 1.0f);        // structure only: every block present; dmel_plan_set_filterbank_dev fills the values
    else if (custom) fb = cit->second;
    else if ((st = dmel_mel_fbanks_host(F, pl->cfg.f_min, pl->f_max, M, pl->cfg.sample_rate, fb.data())) != DMEL_OK) return st;
    DMEL_UP(fb, &tb.fb_dense);
    dmel::HostTables h;
    if (!dmel::build_host_tables(fb, N, M, custom || dense_dev, !dense_dev && std::getenv("DMEL_WLC_NOSPLIT") == nullptr, &h))
        return fail(DMEL_ERR_UNSUPPORTED, "n_fft has no FFT plan");
    tb.long_rows = h.rows.long_rows;
    tb.KS = h.bs.KS; tb.NT = h.bs.NT; tb.groups = h.bs.groups; tb.n_entries = h.bs.n_entries; tb.n_dense = h.bs.n_dense;
    tb.xch_groups = h.bs.xch_groups; tb.ent_b_floats = (int)h.bs.ent_b.size();
    std::copy(h.pre.pre_groups, h.pre.pre_groups + 16, tb.pre_groups);
    tb.wl_phases = h.wl.phases; tb.wl_total4 = h.wl.total4;
    std::copy(h.wl.len4, h.wl.len4 + dmel::kWlMaxPhases, tb.wl_len4);
    std::copy(h.wl.mg, h.wl.mg + dmel::kWlMaxPhases, tb.wl_mg);
    // (in the order the tables have always been allocated; upload leaves the pointer of an empty table null, the three with a minimum length exist whenever their neighbours do)
    DMEL_UP(h.tw_long, &tb.tw_long, 1);
    DMEL_UP(h.rows.rowband, &tb.rowband);
    DMEL_UP(h.rows.rowpk, &tb.rowpk);
    DMEL_UP(h.tbank.fbT, &tb.fbT);
    DMEL_UP(h.tbank.band, &tb.band);
    DMEL_UP(h.tw.tw1, &tb.tw1);
    DMEL_UP(h.tw.tw2, &tb.tw2);
    if (h.twp_same) { tb.tw1p = tb.tw1; tb.tw2p = tb.tw2; }
    DMEL_UP(h.twp.tw1, &tb.tw1p);
    DMEL_UP(h.twp.tw2, &tb.tw2p);
    DMEL_UP(h.h.ent_h, &tb.ent_h);
    DMEL_UP(h.h.fb_nyq, &tb.fb_nyq);
    DMEL_UP(h.wl.lane, &tb.wl_lane);
    DMEL_UP(h.wl.merge, &tb.wl_merge);
    DMEL_UP(h.wl.b4, &tb.wl_b4, h.wl.lane.empty() ? 0 : 64);
    DMEL_UP(h.pre.ent_pre, &tb.ent_pre);
    DMEL_UP(h.bs.ent_b, &tb.ent_b, h.bs.tile_ranges.empty() ? 0 : 64);
    DMEL_UP(h.bs.tile_ranges, &tb.tile_ranges);
#undef DMEL_UP
    auto ins = pl->tables.emplace(N, std::move(tb));
    guard.keep = true;
    *out = &ins.first->second;
    return DMEL_OK;
}

// ---- per-call device scratch -----------------------------------------------------------------------------------------
// [0] handled word of the launch group | [64] 1024 fp64 partials of the dot kernel | [8256] its ticket counter |
// [8320] window table (w, w d^2 2^-2e) for the kernels that read it from memory | [kScratchPsum] partial clip sums
constexpr size_t kScratchPartials = 64, kScratchCounter = 64 + 8192, kScratchWin = 8320;
constexpr size_t kScratchPsum = kScratchWin + (size_t)dmel::kMaxNfft * 8;
// the dot kernel's group counters live in the upper half of the partials array, found from the ticket word (dmel_kernels.h: dot_group_counters)
static_assert(kScratchCounter - kScratchPartials == 1024 * sizeof(double) && dmel::kDotMaxBlocks * sizeof(double) == 4096 &&
              (dmel::kDotMaxBlocks / dmel::kDotGroup) * 64 <= 4096, "scratch layout the ticket tree relies on");

struct Scratch {
    unsigned* handled = nullptr; double* partials = nullptr; unsigned* counter = nullptr; float2* win = nullptr; float* psum = nullptr;
};

size_t scratch_bytes(const dmel_plan* pl, int batch)
{
    const size_t ps = ((size_t)std::max(batch, 1) * pl->nchunks * sizeof(float) + 255) / 256 * 256;
    return kScratchPsum + ps;
}

// the multi-window layer's scratch: the same layout with one window table per channel in front of the partial clip sums
size_t scratch_bytes_multi(const dmel_plan* pl, int batch, int channels)
{
    return scratch_bytes(pl, batch) + (size_t)(channels - 1) * dmel::kMaxNfft * 8;
}

Scratch carve(void* base, int channels)
{
    unsigned char* b = static_cast<unsigned char*>(base);
    Scratch sc;
    sc.handled = reinterpret_cast<unsigned*>(b);
    sc.partials = reinterpret_cast<double*>(b + kScratchPartials);
    sc.counter = reinterpret_cast<unsigned*>(b + kScratchCounter);
    sc.win = reinterpret_cast<float2*>(b + kScratchWin);
    sc.psum = reinterpret_cast<float*>(b + kScratchPsum + (size_t)(channels - 1) * dmel::kMaxNfft * 8);
    return sc;
}

bool is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// Plan-owned buffers (own_scratch, fbw) are shared by every call on the plan: a call on another stream than the previous
// one first waits for that stream's work (one event), so concurrent streams serialise on the plan instead of racing.
dmel_status order_after_last_stream(dmel_plan* pl, hipStream_t s)
{
    if (pl->last_stream_valid && pl->last_stream != s && !is_capturing(s)) {
        if (hipEventRecord(pl->xev, pl->last_stream) == hipSuccess) DMEL_HIP(hipStreamWaitEvent(s, pl->xev, 0));
        else { (void)hipGetLastError(); DMEL_HIP(hipDeviceSynchronize()); }      // the old stream is gone: be safe
    }
    pl->last_stream = s;
    pl->last_stream_valid = true;
    return DMEL_OK;
}

dmel_status ensure_own_scratch(dmel_plan* pl, int batch, hipStream_t s, Scratch* sc)
{
    if (!pl->own_scratch || batch > pl->own_scratch_clips) {
        if (is_capturing(s)) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan scratch must grow but the stream is capturing: run one call eagerly first or pass scratch");
        if (pl->own_scratch) { DMEL_HIP(hipDeviceSynchronize()); (void)hipFree(pl->own_scratch); pl->own_scratch = nullptr; pl->own_scratch_clips = 0; }
        const int clips = std::max(batch, pl->cfg.max_batch);
        const size_t bytes = scratch_bytes(pl, clips);
        DMEL_HIP(hipMalloc(&pl->own_scratch, bytes));
        DMEL_HIP(hipMemset(pl->own_scratch, 0, kScratchWin));
        pl->own_scratch_clips = clips;
    }
    *sc = carve(pl->own_scratch, 1);
    return DMEL_OK;
}

// the scratch of a call: the caller's, or the plan's own behind whatever the plan's previous stream still runs
dmel_status select_scratch(dmel_plan* pl, void* scratch, int batch, hipStream_t s, Scratch* sc)
{
    if (scratch) { *sc = carve(scratch, 1); return DMEL_OK; }
    const dmel_status st = order_after_last_stream(pl, s);
    if (st != DMEL_OK) return st;
    return ensure_own_scratch(pl, batch, s, sc);
}

// a plan-owned workspace of floats (dmel_plan::fbw, xmw) grows to `need`: never under capture (`who`: the refusal's first words)
dmel_status grow_floats(float** buf, size_t* have, size_t need, hipStream_t s, const std::string& who)
{
    if (need <= *have) return DMEL_OK;
    if (is_capturing(s)) return fail(DMEL_ERR_INVALID_ARGUMENT, who + "workspace must grow but the stream is capturing: run one call eagerly first");
    DMEL_HIP(hipStreamSynchronize(s));
    (void)hipFree(*buf); *buf = nullptr; *have = 0;
    DMEL_HIP(hipMalloc(buf, need * sizeof(float)));
    *have = need;
    return DMEL_OK;
}

// a plan-owned twiddle table of the big path, exp(-2 pi i k / n) for k < n / 2, made on first use
dmel_status big_twiddles(dmel_plan* pl, std::map<int, float2*>* tabs, int n, const float2** out)
{
    auto it = tabs->find(n);
    if (it == tabs->end()) {
        float2* d = nullptr;
        const dmel_status st = upload(&pl->big_dev, dmel::build_long_twiddles(n), &d, 1);
        if (st != DMEL_OK) return st;
        it = tabs->emplace(n, d).first;
    }
    *out = it->second;
    return DMEL_OK;
}

// tables of the big path for DFT length N: twiddles of the power-of-two FFT behind it and, when N is not a power of two,
// Bluestein's chirp c[n] = exp(-i pi n^2 / N) and the transform of its filter
dmel_status big_tables_for(dmel_plan* pl, int N, dmel_plan::BigTab* out, const float2** tw)
{
    const int M = dmel::big_fft_length(N);
    if (M > dmel::kMaxBigFft)
        return fail(DMEL_ERR_UNSUPPORTED, "transform length " + std::to_string(N) + " needs an FFT of " + std::to_string(M) +
                    " points; the HIP path stops at " + std::to_string(dmel::kMaxBigFft));
    dmel_status st = big_twiddles(pl, &pl->big_tw, M, tw);
    if (st != DMEL_OK) return st;
    auto bit = pl->big_tabs.find(N);
    if (bit == pl->big_tabs.end()) {
        dmel_plan::BigTab bt;
        bt.M = M; bt.logM = 0; while ((1 << bt.logM) < M) ++bt.logM;
        if (M != N) {
            if ((st = upload(&pl->big_dev, dmel::build_chirp(N), &bt.chirp)) != DMEL_OK) return st;
            if ((st = upload(&pl->big_dev, dmel::build_chirp_filter(N, M), &bt.hbr)) != DMEL_OK) return st;
        }
        bit = pl->big_tabs.emplace(N, bt).first;
    }
    *out = bit->second;
    return DMEL_OK;
}

// the window's centre in table coordinates.  The whole-clip window of the optimized=False branches is centred at L/2 as a real number inside its
// L = n_fft/2 entries (time_frequency.py:24), which torch.stft places (n_fft - L) / 2 = L/2 (integer) entries into the frame
float window_center(int N, int win_half) { return win_half ? (float)((N / 2) / 2) + (float)(N / 2) / 2.0f : (float)N / 2.0f; }

// the big path's plan-owned window table (N entries) and per-workgroup sequences (need_z entries, transforms longer than LDS) grow here
dmel_status grow_big_workspace(dmel_plan* pl, int N, size_t need_z, hipStream_t s)
{
    if ((size_t)N <= pl->big_win_n && need_z <= pl->big_z_n) return DMEL_OK;
    if (is_capturing(s)) return fail(DMEL_ERR_INVALID_ARGUMENT, "workspace must grow but the stream is capturing: run one call eagerly first");
    DMEL_HIP(hipDeviceSynchronize());
    if ((size_t)N > pl->big_win_n) {
        (void)hipFree(pl->big_win); pl->big_win = nullptr; pl->big_win_n = 0;
        DMEL_HIP(hipMalloc(&pl->big_win, (size_t)N * sizeof(float2)));
        pl->big_win_n = (size_t)N;
    }
    if (need_z > pl->big_z_n) {
        (void)hipFree(pl->big_z); pl->big_z = nullptr; pl->big_z_n = 0;
        DMEL_HIP(hipMalloc(&pl->big_z, need_z * sizeof(float2)));
        pl->big_z_n = need_z;
    }
    return DMEL_OK;
}

// one launch of the multi-window layer: `count` channels (nibbles of `list`, with their lambd roles in `roles`) of an output with `ch_out` channels (edges !=
// nullptr: the band-split layer -- ch_out = 1, channel c writes rows [edges[c], edges[c + 1]) of the one image: dmel_fwd_band_kernel).  channels = 0: none
struct MultiLaunch { int ch_out = 0, count = 0; unsigned list = 0, roles = 0; float vals[dmel::kMaxChannels] = {}; const int32_t* edges = nullptr; int channels = 0; };

// What a forward call asks for, filled by field name at the entry points; what varies between the launches of one call (n_fft, lambd roles) travels next to it
struct FwdCall {
    const float* x = nullptr; int batch = 0; unsigned flags = 0; double eps = 0.0; float* out = nullptr; float* tangent = nullptr;
    int mode = dmel::kInfer, remove_dc = 1, win_half = 0;
    float* spec_out = nullptr; const int32_t* lengths = nullptr;       // dmel_forward_dev_fixed_spec: the spectrogram is saved too; per-clip lengths (device)
    bool fb_len = false;        // lengths through a trained bank (dmel_forward_dev_fixed_lengths, dmel_backward_fb_dev_lengths): dmel_fwd_fb_len_kernel -- kTrainH, kSpec, spec_out
    MultiLaunch ml;
    bool multi() const { return ml.channels > 0; }
    // DMEL_FLAG_X_INDIRECT: x is a pointer cell that holds the batch's address, read by every kernel of the forward
    const float* const* x_cell() const { return (flags & DMEL_FLAG_X_INDIRECT) ? reinterpret_cast<const float* const*>(x) : nullptr; }
    const float* x_direct() const { return (flags & DMEL_FLAG_X_INDIRECT) ? nullptr : x; }
};
// the mel layer's forward: the training kernels when a tangent is asked for, DC removed
FwdCall mel_call(const float* x, int batch, unsigned flags, double eps, void* out, float* tangent)
{
    FwdCall c;
    c.x = x; c.batch = batch; c.flags = flags; c.eps = eps; c.out = static_cast<float*>(out); c.tangent = tangent; c.mode = tangent ? dmel::kTrain : dmel::kInfer;
    return c;
}
// the K-window layers: K channels of (batch, K, M, T), or with band_edges the row groups of ONE (batch, 1, M, T) image
FwdCall k_call(const float* x, int batch, int channels, const int32_t* band_edges, unsigned flags, double eps, void* out, float* tangent)
{
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    c.ml.channels = channels; c.ml.ch_out = channels; c.ml.edges = band_edges;
    return c;
}
// the spectrogram layer's forward: no mel stage, no log
FwdCall spec_call(const float* x, int batch, float* spec, float* tangent, uint32_t spec_flags)
{
    FwdCall c;
    c.x = x; c.batch = batch; c.out = spec; c.tangent = tangent; c.mode = tangent ? dmel::kSpecTrain : dmel::kSpec;
    c.remove_dc = (spec_flags & DMEL_SPEC_REMOVE_DC) ? 1 : 0; c.win_half = (spec_flags & DMEL_SPEC_HALF_WINDOW) ? 1 : 0;
    return c;
}

// the prep kernel in front of a forward launch: clip sums (kPrepSums) and / or window table (kPrepWindow; multi-window: one per channel at win + c kMaxNfft)
constexpr unsigned kPrepSums = 1u, kPrepWindow = 2u;
dmel_status forward_prep(dmel_plan* pl, int N, float2* win, const dmel::LamArgs& lam, const FwdCall& c, const Scratch& sc, hipStream_t s, unsigned what)
{
    const bool need_sums = (what & kPrepSums) != 0, need_window = (what & kPrepWindow) != 0;
    dmel::PrepParams pp{};
    pp.x = c.x_direct(); pp.x_ind = c.x_cell(); pp.psum = sc.psum; pp.win2 = win;
    pp.B = need_sums ? c.batch : 0; pp.L = pl->cfg.n_points; pp.nchunks = pl->nchunks; pp.chunk = pl->chunk;
    pp.N = need_window ? N : 0; pp.normalize = pl->cfg.normalize_window; pp.win_half = c.win_half; pp.center = window_center(N, c.win_half);
    pp.lam = lam; pp.lam.role = dmel::kLamQuiet; pp.lengths = need_sums ? c.lengths : nullptr;
    if (c.multi() && need_window) {
        for (int i = 0; i < c.ml.count; ++i) {
            const int ch = (int)((c.ml.list >> (4 * i)) & 15u);
            pp.lam = dmel::lam_for_channel(lam, ch, 0, dmel::kLamQuiet, c.ml.vals);
            pp.win2 = win + (size_t)ch * dmel::kMaxNfft;
            pp.B = (need_sums && i == 0) ? c.batch : 0;
            DMEL_HIP(dmel::launch_prep(pp, s));
        }
        return DMEL_OK;
    }
    DMEL_HIP(dmel::launch_prep(pp, s));
    return DMEL_OK;
}

// ---- lengths the LDS kernels do not reach: global-memory FFT / Bluestein (dmel_big.hip) --------------------------------
dmel_status forward_big(dmel_plan* pl, NfftTables* tb, const dmel::LamArgs& lam, const FwdCall& c, const Scratch& sc, hipStream_t s,
                        bool* sums_done, dmel_plan_info* info)
{
    const int N = tb->n_fft;
    dmel_plan::BigTab bt;
    const float2* tw = nullptr;
    dmel_status st = big_tables_for(pl, N, &bt, &tw);
    if (st != DMEL_OK) return st;
    // split mode (dmel_big.hip): the transform itself would live in global memory, its two halves fit LDS
    const float2* wodd = nullptr;
    bool split = false;
    if (dmel::big_uses_global(bt.M)) {
        const int H = N / 2;
        int Mh = H;
        if (H & (H - 1)) { Mh = 1; while (Mh < 2 * H - 1) Mh <<= 1; }
        if (H >= 2 && dmel::big_can_split(Mh, pl->cfg.n_mels)) {
            if ((st = big_tables_for(pl, H, &bt, &tw)) != DMEL_OK) return st;
            if ((st = big_twiddles(pl, &pl->big_wodd, N, &wodd)) != DMEL_OK) return st;
            split = true;
        }
    }
    if ((st = order_after_last_stream(pl, s)) != DMEL_OK) return st;          // window table and sequences are plan-owned
    const bool pair = (c.mode == dmel::kInfer || c.mode == dmel::kSpec);
    const long long units = (long long)c.batch * (pair ? (pl->T + 1) / 2 : pl->T);
    const int grid = dmel::big_grid(units, bt.M);
    const size_t need_z = dmel::big_uses_global(bt.M) ? (size_t)grid * bt.M : 0;
    if ((st = grow_big_workspace(pl, N, need_z, s)) != DMEL_OK) return st;
    const bool need_sums = c.remove_dc && !*sums_done;
    const size_t m0 = prof_mark(pl, s);
    if ((st = forward_prep(pl, N, pl->big_win, lam, c, sc, s, kPrepWindow | (need_sums ? kPrepSums : 0u))) != DMEL_OK) return st;
    if (need_sums) *sums_done = true;
    const size_t m1 = prof_mark(pl, s);
    prof_span(pl, m0, m1, 0);
    dmel::BigParams bp{};
    bp.x = c.x_direct(); bp.x_ind = c.x_cell(); bp.out = c.out; bp.tangent = c.tangent; bp.psum = sc.psum; bp.win2 = pl->big_win;
    bp.tw = tw; bp.chirp = bt.chirp; bp.hbr = bt.hbr; bp.zws = pl->big_z; bp.fbT = tb->fbT; bp.band = tb->band;
    bp.B = c.batch; bp.L = pl->cfg.n_points; bp.T = pl->T; bp.hop = pl->cfg.hop_length; bp.M = pl->cfg.n_mels;
    bp.nchunks = pl->nchunks; bp.N = N; bp.F = tb->F; bp.mode = c.mode; bp.Mfft = bt.M; bp.logM = bt.logM;
    bp.inv_L = 1.0f / (float)pl->cfg.n_points; bp.eps = (float)c.eps; bp.flags = c.flags; bp.remove_dc = c.remove_dc; bp.lam = lam;
    bp.split = split ? 1 : 0; bp.wodd = wodd;
    DMEL_HIP(dmel::launch_big(bp, s));
    prof_span(pl, m1, prof_mark(pl, s), 1);
    info->kernel_path = 3; info->frames_per_tile = pair ? 2 : 1; info->grid_fwd = grid;
    info->fb_blocks = 0; info->fb_blocks_dense = 0; info->lds_bytes = dmel::big_uses_global(bt.M) ? 0 : bt.M * 8;
    info->contraction = -1; info->wl_steps = 0;
    return DMEL_OK;
}

// ---- n_fft < 32: the direct-DFT kernel (its window table and clip sums come from the prep kernel, already issued) ----------
dmel_status forward_naive(dmel_plan* pl, NfftTables* tb, const dmel::LamArgs& lam, const FwdCall& c, const Scratch& sc, hipStream_t s,
                          dmel_plan_info* info)
{
    const int N = tb->n_fft;
    dmel::NaiveParams np{};
    np.x = c.x_direct(); np.x_ind = c.x_cell(); np.out = c.out; np.tangent = c.tangent; np.psum = sc.psum; np.win2 = sc.win; np.fb = tb->fb_dense;
    np.B = c.batch; np.L = pl->cfg.n_points; np.T = pl->T; np.hop = pl->cfg.hop_length; np.M = pl->cfg.n_mels;
    np.nchunks = pl->nchunks; np.N = N; np.F = tb->F; np.mode = c.mode;
    np.inv_L = 1.0f / (float)pl->cfg.n_points; np.eps = (float)c.eps; np.flags = c.flags; np.remove_dc = c.remove_dc; np.lam = lam;
    DMEL_HIP(dmel::launch_naive(np, s));
    info->kernel_path = 1; info->frames_per_tile = 1; info->grid_fwd = c.batch * pl->T;
    info->fb_blocks = 0; info->fb_blocks_dense = 0; info->lds_bytes = (2 * N + 2 * tb->F) * 4;
    info->contraction = -1; info->wl_steps = 0;
    return DMEL_OK;
}

// ---- n_fft 32 ... 16384: the fused wave-FFT + MFMA kernel; `kernel_mean`: it forms the clip mean itself --------------------
dmel_status forward_fused(dmel_plan* pl, NfftTables* tb, const dmel::LamArgs& lam, const FwdCall& c, const Scratch& sc, hipStream_t s,
                          bool kernel_mean, dmel_plan_info* info)
{
    const int N = tb->n_fft;
    const MultiLaunch* ml = c.multi() ? &c.ml : nullptr;
    int mode = c.mode;
    const unsigned flags = c.flags & ~DMEL_FLAG_X_INDIRECT;
    dmel::FwdParams fp{};
    fp.x = c.x_direct(); fp.x_ind = c.x_cell(); fp.out = c.out; fp.tangent = c.tangent; fp.psum = (c.remove_dc && !kernel_mean) ? sc.psum : nullptr; fp.win2 = sc.win;
    fp.tw1 = dmel::mode_pairs(mode) ? tb->tw1p : tb->tw1; fp.tw2 = dmel::mode_pairs(mode) ? tb->tw2p : tb->tw2; fp.ent_b = tb->ent_b; fp.tile_ranges = tb->tile_ranges; fp.ent_b_floats = tb->ent_b_floats; fp.ent_pre = tb->ent_pre;
    for (int i = 0; i < 16; ++i) fp.pre_groups[i] = tb->pre_groups[i];
    fp.B = c.batch; fp.L = pl->cfg.n_points; fp.T = pl->T; fp.hop = pl->cfg.hop_length; fp.M = pl->cfg.n_mels;
    fp.nchunks = pl->nchunks; fp.groups = tb->groups; fp.xch_groups = tb->xch_groups;
    // DMEL_FLAG_MFMA_BF16X3: the training forward through a caller-supplied (dense) bank contracts on the bf16 matrix pipe
    const bool hsplit = (flags & DMEL_FLAG_MFMA_BF16X3) && mode == dmel::kTrain && tb->ent_h != nullptr && (!c.lengths || c.fb_len);
    if (hsplit) mode = dmel::kTrainH;
    // the wave-local contraction where it is built (n_fft 1024, up to 512 mel bands): DMEL_WLC=0 keeps the round-4 kernel, DMEL_WLC=1
    // the 8-wave workgroups, DMEL_WLC=2 the 16-wave ones where they are built (diagnostics).
    static const int wlc_env = std::getenv("DMEL_WLC") ? std::atoi(std::getenv("DMEL_WLC")) : -1;
    // (a dense bank -- a caller-supplied or trainable matrix -- makes every quad's band the whole spectrum: 1 032 steps per wave at n_fft 1024
    // against 68 for the HTK bank; the 16 x 16 x 4 tiles of kTrain then win -- trainable-filterbank step 128.9 against 114.4 us, round 5)
    const bool wl_compact = tb->wl_total4 * 4 <= 320;
    if (mode == dmel::kTrain && tb->wl_b4 != nullptr && wlc_env != 0 && (wl_compact || wlc_env > 0)) {
        const int wide_fpt = dmel::forward_has_wlc_wide(N) ? dmel::forward_frames_per_tile(N, dmel::kTrainWW) : 0;
        const bool wide = wide_fpt > 0 && wlc_env == 2 && !c.lengths;      // (16-wave workgroups: measured slower, dmel_kernels.h; built only on request)
        mode = wide ? dmel::kTrainWW : dmel::kTrainW;
        fp.wl_b4 = tb->wl_b4; fp.wl_lane = tb->wl_lane; fp.wl_phases = tb->wl_phases; fp.wl_total4 = tb->wl_total4;
        for (int i = 0; i < dmel::kWlMaxPhases; ++i) { fp.wl_len4[i] = tb->wl_len4[i]; fp.wl_mg[i] = tb->wl_mg[i]; }
        fp.wl_merge = tb->wl_merge;
    }
    const int fpt = dmel::forward_frames_per_tile(N, mode);
    fp.tiles_per_clip = (pl->T + fpt - 1) / fpt;
    fp.inv_L = 1.0f / (float)pl->cfg.n_points; fp.eps = (float)c.eps; fp.flags = flags; fp.lam = lam;
    fp.remove_dc = c.remove_dc; fp.normalize = pl->cfg.normalize_window; fp.win_half = c.win_half;
    fp.spec_out = c.spec_out;
    fp.ent_h = tb->ent_h; fp.fb_nyq = tb->fb_nyq;
    static const int force_tpw = std::getenv("DMEL_TILES_PER_WG") ? std::atoi(std::getenv("DMEL_TILES_PER_WG")) : 0;   // diagnostics
    int tpw = dmel::forward_tiles_per_wg(N, mode, c.batch, fp.tiles_per_clip);
    if (force_tpw == 1 || (force_tpw == 2 && dmel::forward_two_tiles(N, mode))) tpw = force_tpw;
    if (hsplit || c.lengths || (ml && ml->edges)) tpw = 1;                  // (the length-aware kernels, dmel_fwd_band_kernel: one tile per workgroup)
    fp.wgs_per_clip = (fp.tiles_per_clip + tpw - 1) / tpw;
    long long grid = (long long)c.batch * fp.wgs_per_clip;
    if (ml) {
        fp.ch_out = ml->ch_out; fp.ch_grid = (int)grid; fp.ch_list = ml->list; fp.ch_roles = ml->roles;
        for (int ch = 0; ch < dmel::kMaxChannels; ++ch) fp.ch_val[ch] = ml->vals[ch];
        grid *= ml->count;
    }
    if (grid > 0x7fffffffLL) return fail(DMEL_ERR_INVALID_ARGUMENT, "too many tiles for one launch");
    if (grid <= dmel::forward_resident_workgroups(N, mode)) fp.flags |= dmel::kFwdEdgeFirst;      // one round: see the kernel's prologue
    // the kernel follows the parameter type: per-clip lengths, the band-split layer's row ranges, both, or neither
    const bool band = ml && ml->edges;
    dmel::FwdLenParams lp{};
    lp.lengths = c.lengths;
    dmel::FwdMultiLenParams mlp{};
    mlp.lengths = c.lengths;
    dmel::FwdBandParams bp{};
    dmel::FwdBandLenParams blp{};
    blp.lengths = c.lengths;
    dmel::FwdFbLenParams flp{};
    flp.lengths = c.lengths;
    // (a trained bank's lengths: kInfer -- a forward without a tangent -- is dmel_fwd_len_kernel's, which contracts through whatever tables the plan holds;
    // the wave-local contraction, never chosen for a dense bank at the sizes it is built for, has no build in that unit)
    const bool fbk = c.fb_len && !ml && (mode == dmel::kTrain || mode == dmel::kTrainH || mode == dmel::kSpec);
    if (c.lengths && c.spec_out && !fbk) return fail(DMEL_ERR_UNSUPPORTED, "per-clip lengths: the spectrogram is saved by the kTrain / kTrainH kernels of a trained bank only");
    for (int ch = 0; band && ch <= dmel::kMaxChannels; ++ch) blp.band_edges[ch] = bp.band_edges[ch] = ml->edges[std::min(ch, ml->channels)];
    auto launch = [&](auto& q) { static_cast<dmel::FwdParams&>(q) = fp; return dmel::launch_forward(N, mode, tpw, q, (int)grid, s); };
    DMEL_HIP(c.lengths ? (band ? launch(blp) : ml ? launch(mlp) : fbk ? launch(flp) : launch(lp)) : band ? launch(bp) : launch(fp));
    info->kernel_path = 0; info->frames_per_tile = fpt; info->grid_fwd = (int)grid;
    info->fb_blocks = tb->n_entries; info->fb_blocks_dense = tb->n_dense;
    info->lds_bytes = dmel::forward_lds_bytes(N, mode);
    const bool spec_only = mode == dmel::kSpec || mode == dmel::kSpecTrain;
    info->contraction = spec_only ? -1 : (dmel::mode_wlc(mode) ? 1 : (mode == dmel::kTrainH ? 2 : 0));
    info->wl_steps = dmel::mode_wlc(mode) ? 4 * fp.wl_total4 : 0;
    return DMEL_OK;
}

// One launch (plus, when needed, the prep kernel in front of it) of the forward `c` for a given n_fft.  `lam`: where lambd comes from and whether the kernels check
// it against N (dmel_kernels.h); `sc`: this call's scratch; `sums_done`: shared by the launches of one call.  The plan mutex is held by the caller.
dmel_status launch_forward_n(dmel_plan* pl, int N, const dmel::LamArgs& lam, const FwdCall& c, const Scratch& sc, hipStream_t s, bool* sums_done)
{
    if (N < 1) return fail(DMEL_ERR_UNSUPPORTED, "n_fft = " + std::to_string(N));
    const bool pow2 = (N & (N - 1)) == 0;
    const bool big = !pow2 || N > dmel::kMaxNfft;
    // per-clip lengths (dmel_fwd_len_kernel; multi-window: dmel_fwd_multi_len_kernel / dmel_fwd_band_len_kernel): the fused kernel's range, the HTK bank
    // (a saved spectrogram and the spectrogram modes: the calls of a trained bank, c.fb_len, alone)
    if (c.lengths && (big || N < dmel::kMinFastNfft || ((c.spec_out || c.mode == dmel::kSpec) && !c.fb_len) || c.win_half))
        return fail(DMEL_ERR_UNSUPPORTED, "per-clip lengths run the fused kernel only: n_fft 32 ... 16384 (n_fft = " + std::to_string(N) + ")");
    if (c.multi() && (big || N < dmel::kMinFastNfft || c.spec_out))
        return fail(DMEL_ERR_UNSUPPORTED, "the multi-window layer runs n_fft 32 ... 16384 only (n_fft = " + std::to_string(N) + ")");
    if (c.spec_out && (big || N < dmel::kMinFastNfft || c.mode != dmel::kTrain))
        return fail(DMEL_ERR_UNSUPPORTED, "the spectrogram is saved by the fused training kernel only (power-of-two n_fft from 32 to 16384, tangent requested)");
    if (big && (N & 1)) return fail(DMEL_ERR_UNSUPPORTED, "n_fft = " + std::to_string(N) + " is odd");
    NfftTables* tb = nullptr;
    dmel_status st = build_tables(pl, N, &tb);
    if (st != DMEL_OK) return st;
    dmel_plan_info info{};
    info.n_fft = N; info.n_freqs = tb->F; info.n_time = pl->T;
    if (big) {
        if ((st = forward_big(pl, tb, lam, c, sc, s, sums_done, &info)) == DMEL_OK) pl->info = info;
        return st;
    }
    // The fused kernel builds its own window table (n_fft <= 4096) and, for clips up to 32768 samples, its own clip mean; the prep kernel only runs for
    // what is left: partial sums of long clips, the window table of n_fft 8192 / 16384, and everything the direct-DFT kernel (n_fft < 32) needs.
    const bool fast = N >= dmel::kMinFastNfft && N <= dmel::kMaxFastNfft;
    const bool kernel_mean = fast && pl->cfg.n_points <= 32768;
    const bool need_sums = c.remove_dc && !kernel_mean && !*sums_done;                  // the launches of one group share the sums
    const bool need_window = !fast || !dmel::forward_window_in_lds(N);
    const size_t m0 = prof_mark(pl, s);
    if (need_sums || need_window) {
        if ((st = forward_prep(pl, N, sc.win, lam, c, sc, s, (need_sums ? kPrepSums : 0u) | (need_window ? kPrepWindow : 0u))) != DMEL_OK) return st;
        if (need_sums) *sums_done = true;
    }
    const size_t m1 = prof_mark(pl, s);
    if (need_sums || need_window) prof_span(pl, m0, m1, 0);
    pl->info.n_fft = info.n_fft; pl->info.n_freqs = info.n_freqs; pl->info.n_time = info.n_time;      // (these three also when the launch below is refused)
    st = N < dmel::kMinFastNfft ? forward_naive(pl, tb, lam, c, sc, s, &info) : forward_fused(pl, tb, lam, c, sc, s, kernel_mean, &info);
    if (st != DMEL_OK) return st;
    prof_span(pl, m1, prof_mark(pl, s), 1);
    pl->info = info;
    return DMEL_OK;
}

// the launches of one forward call, in order; dmel_plan_get_info then describes the first, the one the host expected to do the work
template <class F> dmel_status issue_group(dmel_plan* pl, int nl, F&& launch)
{
    dmel_plan_info primary_info = pl->info;
    for (int i = 0; i < nl; ++i) {
        const dmel_status st = launch(i);
        if (st != DMEL_OK) return st;
        if (i == 0) primary_info = pl->info;
    }
    pl->info = primary_info;
    return DMEL_OK;
}

// An exchange of the plan's mailbox that gave up on a rank left NaN in lambd.grad on the ranks that waited: every later call on
// the plan says so (one pinned word read, no synchronisation) until dmel_mailbox_error has read and cleared the word.
dmel_status mailbox_status(const dmel_plan* pl)
{
    const unsigned long long w = dmel::mailbox_peek_error(pl->mailbox);
    if (w == 0) return DMEL_OK;
    return fail(DMEL_ERR_MAILBOX_TIMEOUT, "mailbox all-reduce: rank " + std::to_string((unsigned)(w & 0xffffffffu)) + " never arrived at exchange " +
                std::to_string((unsigned)(w >> 32)) + ": the reduced gradient of that step was NaN on this rank (dmel_mailbox_error clears this)");
}

// a plan's tables and scratch live on the device it was created on: launching from a thread whose current device is another
// one would run the kernels there, on pointers that mean nothing there
dmel_status check_device(const dmel_plan* pl)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return fail(DMEL_ERR_NO_DEVICE, "no current HIP device"); }
    if (dev != pl->device)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "the plan belongs to device " + std::to_string(pl->device) + " but the current device is " +
                    std::to_string(dev) + " (hipSetDevice / torch.cuda.device before the call)");
    return DMEL_OK;
}

// include/dmel.h, "Alignment": what the library only reads (x, grad_out, lengths, the filterbank, a saved tangent or spectrogram) needs
// the alignment of its element -- the kernels dispatch on the address --, what it stores through is written
// with 16- and 8-byte stores that no kernel guards (the fused forward's epilogue: float4 / float2 / packed bf16 rows of out and
// tangent; fp64 partials in scratch) and must be 16-byte aligned.  Checked on the host before anything is launched; NULL = not given.
struct StorePtr { const char* name; const void* ptr; };
dmel_status check_store_aligned(const char* fn, std::initializer_list<StorePtr> ptrs)
{
    for (const StorePtr& sp : ptrs)
        if (sp.ptr && (reinterpret_cast<uintptr_t>(sp.ptr) & 15u) != 0)
            return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + sp.name + " must be 16-byte aligned (the kernels store through it with "
                        "16-byte writes); its address ends in " + std::to_string((unsigned)(reinterpret_cast<uintptr_t>(sp.ptr) & 15u)) +
                        " modulo 16.  Pointers that are only read (x, grad_out, lengths, filterbank) need their element's alignment");
    return DMEL_OK;
}

dmel_status check_forward_args(dmel_plan* pl, const float* x, int batch, const void* out)
{
    if (!pl) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (batch < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch < 0");
    if (batch > 0 && (!x || !out)) return fail(DMEL_ERR_INVALID_ARGUMENT, "x / out is NULL");
    if (batch > 65534) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch > 65534 (split the call)");
    if (pl->mailbox) { dmel_status ms = mailbox_status(pl); if (ms != DMEL_OK) return ms; }
    return check_device(pl);
}

// lambd by value (the host has read it, as time_frequency.py:39 does): one launch, plan-owned scratch unless given; the plan mutex is held by the caller.
// lambd_dev != nullptr: the kernels read lambd from the device instead (no host read: capturable); the transform length must then
// be given (n_fft_override: the lengths that do not depend on lambd -- optimized=False branches, the spectrogram layer).
dmel_status run_forward_nolock(dmel_plan* pl, const FwdCall& c, float lambd, const float* lambd_dev, int n_fft_override, void* scratch, void* stream)
{
    dmel_status st = check_forward_args(pl, c.x, c.batch, c.out);
    if (st != DMEL_OK) return st;
    if (c.batch == 0) return DMEL_OK;
    if (lambd_dev && n_fft_override <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd on the device needs an explicit n_fft");
    if (!lambd_dev && !std::isfinite(lambd)) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int N = n_fft_override > 0 ? n_fft_override : dmel_n_fft(lambd);
    Scratch sc;
    if ((st = select_scratch(pl, scratch, c.batch, s, &sc)) != DMEL_OK) return st;
    dmel::LamArgs lam{};
    lam.dev = lambd_dev; lam.val = lambd_dev ? 0.f : lambd; lam.n_expected = 0;      // N was derived from this very value (or given explicitly)
    lam.role = dmel::kLamFirst | dmel::kLamLast;
    lam.dot_counter = scratch ? sc.counter : nullptr;            // plan-owned counters are zeroed at allocation and reset themselves
    bool sums_done = false;
    return launch_forward_n(pl, N, lam, c, sc, s, &sums_done);
}

dmel_status run_forward(dmel_plan* pl, const FwdCall& c, float lambd, const float* lambd_dev, int n_fft_override, void* scratch, void* stream)
{
    if (!pl) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    std::lock_guard<std::mutex> lock(pl->mu);
    return run_forward_nolock(pl, c, lambd, lambd_dev, n_fft_override, scratch, stream);
}

// ---- device-resident lambd: the host steps around the rule of dmel_lamtrack.h ------------------------------------------------------
static_assert(dmel::lamtrack::kMaxGuardNfft == dmel::kMaxBigFft, "dmel_lamtrack.h stops guarding where the HIP path stops");
namespace lt = dmel::lamtrack;

// K tracked values: their pictures and pinned words -- value c has its ring of kLamRing reports and, behind it, its sticky error word at words + c
// kLamMultiStride.  The scalar layer is K = 1 over dmel_plan::track / host_words, the multi-window layer its channels over multi / multi_words
struct Tracked {
    dmel::LamTrack* tr; unsigned long long* words; int K; bool multi;       // multi: the multi-window layer's channels (their texts, their n_fft range)
    unsigned long long* ring(int c) const { return words + (size_t)c * dmel::kLamMultiStride; }
};

// forwards that no launch covered (NaN on the device): every sticky word is read and cleared, its value started over; the first is returned for the caller's text
struct LamError { int channel = -1; float seen = 0.f, lam = 0.f; unsigned seq = 0; };
LamError take_errors(const Tracked& t)
{
    LamError e;
    for (int c = 0; c < t.K; ++c) {
        float lam = 0.f; unsigned seq = 0;
        if (!lt::take_error(t.ring(c), dmel::kLamRing, &seq, &lam)) continue;
        const float seen = t.tr[c].lam_seen;
        lt::reset(&t.tr[c]);
        if (e.channel < 0) { e.channel = c; e.seen = seen; e.lam = lam; e.seq = seq; }
    }
    return e;
}

bool multi_in_range(int n) { return n >= dmel::kMinFastNfft && n <= dmel::kMaxFastNfft; }

// the multi-window layer's K host values: finite, n_fft inside the fused kernel's range
dmel_status check_lambd_multi(const float* lam, int channels)
{
    for (int c = 0; c < channels; ++c) {
        if (!std::isfinite(lam[c])) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd of channel " + std::to_string(c) + " is not finite");
        const int n = dmel_n_fft(lam[c]);
        if (!multi_in_range(n))
            return fail(DMEL_ERR_UNSUPPORTED, "channel " + std::to_string(c) + ": lambd = " + std::to_string(lam[c]) + " gives n_fft " +
                        std::to_string(n) + ", the multi-window layer serves 32 ... 16384");
    }
    return DMEL_OK;
}

// Fold the latest reports into every picture; then the cold start if one of them is empty -- the one blocking read of the K values (the reference does one
// per sample, time_frequency.py:39) -- and otherwise the bounded run-ahead: the picture the launches are chosen from is at most max_ahead calls old
dmel_status settle_pictures(dmel_plan* pl, const Tracked& t, const float* lambd_dev, hipStream_t s, bool capturing)
{
    bool cold = false;
    for (int c = 0; c < t.K; ++c) { lt::observe(&t.tr[c], t.ring(c), dmel::kLamRing); cold |= !t.tr[c].lam_known; }
    if (cold) {
        if (capturing) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(t.multi ? "dmel_forward_multi_dev" : "dmel_forward_dev") + ": run the layer once eagerly before capturing it into a graph");
        float lam[dmel::kMaxChannels];
        DMEL_HIP(hipMemcpyAsync(lam, lambd_dev, t.K * sizeof(float), hipMemcpyDeviceToHost, s));
        DMEL_HIP(hipStreamSynchronize(s));
        // (the scalar layer follows a finite lambd to any n_fft; a channel of the multi-window layer must stay in the fused kernel's range)
        if (!t.multi && !std::isfinite(lam[0])) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
        const dmel_status st = t.multi ? check_lambd_multi(lam, t.K) : DMEL_OK;
        if (st != DMEL_OK) return st;
        for (int c = 0; c < t.K; ++c)
            if (!t.tr[c].lam_known) lt::cold_start(&t.tr[c], t.ring(c), dmel::kLamRing, lam[c]);
    } else if (!capturing && pl->max_ahead > 0) {
        for (int c = 0; c < t.K; ++c) {
            dmel::LamTrack& tr = t.tr[c];
            for (long spins = 0; tr.issued - tr.seq_seen > (unsigned)pl->max_ahead && spins < 200000000L; ++spins) {
                if (!lt::observe(&tr, t.ring(c), dmel::kLamRing) && (spins & 1023) == 1023 && hipStreamQuery(s) == hipSuccess) { lt::observe(&tr, t.ring(c), dmel::kLamRing); break; }
            }
        }
        (void)hipGetLastError();
    }
    return DMEL_OK;
}

// tables of the sizes about to be launched and of their neighbours inside [lo, hi] exist before they are needed: building allocates and copies (no capture)
dmel_status prebuild_tables(dmel_plan* pl, const int* ns, int nl, int lo, int hi)
{
    NfftTables* tb = nullptr;
    for (int i = 0; i < nl; ++i)
        for (int n : {ns[i], 2 * ns[i], ns[i] / 2}) {
            const dmel_status st = (n >= lo && n <= hi) ? build_tables(pl, n, &tb) : DMEL_OK;
            if (st != DMEL_OK) return st;
        }
    return DMEL_OK;
}

// a captured forward executes when (and as often as) its graph is replayed: only eager calls draw an execution number now
void count_call(dmel_plan* pl, const Tracked& t, bool capturing)
{
    ++pl->calls;
    for (int c = 0; !capturing && c < t.K; ++c) ++t.tr[c].issued;
}

// where a tracked forward's kernels find lambd, their execution counter(s) and the words they report into
dmel::LamArgs tracked_lam_args(const float* lambd_dev, unsigned* exec_counter, unsigned long long* words, const Scratch& sc)
{
    dmel::LamArgs lam{};
    lam.dev = lambd_dev; lam.exec_counter = exec_counter; lam.handled = sc.handled; lam.host_seen = words; lam.host_error = words + dmel::kLamRing;
    return lam;
}

// the scalar layer's launch choice: the caller's (dmel_plan_force_launch; the multi-window layer has none) or the tracker's
void decide_scalar(const dmel_plan* pl, bool capturing, int* n_fft, int* guards)
{
    if (pl->forced_n_fft > 0) { *n_fft = pl->forced_n_fft; *guards = pl->forced_guards; return; }
    lt::decide(pl->track, pl->guard_mode, pl->max_ahead, capturing, n_fft, guards);
}

// The launches of a multi-window call: one entry per distinct n_fft, ascending, each with the mask of the channels that need it
struct LaunchList { int ns[3 * dmel::kMaxChannels] = {}; uint32_t mask[3 * dmel::kMaxChannels] = {}; int nl = 0; };
// channel c needs n[c] and, where `guards` says so (bit 0: n / 2, bit 1: 2 n; nullptr: none), the neighbours that lie inside [lo, hi]
LaunchList group_by_nfft(const int* n, const int* guards, int channels, int lo, int hi)
{
    std::map<int, uint32_t> u;
    for (int c = 0; c < channels; ++c) {
        u[n[c]] |= 1u << c;
        const int g = guards ? guards[c] : 0;
        if ((g & 2) && 2 * n[c] >= lo && 2 * n[c] <= hi) u[2 * n[c]] |= 1u << c;
        if ((g & 1) && n[c] / 2 >= lo && n[c] / 2 <= hi) u[n[c] / 2] |= 1u << c;
    }
    LaunchList ll;
    for (const auto& kv : u) { ll.ns[ll.nl] = kv.first; ll.mask[ll.nl] = kv.second; ++ll.nl; }
    return ll;
}

// the launches K host values ask for: each channel's own n_fft
LaunchList group_host_values(const float* lambd, int channels)
{
    int n[dmel::kMaxChannels];
    for (int c = 0; c < channels; ++c) n[c] = dmel_n_fft(lambd[c]);
    return group_by_nfft(n, nullptr, channels, 0, 0);
}

std::mutex g_plans_mu;             // guards dmel_plan::refs and g_live_plans
std::unordered_set<const dmel_plan*> g_live_plans;     // every plan between dmel_plan_create and its last release (dmel_plan_is_live)

}  // namespace

extern "C" {

int32_t dmel_abi_version(void) { return DMEL_ABI_VERSION; }

const char* dmel_last_error(void) { return g_err.c_str(); }

int32_t dmel_n_fft(float lambd) { return lt::n_fft(lambd); }

dmel_status dmel_window_host(float lambd, int32_t n_fft, int32_t normalize, float* window, float* dwindow)
{
    if (n_fft < 1 || !window) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_window_host: bad arguments");
    const float denom = std::fabs(lambd) + 1e-15f;
    const double den = (double)denom;
    std::vector<double> dw(n_fft);
    double ww = 0.0, wd = 0.0;
    for (int n = 0; n < n_fft; ++n) {
        const float d = (float)n - (float)n_fft / 2.0f;
        const float t = d / denom;
        window[n] = std::exp(-0.5f * (t * t));
        dw[n] = (double)window[n] * (double)d * (double)d / (den * den * den);
        ww += (double)window[n] * (double)window[n];
        wd += (double)window[n] * dw[n];
    }
    if (normalize) {
        const double nrm = std::sqrt(ww);
        for (int n = 0; n < n_fft; ++n) {
            const double w = (double)window[n];
            dw[n] = dw[n] / nrm - w * wd / (nrm * nrm * nrm);
            window[n] = (float)(w / nrm);
        }
    }
    if (dwindow) for (int n = 0; n < n_fft; ++n) dwindow[n] = (float)dw[n];
    return DMEL_OK;
}

dmel_status dmel_contraction_partition_host(const int32_t* units, int32_t n_tiles, int32_t waves, int32_t* own, int32_t* n_pieces,
                                            int32_t* piece_wave, int32_t* piece_tile, int32_t* piece_first, int32_t* piece_units)
{
    if (!units || !own || !n_pieces || !piece_wave || !piece_tile || !piece_first || !piece_units || (waves != 4 && waves != 8) ||
        n_tiles < 0 || n_tiles > waves)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_contraction_partition_host: bad arguments");
    int u[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
    for (int t = 0; t < n_tiles; ++t) { if (units[t] < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_contraction_partition_host: negative extent"); u[t] = units[t]; }
    std::vector<dmel::Piece> pieces;
    dmel::deal_ksteps(u, n_tiles, waves, o, &pieces);
    for (int w = 0; w < 8; ++w) own[w] = o[w];
    *n_pieces = (int32_t)pieces.size();
    for (size_t i = 0; i < pieces.size() && i < 8; ++i) {
        piece_wave[i] = pieces[i].wave; piece_tile[i] = pieces[i].tile; piece_first[i] = pieces[i].a; piece_units[i] = pieces[i].n;
    }
    return DMEL_OK;
}

dmel_status dmel_mel_fbanks_host(int32_t n_freqs, double f_min, double f_max, int32_t n_mels,
                                 int32_t sample_rate, float* fb)
{
    if (n_freqs < 1 || n_mels < 1 || sample_rate < 2 || !fb)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_mel_fbanks_host: bad arguments");
    dmel::mel_fbanks_htk(n_freqs, f_min, f_max, n_mels, sample_rate, fb);
    return DMEL_OK;
}

int32_t dmel_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

dmel_status dmel_plan_create(const dmel_config* cfg, dmel_plan** plan)
{
    if (!cfg || !plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "cfg / plan is NULL");
    *plan = nullptr;
    if (cfg->n_points < 1 || cfg->hop_length < 1 || cfg->n_mels < 1 || cfg->sample_rate < 2)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_points, hop_length, n_mels must be >= 1 and sample_rate >= 2");
    if (cfg->n_mels > 65535) return fail(DMEL_ERR_INVALID_ARGUMENT, "n_mels too large");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return fail(DMEL_ERR_NO_DEVICE, "no HIP device"); }
    hipDeviceProp_t prop;
    DMEL_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DMEL_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libdmel_hip is built for gfx950 only");
    DMEL_HIP(dmel::prepare_attributes());
    dmel_plan* pl = new (std::nothrow) dmel_plan();
    if (!pl) return fail(DMEL_ERR_OUT_OF_MEMORY, "host allocation failed");
    pl->cfg = *cfg;
    pl->device = dev;
    pl->T = cfg->n_points / cfg->hop_length + 1;                      // models.py:30
    pl->f_max = cfg->f_max < 0 ? (double)(cfg->sample_rate / 2) : cfg->f_max;   // models.py:25
    int nch = (cfg->n_points + 4095) / 4096;
    nch = std::max(1, std::min(nch, dmel::kMaxChunks));
    pl->nchunks = nch;
    pl->chunk = ((cfg->n_points + nch - 1) / nch + 3) / 4 * 4;   // multiple of 4 samples: chunks keep 16-byte alignment
    hipError_t e = hipEventCreateWithFlags(&pl->xev, hipEventDisableTiming);
    // two words the kernels write and the host reads without synchronising (device-resident lambd, dmel_forward_dev)
    constexpr size_t kHostWordBytes = (dmel::kLamRing + 8) * sizeof(unsigned long long);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&pl->host_words), kHostWordBytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&pl->exec_counter), 64);
    if (e == hipSuccess) e = hipMemset(pl->exec_counter, 0, 64);
    if (e != hipSuccess) { dmel_plan_destroy(pl); return fail(DMEL_ERR_HIP, std::string("plan resources: ") + hipGetErrorString(e)); }
    std::memset(pl->host_words, 0, kHostWordBytes);
    {
        Scratch sc;
        dmel_status st = ensure_own_scratch(pl, std::max(1, cfg->max_batch), nullptr, &sc);
        if (st != DMEL_OK) { dmel_plan_destroy(pl); return st; }
    }
    {
        std::lock_guard<std::mutex> lock(g_plans_mu);
        g_live_plans.insert(pl);
    }
    *plan = pl;
    return DMEL_OK;
}

int32_t dmel_lambd_ring_size(void) { return (int32_t)dmel::kLamRing; }

int32_t dmel_plan_is_live(const dmel_plan* plan)
{
    if (!plan) return 0;
    std::lock_guard<std::mutex> lock(g_plans_mu);
    return g_live_plans.count(plan) ? 1 : 0;
}

dmel_status dmel_plan_retain(dmel_plan* plan)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    std::lock_guard<std::mutex> lock(g_plans_mu);
    if (!g_live_plans.count(plan)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_retain: not a live plan (destroyed, or never created)");
    if (plan->refs < 1) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_retain: the plan has been destroyed");
    ++plan->refs;
    return DMEL_OK;
}

dmel_status dmel_plan_release(dmel_plan* plan)
{
    if (!plan) return DMEL_OK;
    {
        std::lock_guard<std::mutex> lock(g_plans_mu);
        if (--plan->refs > 0) return DMEL_OK;
        g_live_plans.erase(plan);          // from here on dmel_plan_is_live says no: a stale integer handle is refused, not dereferenced
    }
    // the last holder is gone.  Work that still reads the tables or writes the report words may be queued (a backward of a
    // graph that outlived its layer, the last launches of a loop): let the device finish before the memory goes away
    int cur = -1;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != plan->device && hipSetDevice(plan->device) == hipSuccess;
    (void)hipDeviceSynchronize();
    dmel::mailbox_attach_count(plan->mailbox, -1);       // after the synchronisation: no queued dot kernel of this plan polls it any more
    plan->mailbox = nullptr;
    for (auto& kv : plan->tables) kv.second.release();
    for (hipEvent_t e : plan->ev_pool) (void)hipEventDestroy(e);
    (void)hipFree(plan->own_scratch); (void)hipFree(plan->fbw); (void)hipFree(plan->xmw);
    plan->big_dev.release();
    (void)hipFree(plan->big_win); (void)hipFree(plan->big_z);
    (void)hipFree(plan->exec_counter);
    if (plan->host_words) (void)hipHostFree(plan->host_words);
    (void)hipFree(plan->multi_exec);
    if (plan->multi_words) (void)hipHostFree(plan->multi_words);
    if (plan->xev) (void)hipEventDestroy(plan->xev);
    if (switched) (void)hipSetDevice(cur);
    (void)hipGetLastError();
    delete plan;
    return DMEL_OK;
}

dmel_status dmel_plan_destroy(dmel_plan* plan) { return dmel_plan_release(plan); }

dmel_status dmel_plan_set_filterbank(dmel_plan* plan, int32_t n_fft, const float* fb)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (n_fft < 1 || n_fft > dmel::kMaxBigFft || (n_fft > 1 && (n_fft & 1)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be 1 or an even length up to 1048576");
    { dmel_status sd = check_device(plan); if (sd != DMEL_OK) return sd; }      // the synchronisation below must be the plan's device's
    std::lock_guard<std::mutex> lock(plan->mu);
    DMEL_HIP(hipDeviceSynchronize());     // tables of this n_fft may be in use by queued kernels
    auto it = plan->tables.find(n_fft);
    if (it != plan->tables.end()) { it->second.release(); plan->tables.erase(it); }
    plan->dense_dev.erase(n_fft);
    if (fb) {
        const size_t n = (size_t)(n_fft / 2 + 1) * plan->cfg.n_mels;
        plan->custom_fb[n_fft] = std::vector<float>(fb, fb + n);
    } else {
        plan->custom_fb.erase(n_fft);
    }
    return DMEL_OK;
}

dmel_status dmel_plan_set_filterbank_dev(dmel_plan* plan, int32_t n_fft, const float* fb_dev, void* stream)
{
    if (!plan || !fb_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan / fb_dev is NULL");
    if (n_fft < 1 || n_fft > dmel::kMaxBigFft || (n_fft > 1 && (n_fft & 1)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be 1 or an even length up to 1048576");
    { dmel_status sd = check_device(plan); if (sd != DMEL_OK) return sd; }
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!plan->dense_dev.count(n_fft)) {
        // first use for this n_fft: the tables get the dense structure (every 4x16 block present) once; from then on an update is
        // one small kernel on the caller's stream, no host copy and no synchronisation
        if (is_capturing(s)) return fail(DMEL_ERR_INVALID_ARGUMENT, "first dmel_plan_set_filterbank_dev for an n_fft builds tables: call it once before capturing");
        DMEL_HIP(hipDeviceSynchronize());
        auto it = plan->tables.find(n_fft);
        if (it != plan->tables.end()) { it->second.release(); plan->tables.erase(it); }
        plan->custom_fb.erase(n_fft);
        plan->dense_dev[n_fft] = true;
    }
    NfftTables* tb = nullptr;
    dmel_status st = build_tables(plan, n_fft, &tb);
    if (st != DMEL_OK) return st;
    dmel::RepackParams rp{};
    rp.fb = fb_dev; rp.ent_b = tb->ent_b; rp.ent_pre = tb->ent_pre; rp.tile_ranges = tb->tile_ranges;
    rp.fb_dense = tb->fb_dense; rp.fbT = tb->fbT; rp.rowpk = tb->rowpk; rp.F = tb->F; rp.M = plan->cfg.n_mels;
    rp.ent_h = tb->ent_h; rp.fb_nyq = tb->fb_nyq; rp.ks32 = tb->ent_h ? n_fft / 64 : 0;
    rp.wl_b4 = tb->wl_b4; rp.wl_lane = tb->wl_lane; rp.wl_total4 = tb->wl_total4; rp.wl_phases = tb->wl_phases;
    for (int i = 0; i < dmel::kWlMaxPhases; ++i) rp.wl_len4[i] = tb->wl_len4[i];
    const bool fast = n_fft >= dmel::kMinFastNfft && n_fft <= dmel::kMaxFastNfft;
    const int waves = fast ? dmel::forward_waves(n_fft) : 0;
    rp.runs = fast ? tb->groups * waves * 2 : 0;
    rp.runs_group0 = waves * 2;
    rp.nbpre = fast ? dmel::forward_nbpre(n_fft) : 0;
    DMEL_HIP(dmel::launch_repack(rp, s));
    return DMEL_OK;
}

dmel_status dmel_forward_scratch(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                                 double eps, void* out, float* tangent, void* scratch, void* stream)
{
    if (flags & DMEL_FLAG_X_INDIRECT) return fail(DMEL_ERR_INVALID_ARGUMENT, "DMEL_FLAG_X_INDIRECT belongs to dmel_forward_dev");
    { dmel_status sa = check_store_aligned("dmel_forward", {{"out", out}, {"tangent", tangent}, {"scratch", scratch}}); if (sa != DMEL_OK) return sa; }
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    if (flags & DMEL_FLAG_FULL_WINDOW) {
        if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
        c.flags = flags & ~DMEL_FLAG_FULL_WINDOW; c.win_half = 1;
        return run_forward(plan, c, lambd, nullptr, 2 * plan->cfg.n_points, scratch, stream);
    }
    return run_forward(plan, c, lambd, nullptr, 0, scratch, stream);
}

dmel_status dmel_forward(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                         double eps, float* out, float* tangent, void* stream)
{
    return dmel_forward_scratch(plan, x, batch, lambd, flags, eps, out, tangent, nullptr, stream);
}

dmel_status dmel_plan_get_config(const dmel_plan* plan, dmel_config* cfg)
{
    if (!plan || !cfg) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan / cfg is NULL");
    *cfg = plan->cfg;
    return DMEL_OK;
}

size_t dmel_scratch_bytes(const dmel_plan* plan, int32_t batch)
{
    if (!plan || batch < 0) return 0;
    return scratch_bytes(plan, batch);
}

static dmel_status forward_dev_fixed_issue(dmel_plan* plan, const FwdCall& c, const float* lambd_dev, int32_t n_fft, void* scratch, void* stream);

// dmel_forward_dev and dmel_forward_dev_lengths (c.lengths: the launches stay in the fused kernel's range): K = 1 of the host steps dmel_forward_multi_dev runs
static dmel_status forward_dev_impl(dmel_plan* plan, const FwdCall& c, const float* lambd_dev, void* scratch, void* stream)
{
    dmel_status st = check_forward_args(plan, c.x, c.batch, c.out);
    if (st != DMEL_OK) return st;
    if ((st = check_store_aligned(c.lengths ? "dmel_forward_dev_lengths" : "dmel_forward_dev", {{"out", c.out}, {"tangent", c.tangent}, {"scratch", scratch}})) != DMEL_OK) return st;
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    if (c.flags & DMEL_FLAG_FULL_WINDOW)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev: DMEL_FLAG_FULL_WINDOW has a fixed n_fft, use dmel_forward");
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool capturing = is_capturing(s);
    const Tracked t{&plan->track, plan->host_words, 1, false};
    const LamError e = take_errors(t);
    if (e.channel >= 0)
        return fail(DMEL_ERR_LAMBD_TRACKING,
                    "lambd moved from " + std::to_string(e.seen) + " (n_fft " + std::to_string(dmel_n_fft(e.seen)) + ") to " +
                    std::to_string(e.lam) + " (n_fft " + std::to_string(dmel_n_fft(e.lam)) + ") faster than the sync-free forward "
                    "tracks it: call " + std::to_string(e.seq) + " produced NaN.  Tracking has been reset; use "
                    "dmel_forward (host read per call), dmel_plan_set_tracking(plan, max_ahead, 1) or a smaller run-ahead");
    if (c.batch == 0) return DMEL_OK;
    if ((st = settle_pictures(plan, t, lambd_dev, s, capturing)) != DMEL_OK) return st;
    int N = 0, guards = 0;
    decide_scalar(plan, capturing, &N, &guards);
    if (c.lengths) {
        // clamped to the fused kernel's range, as dmel_forward_multi_dev: a forward whose lambd left it is poisoned and reported (without lengths: every length)
        N = std::min(std::max(N, dmel::kMinFastNfft), dmel::kMaxFastNfft);
        if (2 * N > dmel::kMaxFastNfft) guards &= ~2;
        if (N / 2 < dmel::kMinFastNfft) guards &= ~1;
    }
    if (!capturing && (st = prebuild_tables(plan, &N, 1, 1, dmel::kMaxBigFft)) != DMEL_OK) return st;     // (N and both neighbours whatever the guards; the multi-window layer: inside 32 ... 16384)
    int cand[3], nc = 0;
    cand[nc++] = N;
    if (guards & 2) cand[nc++] = 2 * N;
    if (guards & 1) cand[nc++] = N / 2;
    plan->track.last_guards = guards;       // (the launches issued; the multi-window layer records a channel's guards before its range cuts them)

    Scratch sc;
    if ((st = select_scratch(plan, scratch, c.batch, s, &sc)) != DMEL_OK) return st;
    count_call(plan, t, capturing);
    bool sums_done = false;
    return issue_group(plan, nc, [&](int i) {
        dmel::LamArgs lam = tracked_lam_args(lambd_dev, plan->exec_counter, plan->host_words, sc);
        lam.n_expected = cand[i];
        lam.role = (i == 0 ? dmel::kLamFirst : 0u) | (i == nc - 1 ? dmel::kLamLast : 0u);
        lam.dot_counter = scratch ? sc.counter : nullptr;
        return launch_forward_n(plan, cand[i], lam, c, sc, s, &sums_done);
    });
}

dmel_status dmel_forward_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, uint32_t flags,
                             double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_dev_impl(plan, mel_call(x, batch, flags, eps, out, tangent), lambd_dev, scratch, stream);
}

// the flags the per-clip-lengths forwards take
constexpr uint32_t kLengthsFlags = DMEL_FLAG_LOG | DMEL_FLAG_OUT_BF16 | DMEL_FLAG_X_INDIRECT;

dmel_status dmel_forward_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, float lambd, uint32_t flags,
                                 double eps, void* out, float* tangent, void* scratch, void* stream)
{
    if (!plan || !x || !lengths || !out) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_lengths: plan / x / lengths / out is NULL");
    if (flags & ~kLengthsFlags) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_lengths: flags other than LOG, OUT_BF16, X_INDIRECT");
    { dmel_status sa = check_store_aligned("dmel_forward_lengths", {{"out", out}, {"tangent", tangent}, {"scratch", scratch}}); if (sa != DMEL_OK) return sa; }
    if (!std::isfinite(lambd)) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
    const int N = dmel_n_fft(lambd);
    if (N < dmel::kMinFastNfft || N > dmel::kMaxFastNfft)
        return fail(DMEL_ERR_UNSUPPORTED, "per-clip lengths run n_fft 32 ... 16384; lambd = " + std::to_string(lambd) + " gives n_fft " + std::to_string(N));
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    c.lengths = lengths;
    return run_forward(plan, c, lambd, nullptr, 0, scratch, stream);
}

dmel_status dmel_forward_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                     uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    if (!plan || !x || !lengths || !out || !lambd_dev)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_lengths: plan / x / lengths / lambd_dev / out is NULL");
    if (flags & ~kLengthsFlags) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_lengths: flags other than LOG, OUT_BF16, X_INDIRECT");
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    c.lengths = lengths;
    return forward_dev_impl(plan, c, lambd_dev, scratch, stream);
}

dmel_status dmel_forward_dev_fixed(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                   uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return dmel_forward_dev_fixed_spec(plan, x, batch, lambd_dev, n_fft, flags, eps, out, tangent, nullptr, scratch, stream);
}

// spec == nullptr is dmel_forward_dev_fixed: its name in the messages, its wider range and its refusal of DMEL_FLAG_X_INDIRECT, which this form never had
dmel_status dmel_forward_dev_fixed_spec(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                        uint32_t flags, double eps, void* out, float* tangent, float* spec, void* scratch, void* stream)
{
    dmel_status st = check_forward_args(plan, x, batch, out);
    if (st != DMEL_OK) return st;
    if ((st = check_store_aligned(spec ? "dmel_forward_dev_fixed_spec" : "dmel_forward_dev_fixed",
                                  {{"out", out}, {"tangent", tangent}, {"spec", spec}, {"scratch", scratch}})) != DMEL_OK) return st;
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    c.spec_out = spec;
    if (spec) {
        if (!lambd_dev || !tangent) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_fixed_spec: lambd_dev / tangent is NULL (the training forward saves the spectrogram)");
        if (flags & DMEL_FLAG_FULL_WINDOW) return fail(DMEL_ERR_UNSUPPORTED, "dmel_forward_dev_fixed_spec: not with DMEL_FLAG_FULL_WINDOW");
        if (n_fft < dmel::kMinFastNfft || n_fft > dmel::kMaxNfft || (n_fft & (n_fft - 1)))
            return fail(DMEL_ERR_UNSUPPORTED, "dmel_forward_dev_fixed_spec: n_fft must be a power of two in [32, 16384]");
    } else {
        if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
        if (flags & DMEL_FLAG_X_INDIRECT) return fail(DMEL_ERR_INVALID_ARGUMENT, "DMEL_FLAG_X_INDIRECT belongs to dmel_forward_dev");
        if (flags & DMEL_FLAG_FULL_WINDOW) {
            // optimized=False (time_frequency.py:41,51): window = the clip, n_fft = 2 n_points whatever lambd is -- nothing to check on
            // the device, nothing for the host to read: lambd only shapes the window, which the kernels build from the device value
            c.flags = flags & ~DMEL_FLAG_FULL_WINDOW; c.win_half = 1;
            return run_forward(plan, c, 0.f, lambd_dev, 2 * plan->cfg.n_points, scratch, stream);
        }
        if (n_fft < 1 || n_fft > dmel::kMaxNfft || (n_fft & (n_fft - 1)))
            return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be a power of two in [1, 16384]");
    }
    return forward_dev_fixed_issue(plan, c, lambd_dev, n_fft, scratch, stream);
}

// the launch of the fixed-n_fft forwards (dmel_forward_dev_fixed, _spec, _lengths), their arguments checked: lambd is read and checked against n_fft on the device
static dmel_status forward_dev_fixed_issue(dmel_plan* plan, const FwdCall& c, const float* lambd_dev, int32_t n_fft, void* scratch, void* stream)
{
    dmel_status st = DMEL_OK;
    const int batch = c.batch;
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Tracked t{&plan->track, plan->host_words, 1, false};
    const LamError e = take_errors(t);
    if (e.channel >= 0)
        return fail(DMEL_ERR_LAMBD_TRACKING,
                    "lambd = " + std::to_string(e.lam) + " asks for n_fft " + std::to_string(dmel_n_fft(e.lam)) + " but the forward was issued for the "
                    "fixed n_fft " + std::to_string(n_fft) + " (a learnable filterbank is tied to one n_fft): call " +
                    std::to_string(e.seq) + " produced NaN");
    if (batch == 0) return DMEL_OK;
    Scratch sc;
    if ((st = select_scratch(plan, scratch, batch, s, &sc)) != DMEL_OK) return st;
    dmel::LamArgs lam = tracked_lam_args(lambd_dev, plan->exec_counter, plan->host_words, sc);
    lam.n_expected = n_fft;
    lam.role = dmel::kLamFirst | dmel::kLamLast;
    lam.dot_counter = scratch ? sc.counter : nullptr;
    count_call(plan, t, is_capturing(s));
    plan->track.last_guards = 0;
    bool sums_done = false;
    return launch_forward_n(plan, n_fft, lam, c, sc, s, &sums_done);
}

// dmel_forward_dev_fixed(_spec) over clips of per-clip lengths: the forward of a trained filterbank on a zero-padded batch
dmel_status dmel_forward_dev_fixed_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                           uint32_t flags, double eps, void* out, float* tangent, float* spec, void* scratch, void* stream)
{
    if (!plan || !x || !lengths || !out || !lambd_dev)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_fixed_lengths: plan / x / lengths / lambd_dev / out is NULL");
    if (spec && !tangent) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_fixed_lengths: tangent is NULL (the training forward saves the spectrogram)");
    if (flags & ~(DMEL_FLAG_LOG | DMEL_FLAG_OUT_BF16 | DMEL_FLAG_MFMA_BF16X3))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_dev_fixed_lengths: flags other than LOG, OUT_BF16, MFMA_BF16X3");
    dmel_status st = check_store_aligned("dmel_forward_dev_fixed_lengths", {{"out", out}, {"tangent", tangent}, {"spec", spec}, {"scratch", scratch}});
    if (st != DMEL_OK) return st;
    if (n_fft < dmel::kMinFastNfft || n_fft > dmel::kMaxFastNfft || (n_fft & (n_fft - 1)))
        return fail(DMEL_ERR_UNSUPPORTED, "dmel_forward_dev_fixed_lengths: n_fft must be a power of two in [32, 16384]");
    if ((st = check_forward_args(plan, x, batch, out)) != DMEL_OK) return st;
    FwdCall c = mel_call(x, batch, flags, eps, out, tangent);
    c.spec_out = spec; c.lengths = lengths; c.fb_len = true;
    return forward_dev_fixed_issue(plan, c, lambd_dev, n_fft, scratch, stream);
}

dmel_status dmel_plan_lambd_status(dmel_plan* plan, dmel_lambd_status* status)
{
    if (!plan || !status) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan / status is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    lt::observe(&plan->track, plan->host_words, dmel::kLamRing);
    dmel_lambd_status r{};
    lt::fill_status(plan->track, plan->host_words, dmel::kLamRing, &r);
    if (r.known) decide_scalar(plan, false, &r.next_n_fft, &r.next_guards);      // (a forced launch is what the next call issues)
    r.calls = plan->calls;
    *status = r;
    return DMEL_OK;
}

dmel_status dmel_plan_set_tracking(dmel_plan* plan, int32_t max_ahead, int32_t guard_mode)
{
    if (!plan || max_ahead < 0 || guard_mode < 0 || guard_mode > 3) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_set_tracking: bad arguments");
    std::lock_guard<std::mutex> lock(plan->mu);
    plan->max_ahead = max_ahead; plan->guard_mode = guard_mode;
    return DMEL_OK;
}

dmel_status dmel_plan_lambd_reset(dmel_plan* plan)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    lt::reset(&plan->track);
    for (auto& tr : plan->multi) lt::reset(&tr);
    return DMEL_OK;
}

dmel_status dmel_plan_lambd_report(dmel_plan* plan, uint32_t number, float* lambd, int32_t* found)
{
    if (!plan || !lambd || !found) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_lambd_report: NULL argument");
    const unsigned long long w = __atomic_load_n(&plan->host_words[number % dmel::kLamRing], __ATOMIC_RELAXED);
    *found = (number != 0 && (unsigned)(w >> 32) == number) ? 1 : 0;
    if (*found) { const unsigned bits = (unsigned)w; std::memcpy(lambd, &bits, 4); }
    return DMEL_OK;
}

dmel_status dmel_plan_force_launch(dmel_plan* plan, int32_t n_fft, int32_t guards)
{
    if (!plan || n_fft < 0 || guards < 0 || guards > 3) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_force_launch: bad arguments");
    if (n_fft > dmel::kMaxBigFft) return fail(DMEL_ERR_UNSUPPORTED, "n_fft beyond the HIP path");
    std::lock_guard<std::mutex> lock(plan->mu);
    plan->forced_n_fft = n_fft; plan->forced_guards = n_fft > 0 ? guards : 0;
    if (n_fft > 0 && 2 * n_fft > dmel::kMaxBigFft) plan->forced_guards &= ~2;
    if (n_fft > 0 && n_fft < 2) plan->forced_guards &= ~1;
    return DMEL_OK;
}

dmel_status dmel_decide_launch(float lambd, float rate, float stale_forwards, int32_t* n_fft, int32_t* guards)
{
    if (!n_fft || !guards || !(rate >= 0.f) || !(stale_forwards >= 0.f)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_decide_launch: bad arguments");
    int n = 0, g = 0;
    lt::decide_launch(lambd, rate, stale_forwards, &n, &g);
    *n_fft = n; *guards = g;
    return DMEL_OK;
}

// ---- the multi-window layer: K window widths as K output channels -----------------------------------------------------
// The launch choice: each channel's dmel_decide_launch, united.  Entries in ascending n_fft, each with the mask of the channels that need it.
dmel_status dmel_decide_launch_multi(const float* lambd, const float* rate, int32_t channels, float stale_forwards, int32_t* n_ffts,
                                     uint32_t* channel_masks, int32_t* count)
{
    if (!lambd || !rate || !n_ffts || !channel_masks || !count || channels < 1 || channels > dmel::kMaxChannels || !(stale_forwards >= 0.f))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_decide_launch_multi: bad arguments");
    int n[dmel::kMaxChannels], g[dmel::kMaxChannels];
    for (int c = 0; c < channels; ++c) {
        if (!(rate[c] >= 0.f)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_decide_launch_multi: rate < 0");
        lt::decide_launch(lambd[c], rate[c], stale_forwards, &n[c], &g[c]);
    }
    const LaunchList ll = group_by_nfft(n, g, channels, 0, 0x7fffffff);
    for (int i = 0; i < ll.nl; ++i) { n_ffts[i] = ll.ns[i]; channel_masks[i] = ll.mask[i]; }
    *count = ll.nl;
    return DMEL_OK;
}

size_t dmel_scratch_bytes_multi(const dmel_plan* plan, int32_t batch, int32_t channels)
{
    if (!plan || batch < 0 || channels < 1 || channels > dmel::kMaxChannels) return 0;
    return scratch_bytes_multi(plan, batch, channels);
}

namespace {

// the flags the multi-window and band-split forwards take
constexpr uint32_t kMultiFlags = DMEL_FLAG_LOG | DMEL_FLAG_OUT_BF16;

dmel_status check_multi_args(dmel_plan* pl, const FwdCall& c, void* scratch, const char* fn)
{
    const int channels = c.ml.channels;
    dmel_status st = check_forward_args(pl, c.x, c.batch, c.out);
    if (st != DMEL_OK) return st;
    if ((st = check_store_aligned(fn, {{"out", c.out}, {"tangent", c.tangent}, {"scratch", scratch}})) != DMEL_OK) return st;
    if (channels < 1 || channels > dmel::kMaxChannels) return fail(DMEL_ERR_INVALID_ARGUMENT, "channels must be 1 ... 8");
    if (c.flags & ~kMultiFlags)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_multi: only DMEL_FLAG_LOG and DMEL_FLAG_OUT_BF16 are accepted");
    if (c.batch > 0 && !scratch) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_multi: scratch (dmel_scratch_bytes_multi) is required");
    if ((long long)c.batch * channels > 65534) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch x channels > 65534 (split the call)");
    return DMEL_OK;
}

// one launch per entry of the list, its channels ascending; a channel's lambd roles are first / last among the launches that carry it (c.ml: the layer)
dmel_status issue_multi(dmel_plan* pl, const LaunchList& ll, const dmel::LamArgs& base, const FwdCall& c, const Scratch& sc, hipStream_t s)
{
    const int channels = c.ml.channels;
    int first[dmel::kMaxChannels], last[dmel::kMaxChannels];
    for (int ch = 0; ch < channels; ++ch) { first[ch] = -1; last[ch] = -1; }
    pl->last_multi_nl = ll.nl;                       // (host code: runs under capture too)
    for (int i = 0; i < ll.nl; ++i) { pl->last_multi_ns[i] = ll.ns[i]; pl->last_multi_mask[i] = ll.mask[i]; }
    for (int i = 0; i < ll.nl; ++i)
        for (int ch = 0; ch < channels; ++ch)
            if (ll.mask[i] >> ch & 1u) { if (first[ch] < 0) first[ch] = i; last[ch] = i; }
    bool sums_done = false;
    return issue_group(pl, ll.nl, [&](int i) {
        FwdCall q = c;
        for (int ch = 0; ch < channels; ++ch) {
            if (!(ll.mask[i] >> ch & 1u)) continue;
            const unsigned role = (first[ch] == i ? dmel::kLamFirst : 0u) | (last[ch] == i ? dmel::kLamLast : 0u);
            q.ml.list |= (unsigned)ch << (4 * q.ml.count);
            q.ml.roles |= role << (4 * q.ml.count);
            ++q.ml.count;
        }
        dmel::LamArgs lam = base;
        lam.n_expected = base.n_expected ? ll.ns[i] : 0;
        if (i != 0) lam.dot_counter = nullptr;
        return launch_forward_n(pl, ll.ns[i], lam, q, sc, s, &sums_done);
    });
}

// K validated band edges, taken by value (they travel in the kernel arguments)
struct BandEdges { int32_t e[dmel::kMaxChannels + 1] = {}; };

// 0 = e_0 < e_1 < ... < e_K = n_mels (every group non-empty)
// (the part of take_band_edges that needs no plan)
dmel_status band_edges_shape(const int32_t* edges, int channels, const char* who)
{
    if (channels < 1 || channels > dmel::kMaxChannels) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": channels must be 1 ... 8");
    if (!edges) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": band_edges is NULL");
    if (edges[0] != 0) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": band_edges must start at 0");
    for (int c = 0; c < channels; ++c)
        if (edges[c + 1] <= edges[c])
            return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": band_edges must be strictly ascending (group " + std::to_string(c) + " is empty)");
    return DMEL_OK;
}

dmel_status take_band_edges(const dmel_plan* pl, const int32_t* edges, int channels, const char* who, BandEdges* out)
{
    if (const dmel_status st = band_edges_shape(edges, channels, who); st != DMEL_OK) return st;
    if (!pl) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (edges[channels] != pl->cfg.n_mels)
        return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": band_edges must end at n_mels = " + std::to_string(pl->cfg.n_mels) + " (got " +
                    std::to_string(edges[channels]) + ")");
    for (int c = 0; c <= channels; ++c) out->e[c] = edges[c];
    return DMEL_OK;
}

dmel_status forward_multi_impl(dmel_plan* plan, FwdCall c, const float* lambd_host, void* scratch, void* stream)
{
    const int channels = c.ml.channels;
    dmel_status st = check_multi_args(plan, c, scratch, c.ml.edges ? "dmel_forward_band" : "dmel_forward_multi");
    if (st != DMEL_OK) return st;
    if (!lambd_host) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_host is NULL");
    if ((st = check_lambd_multi(lambd_host, channels)) != DMEL_OK) return st;
    if (c.batch == 0) return DMEL_OK;
    std::lock_guard<std::mutex> lock(plan->mu);
    const LaunchList ll = group_host_values(lambd_host, channels);
    for (int ch = 0; ch < channels; ++ch) c.ml.vals[ch] = lambd_host[ch];
    const Scratch sc = carve(scratch, channels);
    dmel::LamArgs base{};
    base.n_expected = 0;                          // every n_fft was derived from these very values
    base.dot_counter = sc.counter;
    return issue_multi(plan, ll, base, c, sc, reinterpret_cast<hipStream_t>(stream));
}

dmel_status forward_multi_dev_impl(dmel_plan* plan, FwdCall c, const float* lambd_dev, void* scratch, void* stream)
{
    const int channels = c.ml.channels;
    dmel_status st = check_multi_args(plan, c, scratch, c.ml.edges ? "dmel_forward_band_dev" : "dmel_forward_multi_dev");
    if (st != DMEL_OK) return st;
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool capturing = is_capturing(s);
    if (!plan->multi_words) {
        if (capturing) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_forward_multi_dev: run the layer once eagerly before capturing it into a graph");
        const size_t bytes = (size_t)dmel::kMaxChannels * dmel::kLamMultiStride * sizeof(unsigned long long);
        DMEL_HIP(hipHostMalloc(reinterpret_cast<void**>(&plan->multi_words), bytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(plan->multi_words, 0, bytes);
        DMEL_HIP(hipMalloc(reinterpret_cast<void**>(&plan->multi_exec), dmel::kMaxChannels * sizeof(unsigned)));
        DMEL_HIP(hipMemset(plan->multi_exec, 0, dmel::kMaxChannels * sizeof(unsigned)));
    }
    const Tracked t{plan->multi, plan->multi_words, channels, true};
    // a channel that no launch covered: NaN in that channel on the device; tell the caller once, naming it (that channel has started over)
    const LamError e = take_errors(t);
    if (e.channel >= 0)
        return fail(DMEL_ERR_LAMBD_TRACKING,
                    "channel " + std::to_string(e.channel) + ": lambd moved from " + std::to_string(e.seen) + " (n_fft " + std::to_string(dmel_n_fft(e.seen)) +
                    ") to " + std::to_string(e.lam) + " (n_fft " + std::to_string(dmel_n_fft(e.lam)) + ") where no launch of the sync-free forward "
                    "covered it (or out of the range 32 ... 16384): execution " + std::to_string(e.seq) + " of that channel "
                    "produced NaN in it.  Its tracking has been reset");
    if (c.batch == 0) return DMEL_OK;
    if ((st = settle_pictures(plan, t, lambd_dev, s, capturing)) != DMEL_OK) return st;
    // each channel's launches, clamped to the range the fused kernel serves (a channel whose lambd left it is then poisoned and reported)
    int n[dmel::kMaxChannels], g[dmel::kMaxChannels];
    for (int ch = 0; ch < channels; ++ch) {
        lt::decide(plan->multi[ch], plan->guard_mode, plan->max_ahead, capturing, &n[ch], &g[ch]);
        plan->multi[ch].last_guards = g[ch];     // (as decided: a guard outside 32 ... 16384 is recorded and not launched; the scalar layer records its launches)
        n[ch] = std::min(std::max(n[ch], dmel::kMinFastNfft), dmel::kMaxFastNfft);
    }
    const LaunchList ll = group_by_nfft(n, g, channels, dmel::kMinFastNfft, dmel::kMaxFastNfft);
    if (!capturing && (st = prebuild_tables(plan, ll.ns, ll.nl, dmel::kMinFastNfft, dmel::kMaxFastNfft)) != DMEL_OK) return st;
    count_call(plan, t, capturing);
    const Scratch sc = carve(scratch, channels);
    dmel::LamArgs base = tracked_lam_args(lambd_dev, plan->multi_exec, plan->multi_words, sc);
    base.n_expected = 1;                          // (issue_multi: check against the n_fft of each launch)
    base.dot_counter = sc.counter;
    return issue_multi(plan, ll, base, c, sc, s);
}

// The eight K-window forwards are named multi | band, [_dev], [_lengths]; `form` says which: kFormDev (lambd on the device: tracked), kFormBand (c.ml.edges,
// the caller's host integers, validated and taken by value), kFormLengths (the NULL and flag checks of those forms first, before the plan is looked at)
constexpr unsigned kFormDev = 1u, kFormBand = 2u, kFormLengths = 4u;
dmel_status forward_k(const char* who, unsigned form, dmel_plan* plan, FwdCall c, const int32_t* lengths, const float* lambd, void* scratch, void* stream)
{
    c.lengths = lengths;
    if (form & kFormLengths) {
        if (!plan || !c.x || !c.lengths || !c.out) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": plan / x / lengths / out is NULL");
        if (c.flags & ~kMultiFlags) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": flags other than LOG, OUT_BF16");
    }
    BandEdges be;
    if (form & kFormBand) {
        const dmel_status st = take_band_edges(plan, c.ml.edges, c.ml.channels, who, &be);
        if (st != DMEL_OK) return st;
        c.ml.edges = be.e; c.ml.ch_out = 1;
    }
    return (form & kFormDev) ? forward_multi_dev_impl(plan, c, lambd, scratch, stream) : forward_multi_impl(plan, c, lambd, scratch, stream);
}

}  // namespace

dmel_status dmel_forward_multi(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels, uint32_t flags,
                               double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_multi", 0u, plan, k_call(x, batch, channels, nullptr, flags, eps, out, tangent), nullptr, lambd_host, scratch, stream);
}

dmel_status dmel_forward_multi_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels, uint32_t flags,
                                   double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_multi_dev", kFormDev, plan, k_call(x, batch, channels, nullptr, flags, eps, out, tangent), nullptr, lambd_dev, scratch, stream);
}

dmel_status dmel_forward_multi_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                       int32_t channels, uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_multi_lengths", kFormLengths, plan, k_call(x, batch, channels, nullptr, flags, eps, out, tangent), lengths, lambd_host, scratch, stream);
}

dmel_status dmel_forward_multi_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                           int32_t channels, uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_multi_dev_lengths", kFormDev | kFormLengths, plan, k_call(x, batch, channels, nullptr, flags, eps, out, tangent), lengths, lambd_dev, scratch, stream);
}

dmel_status dmel_forward_band(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels, const int32_t* band_edges,
                              uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_band", kFormBand, plan, k_call(x, batch, channels, band_edges, flags, eps, out, tangent), nullptr, lambd_host, scratch, stream);
}

dmel_status dmel_forward_band_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels, const int32_t* band_edges,
                                  uint32_t flags, double eps, void* out, float* tangent, void* scratch, void* stream)
{
    return forward_k("dmel_forward_band_dev", kFormDev | kFormBand, plan, k_call(x, batch, channels, band_edges, flags, eps, out, tangent), nullptr, lambd_dev, scratch, stream);
}

dmel_status dmel_forward_band_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                      int32_t channels, const int32_t* band_edges, uint32_t flags, double eps, void* out, float* tangent,
                                      void* scratch, void* stream)
{
    return forward_k("dmel_forward_band_lengths", kFormBand | kFormLengths, plan, k_call(x, batch, channels, band_edges, flags, eps, out, tangent), lengths, lambd_host, scratch, stream);
}

dmel_status dmel_forward_band_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                          int32_t channels, const int32_t* band_edges, uint32_t flags, double eps, void* out, float* tangent,
                                          void* scratch, void* stream)
{
    return forward_k("dmel_forward_band_dev_lengths", kFormDev | kFormBand | kFormLengths, plan, k_call(x, batch, channels, band_edges, flags, eps, out, tangent), lengths, lambd_dev, scratch, stream);
}

namespace {

// what the dot entry points refuse alike, each under its own name
dmel_status check_grad_dtype(int32_t grad_dtype, const char* who)
{
    if (grad_dtype == DMEL_DTYPE_F32 || grad_dtype == DMEL_DTYPE_BF16) return DMEL_OK;
    return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": grad_dtype must be DMEL_DTYPE_F32 or DMEL_DTYPE_BF16");
}

// the reducers that live in the scalar layer's dot kernel
dmel_status check_scalar_reducers_only(const dmel_plan* plan, const char* who)
{
    if (!plan->mailbox && !plan->fused_adam.param) return DMEL_OK;
    return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(who) + ": a plan with an attached mailbox or fused Adam serves the scalar layer only");
}

}  // namespace

dmel_status dmel_backward_band(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int32_t batch, int32_t channels,
                               const int32_t* band_edges, int32_t accumulate, float* dlambd, void* scratch, void* stream)
{
    BandEdges be;
    dmel_status st = take_band_edges(plan, band_edges, channels, "dmel_backward_band", &be);
    if (st != DMEL_OK) return st;
    if (batch < 0 || !dlambd || !scratch || (batch > 0 && (!grad_out || !tangent)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_band: bad arguments");
    if ((st = check_store_aligned("dmel_backward_band", {{"scratch", scratch}})) != DMEL_OK) return st;
    if ((st = check_grad_dtype(grad_dtype, "dmel_backward_band")) != DMEL_OK) return st;
    if ((st = check_scalar_reducers_only(plan, "dmel_backward_band")) != DMEL_OK) return st;
    if ((st = check_device(plan)) != DMEL_OK) return st;
    if ((long long)batch * plan->cfg.n_mels * plan->T >= (1LL << 31)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_band: more than 2^31 elements");
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Scratch sc = carve(scratch, channels);
    dmel::DotBandParams dp{};
    dp.g = grad_out; dp.t = tangent; dp.partials = sc.partials; dp.counter = sc.counter; dp.result = dlambd;
    dp.g_bf16 = grad_dtype == DMEL_DTYPE_BF16; dp.batch = batch; dp.channels = channels; dp.M = plan->cfg.n_mels; dp.T = plan->T;
    dp.accumulate = accumulate;
    for (int c = 0; c <= dmel::kMaxChannels; ++c) dp.edges[c] = be.e[std::min(c, channels)];
    // at most kDotMaxBlocks partials in all (the ticket tree's layout), dealt to the groups in proportion to their rows
    dmel::dot_band_deal(dp.edges, channels, batch, plan->T, dp.blocks);
    const size_t m0 = prof_mark(plan, s);
    DMEL_HIP(dmel::launch_dot_band(dp, s));
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}

dmel_status dmel_backward_multi(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int32_t batch, int32_t channels,
                                int32_t accumulate, float* dlambd, void* scratch, void* stream)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (batch < 0 || channels < 1 || channels > dmel::kMaxChannels || !dlambd || !scratch || (batch > 0 && (!grad_out || !tangent)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_multi: bad arguments");
    dmel_status st = check_store_aligned("dmel_backward_multi", {{"scratch", scratch}});
    if (st != DMEL_OK) return st;
    if ((st = check_grad_dtype(grad_dtype, "dmel_backward_multi")) != DMEL_OK) return st;
    if ((st = check_scalar_reducers_only(plan, "dmel_backward_multi")) != DMEL_OK) return st;
    if ((st = check_device(plan)) != DMEL_OK) return st;
    const long long per_row = (long long)plan->cfg.n_mels * plan->T;
    if ((long long)batch * per_row >= (1LL << 31)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_multi: more than 2^31 elements per channel");
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Scratch sc = carve(scratch, channels);
    // the ticket tree holds at most kDotMaxBlocks partials in all (its group counters live in the upper half of the partials array)
    const int bpc = dmel::dot_multi_blocks_per_channel((long long)batch * per_row, channels);
    if ((long long)bpc * channels > dmel::kDotMaxBlocks) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_multi: too many partials");
    const size_t m0 = prof_mark(plan, s);
    DMEL_HIP(dmel::launch_dot_multi(grad_out, grad_dtype == DMEL_DTYPE_BF16, tangent, batch, channels, per_row, bpc, accumulate,
                                    sc.partials, sc.counter, dlambd, s));
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}

dmel_status dmel_plan_lambd_status_channel(dmel_plan* plan, int32_t channel, dmel_lambd_status* status)
{
    if (!plan || !status || channel < 0 || channel >= dmel::kMaxChannels)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_lambd_status_channel: bad arguments");
    std::lock_guard<std::mutex> lock(plan->mu);
    dmel_lambd_status r{};
    if (plan->multi_words) {
        const Tracked t{plan->multi, plan->multi_words, dmel::kMaxChannels, true};
        lt::observe(&t.tr[channel], t.ring(channel), dmel::kLamRing);
        lt::fill_status(t.tr[channel], t.ring(channel), dmel::kLamRing, &r);
        if (r.known) lt::decide(t.tr[channel], plan->guard_mode, plan->max_ahead, false, &r.next_n_fft, &r.next_guards);
    }
    r.calls = plan->calls;
    *status = r;
    return DMEL_OK;
}

dmel_status dmel_spectrogram(dmel_plan* plan, const float* x, int32_t batch, float lambd,
                             int32_t remove_dc, float* spec, void* stream)
{
    { dmel_status sa = check_store_aligned("dmel_spectrogram", {{"spec", spec}}); if (sa != DMEL_OK) return sa; }
    return run_forward(plan, spec_call(x, batch, spec, nullptr, remove_dc ? DMEL_SPEC_REMOVE_DC : 0u), lambd, nullptr, 0, nullptr, stream);
}

dmel_status dmel_spectrogram_ex(dmel_plan* plan, const float* x, int32_t batch, float lambd, int32_t n_fft,
                                uint32_t flags, float* spec, float* tangent, void* stream)
{
    if (n_fft < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft < 0");
    { dmel_status sa = check_store_aligned("dmel_spectrogram_ex", {{"spec", spec}, {"tangent", tangent}}); if (sa != DMEL_OK) return sa; }
    return run_forward(plan, spec_call(x, batch, spec, tangent, flags), lambd, nullptr, n_fft, nullptr, stream);
}

dmel_status dmel_spectrogram_ex_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                    uint32_t flags, float* spec, float* tangent, void* stream)
{
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    { dmel_status sa = check_store_aligned("dmel_spectrogram_ex_dev", {{"spec", spec}, {"tangent", tangent}}); if (sa != DMEL_OK) return sa; }
    if (n_fft <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_spectrogram_ex_dev: n_fft must be given (a length that depends on lambd needs the host value: dmel_spectrogram_ex)");
    return run_forward(plan, spec_call(x, batch, spec, tangent, flags), 0.f, lambd_dev, n_fft, nullptr, stream);
}

dmel_status dmel_backward_ex(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int64_t count,
                             int32_t accumulate, float* dlambd, void* stream)
{
    // (dmel_backward_scratch's first two checks, ahead of the one message that carries this function's name)
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (count < 0 || !dlambd || (count > 0 && (!grad_out || !tangent))) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward: bad arguments");
    const dmel_status st = check_grad_dtype(grad_dtype, "dmel_backward_ex");
    return st != DMEL_OK ? st : dmel_backward_scratch(plan, grad_out, grad_dtype, tangent, count, accumulate, dlambd, nullptr, stream);
}

dmel_status dmel_backward_scratch(dmel_plan* plan, const void* grad_out, int32_t grad_dtype, const float* tangent, int64_t count,
                                  int32_t accumulate, float* dlambd, void* scratch, void* stream)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (count < 0 || !dlambd || (count > 0 && (!grad_out || !tangent))) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward: bad arguments");
    dmel_status st = check_grad_dtype(grad_dtype, "dmel_backward");
    if (st != DMEL_OK) return st;
    if ((st = check_store_aligned("dmel_backward", {{"scratch", scratch}})) != DMEL_OK) return st;
    if ((st = check_device(plan)) != DMEL_OK) return st;
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc;
    if ((st = select_scratch(plan, scratch, 1, s, &sc)) != DMEL_OK) return st;
    dmel::MailboxArgs mba;
    const bool use_mb = plan->mailbox != nullptr;
    if (use_mb && !dmel::mailbox_args(plan->mailbox, &mba)) return fail(DMEL_ERR_INVALID_ARGUMENT, "the plan's mailbox is not connected");
    if (use_mb && (st = mailbox_status(plan)) != DMEL_OK) return st;
    const size_t m0 = prof_mark(plan, s);
    DMEL_HIP(dmel::launch_dot(grad_out, grad_dtype == DMEL_DTYPE_BF16, tangent, (long long)count, accumulate, sc.partials,
                              sc.counter, kMaxPartials, dlambd, s, use_mb ? &mba : nullptr, plan->fused_adam.param ? &plan->fused_adam : nullptr));
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}

dmel_status dmel_plan_attach_adam(dmel_plan* plan, float* param, float* exp_avg, float* exp_avg_sq, float* step,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int32_t maximize)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    if (!param) { plan->fused_adam = dmel::AdamParams{}; return DMEL_OK; }
    if (!exp_avg || !exp_avg_sq || !step) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_attach_adam: NULL state pointer");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(lr) || !(lr >= 0.0) ||
        !std::isfinite(weight_decay) || !(weight_decay >= 0.0))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_attach_adam: lr / betas / eps / weight_decay out of range");
    dmel::AdamParams ap{};
    ap.param = param; ap.grad = nullptr; ap.exp_avg = exp_avg; ap.exp_avg_sq = exp_avg_sq; ap.step = step; ap.ticket = nullptr;
    ap.n = 1; ap.maximize = maximize ? 1 : 0;
    ap.lr = lr; ap.beta1 = beta1; ap.beta2 = beta2; ap.eps = eps; ap.weight_decay = weight_decay;
    plan->fused_adam = ap;
    return DMEL_OK;
}

dmel_status dmel_plan_attach_mailbox(dmel_plan* plan, dmel_mailbox* mb)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (mb && dmel::mailbox_device(mb) != plan->device) return fail(DMEL_ERR_INVALID_ARGUMENT, "the mailbox and the plan live on different devices");
    std::lock_guard<std::mutex> lock(plan->mu);
    if (plan->mailbox == mb) return DMEL_OK;
    dmel::mailbox_attach_count(plan->mailbox, -1);       // the mailbox counts its plans: dmel_mailbox_destroy refuses while any holds it
    dmel::mailbox_attach_count(mb, +1);
    plan->mailbox = mb;
    return DMEL_OK;
}

dmel_status dmel_backward(dmel_plan* plan, const float* grad_out, const float* tangent, int64_t count,
                          int32_t accumulate, float* dlambd, void* stream)
{
    return dmel_backward_ex(plan, grad_out, DMEL_DTYPE_F32, tangent, count, accumulate, dlambd, stream);
}

namespace {
// lambd by value (lambd_dev == nullptr; n_fft derived from it) or on the device with the n_fft the caller's forward was issued for; saved_spec: the (batch,
// n_fft_dev/2+1, n_time) power spectrogram the training forward wrote: no recompute; dlambd: d lambd computed in the same launch (dmel_backward_fb_saved_dl)
struct FbGradCall {
    const float* x = nullptr; int batch = 0; float lambd = 0.f; const float* lambd_dev = nullptr; int n_fft_dev = 0; uint32_t flags = 0;
    const float* grad_out = nullptr; const float* out = nullptr; float* grad_fb = nullptr; const float* saved_spec = nullptr;
    const float* tangent = nullptr; float* dlambd = nullptr; void* scratch = nullptr;
    const int32_t* lengths = nullptr;       // per-clip lengths (device): dmel_backward_fb_dev_lengths, dmel_backward_fb_saved_lengths
};

dmel_status backward_fb_impl(dmel_plan* plan, const FbGradCall& c, void* stream)
{
    const int batch = c.batch;
    const bool rider = c.dlambd != nullptr;
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (batch < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch < 0");
    if (!c.grad_fb || (batch > 0 && ((!c.x && !c.saved_spec) || !c.grad_out))) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_fb: x / grad_out / grad_fb is NULL");
    if ((c.flags & DMEL_FLAG_LOG) && batch > 0 && !c.out)
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_fb: DMEL_FLAG_LOG needs the saved log output");
    { dmel_status sa = check_store_aligned("dmel_backward_fb", {{"grad_fb", c.grad_fb}, {"scratch", c.scratch}}); if (sa != DMEL_OK) return sa; }
    if (!c.lambd_dev && !c.saved_spec && !std::isfinite(c.lambd)) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
    const bool full = (c.flags & DMEL_FLAG_FULL_WINDOW) != 0;
    if (c.lambd_dev && !full && (c.n_fft_dev < 1 || c.n_fft_dev > dmel::kMaxNfft || (c.n_fft_dev & (c.n_fft_dev - 1))))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be a power of two in [1, 16384]");
    const int n_over = full ? 2 * plan->cfg.n_points : 0;     // any clip length: the spectrogram pass takes the chirp-z path where it has to
    const int N = n_over ? n_over : ((c.lambd_dev || c.saved_spec) ? c.n_fft_dev : dmel_n_fft(c.lambd));
    if (N > dmel::kMaxBigFft)
        return fail(DMEL_ERR_UNSUPPORTED, "n_fft = " + std::to_string(N) + " > " + std::to_string(dmel::kMaxBigFft) + " is not supported by the HIP kernels");
    const int F = N / 2 + 1, M = plan->cfg.n_mels, T = plan->T;
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (batch == 0) { DMEL_HIP(hipMemsetAsync(c.grad_fb, 0, (size_t)F * M * sizeof(float), s)); return DMEL_OK; }
    dmel_status st = order_after_last_stream(plan, s);       // fbw is shared by every call on the plan
    if (st != DMEL_OK) return st;
    int splits = dmel::fbgrad_splits(batch, F, M, T);
    // d lambd rides along unless the plan's reducer lives in the dot kernel (mailbox) or the launch has no room for it
    Scratch rsc;
    int dot_wgs = 0, dot_vblocks = 0;
    const long long dot_count = (long long)batch * M * T;
    if (rider) {
        if ((st = select_scratch(plan, c.scratch, batch, s, &rsc)) != DMEL_OK) return st;
        if (!plan->mailbox) {
            dot_vblocks = dmel::dot_blocks_for(dot_count, kMaxPartials);
            const int left = dmel::fbgrad_fuse_dot(F, M, splits, dot_vblocks, &dot_wgs);
            if (left > 0) splits = left; else dot_wgs = 0;
        }
    }
    const size_t spec_floats = c.saved_spec ? 0 : ((size_t)batch * F * T + 63) / 64 * 64;
    const size_t part_floats = ((size_t)splits * F * M + 63) / 64 * 64;     // (gm = grad_out * exp(-out) is formed inside the GEMM kernel)
    if ((st = grow_floats(&plan->fbw, &plan->fbw_floats, spec_floats + part_floats, s, "")) != DMEL_OK) return st;
    // the spectrogram the layer contracted at models.py:53 (DC removed, models.py:38): P is recomputed, not saved
    FwdCall sp = spec_call(c.x, batch, plan->fbw, nullptr, DMEL_SPEC_REMOVE_DC | (full ? DMEL_SPEC_HALF_WINDOW : 0u));
    sp.lengths = c.lengths; sp.fb_len = c.lengths != nullptr;      // (the recompute pass over clips of Lc samples: dmel_fwd_fb_len_kernel, kSpec)
    if (c.saved_spec) {
        st = DMEL_OK;
    } else if (c.lambd_dev && !full) {
        // lambd read on the device and checked against N: a mismatch (the forward of this step reported it) leaves NaN here too
        Scratch sc;
        if ((st = ensure_own_scratch(plan, batch, s, &sc)) != DMEL_OK) return st;
        dmel::LamArgs lam{};
        lam.dev = c.lambd_dev; lam.n_expected = N; lam.role = dmel::kLamFirst | dmel::kLamLast;
        bool sums_done = false;
        st = launch_forward_n(plan, N, lam, sp, sc, s, &sums_done);
    } else {
        // (on the device: n_fft = 2 n_points does not depend on lambd: the kernels take the window's width from the device value, nothing to check)
        st = run_forward_nolock(plan, sp, c.lambd_dev ? 0.f : c.lambd, c.lambd_dev, n_over, nullptr, stream);
    }
    if (st != DMEL_OK) return st;
    dmel::FbGradParams fp{};
    fp.spec = c.saved_spec ? c.saved_spec : plan->fbw; fp.grad_out = c.grad_out; fp.out = (c.flags & DMEL_FLAG_LOG) ? c.out : nullptr;
    fp.partials = plan->fbw + spec_floats; fp.grad_fb = c.grad_fb;
    fp.gm_ws = plan->fbw + spec_floats + part_floats;
    fp.B = batch; fp.F = F; fp.M = M; fp.T = T; fp.splits = splits;
    fp.bf16x3 = (c.flags & DMEL_FLAG_MFMA_BF16X3) ? 1 : 0;
    fp.lengths = c.lengths; fp.hop = plan->cfg.hop_length;
    if (dot_wgs > 0) {
        fp.dot_g = c.grad_out; fp.dot_t = c.tangent; fp.dot_count = dot_count; fp.dot_partials = rsc.partials; fp.dot_counter = rsc.counter;
        fp.dot_result = c.dlambd; fp.dot_vblocks = dot_vblocks; fp.dot_wgs = dot_wgs; fp.dot_accumulate = 0;
    }
    const size_t m0 = prof_mark(plan, s);
    DMEL_HIP(dmel::launch_fbgrad(fp, s));
    if (rider && dot_wgs == 0) {
        // the stand-alone kernel (dmel_backward_scratch): the mailbox exchange lives there
        dmel::MailboxArgs mba;
        const bool use_mb = plan->mailbox != nullptr;
        if (use_mb && !dmel::mailbox_args(plan->mailbox, &mba)) return fail(DMEL_ERR_INVALID_ARGUMENT, "the plan's mailbox is not connected");
        if (use_mb) { dmel_status ms = mailbox_status(plan); if (ms != DMEL_OK) return ms; }
        DMEL_HIP(dmel::launch_dot(c.grad_out, 0, c.tangent, dot_count, 0, rsc.partials, rsc.counter, kMaxPartials, c.dlambd, s,
                                  use_mb ? &mba : nullptr));
    }
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}
}  // namespace

dmel_status dmel_backward_fb(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                             const float* grad_out, const float* out, float* grad_fb, void* stream)
{
    FbGradCall c;
    c.x = x; c.batch = batch; c.lambd = lambd; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb;
    return backward_fb_impl(plan, c, stream);
}

dmel_status dmel_backward_fb_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                 const float* grad_out, const float* out, float* grad_fb, void* stream)
{
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    FbGradCall c;
    c.x = x; c.batch = batch; c.lambd_dev = lambd_dev; c.n_fft_dev = n_fft; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb;
    return backward_fb_impl(plan, c, stream);
}

dmel_status dmel_backward_fb_saved(dmel_plan* plan, const float* spec, int32_t batch, int32_t n_fft, uint32_t flags,
                                   const float* grad_out, const float* out, float* grad_fb, void* stream)
{
    if (!spec) return fail(DMEL_ERR_INVALID_ARGUMENT, "spec is NULL");
    if (flags & DMEL_FLAG_FULL_WINDOW) return fail(DMEL_ERR_UNSUPPORTED, "dmel_backward_fb_saved: not with DMEL_FLAG_FULL_WINDOW");
    if (n_fft < 2 || (n_fft & 1)) return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be the (even) transform length the spectrogram was computed with");
    FbGradCall c;
    c.batch = batch; c.n_fft_dev = n_fft; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb; c.saved_spec = spec;
    return backward_fb_impl(plan, c, stream);
}

dmel_status dmel_backward_fb_saved_dl(dmel_plan* plan, const float* spec, int32_t batch, int32_t n_fft, uint32_t flags,
                                      const float* grad_out, const float* out, const float* tangent, float* grad_fb, float* dlambd,
                                      void* scratch, void* stream)
{
    if (!spec) return fail(DMEL_ERR_INVALID_ARGUMENT, "spec is NULL");
    if (!tangent || !dlambd) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_fb_saved_dl: tangent / dlambd is NULL");
    if (batch <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_fb_saved_dl: batch must be positive");
    if (flags & DMEL_FLAG_FULL_WINDOW) return fail(DMEL_ERR_UNSUPPORTED, "dmel_backward_fb_saved_dl: not with DMEL_FLAG_FULL_WINDOW");
    if (n_fft < 2 || (n_fft & 1)) return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be the (even) transform length the spectrogram was computed with");
    FbGradCall c;
    c.batch = batch; c.n_fft_dev = n_fft; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb; c.saved_spec = spec;
    c.tangent = tangent; c.dlambd = dlambd; c.scratch = scratch;
    return backward_fb_impl(plan, c, stream);
}

// the two filterbank gradients over clips of per-clip lengths: the recompute path (a kSpec pass with lengths in front of the GEMM) and the saved spectrogram
static dmel_status fb_lengths_args(const char* who, dmel_plan* plan, const void* first, const int32_t* lengths, int32_t batch, int32_t n_fft, uint32_t flags,
                                   const float* grad_out, const float* out, float* grad_fb)
{
    const std::string w(who);
    if (!plan || !first || !lengths || !grad_out || !grad_fb)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": plan / " + (w.find("saved") != std::string::npos ? "spec" : "x / lambd_dev") + " / lengths / grad_out / grad_fb is NULL");
    if (batch <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": batch must be positive");
    if (flags & ~(DMEL_FLAG_LOG | DMEL_FLAG_MFMA_BF16X3)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": flags other than LOG, MFMA_BF16X3");
    if ((flags & DMEL_FLAG_LOG) && !out) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": DMEL_FLAG_LOG needs the saved log output");
    if (n_fft < dmel::kMinFastNfft || n_fft > dmel::kMaxFastNfft || (n_fft & (n_fft - 1)))
        return fail(DMEL_ERR_UNSUPPORTED, w + ": n_fft must be a power of two in [32, 16384]");
    return DMEL_OK;
}

dmel_status dmel_backward_fb_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev, int32_t n_fft,
                                         uint32_t flags, const float* grad_out, const float* out, float* grad_fb, void* stream)
{
    dmel_status st = fb_lengths_args("dmel_backward_fb_dev_lengths", plan, (x && lambd_dev) ? (const void*)x : nullptr, lengths, batch, n_fft, flags, grad_out, out, grad_fb);
    if (st != DMEL_OK) return st;
    if ((st = check_store_aligned("dmel_backward_fb_dev_lengths", {{"grad_fb", grad_fb}})) != DMEL_OK) return st;
    FbGradCall c;
    c.x = x; c.batch = batch; c.lambd_dev = lambd_dev; c.n_fft_dev = n_fft; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb;
    c.lengths = lengths;
    return backward_fb_impl(plan, c, stream);
}

dmel_status dmel_backward_fb_saved_lengths(dmel_plan* plan, const float* spec, const int32_t* lengths, int32_t batch, int32_t n_fft, uint32_t flags,
                                           const float* grad_out, const float* out, const float* tangent, float* grad_fb, float* dlambd,
                                           void* scratch, void* stream)
{
    dmel_status st = fb_lengths_args("dmel_backward_fb_saved_lengths", plan, spec, lengths, batch, n_fft, flags, grad_out, out, grad_fb);
    if (st != DMEL_OK) return st;
    if ((tangent == nullptr) != (dlambd == nullptr))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_fb_saved_lengths: tangent and dlambd are given together (d lambd in the same launch) or both NULL");
    if ((st = check_store_aligned("dmel_backward_fb_saved_lengths", {{"grad_fb", grad_fb}, {"scratch", scratch}})) != DMEL_OK) return st;
    FbGradCall c;
    c.batch = batch; c.n_fft_dev = n_fft; c.flags = flags; c.grad_out = grad_out; c.out = out; c.grad_fb = grad_fb; c.saved_spec = spec;
    c.tangent = tangent; c.dlambd = dlambd; c.scratch = scratch; c.lengths = lengths;
    return backward_fb_impl(plan, c, stream);
}

namespace {
// The rows the x-gradient kernels leave in the workspace at n_fft N (mels = 0: the spectrogram layer).  n_fft 32 ... 2048: the wave-FFT kernel leaves one
// overlap-added segment per tile of frames (and, for short clips with the plain Gaussian window, forms window and clip sum itself: own_prep); else a row per frame
struct XgShape { bool wave, own_prep; int fpt, tiles, span, ts; size_t frame_floats, csum_doubles; };

// false: the segment of a tile does not fit 30 bits (hop_length too large); the sizes are filled in either way
bool xgrad_shape(const dmel_plan* pl, int N, int batch, int mels, int win_half, XgShape* r)
{
    const bool lds = N > dmel::kMaxNfft || (N & (N - 1));             // (dmel_big.hip, both directions: one row per frame too)
    const int win_n = win_half ? N : N / 2 + 1;             // the plain Gaussian is symmetric about N/2 (the whole-clip window need not be)
    r->fpt = 0;
    r->wave = !lds && dmel::xgrad_wave_shape(N, mels, win_n, &r->fpt) && std::getenv("DMEL_XGRAD_LDS") == nullptr;
    r->own_prep = r->wave && !win_half && !pl->cfg.normalize_window && pl->cfg.n_points <= 32768 && std::getenv("DMEL_XGRAD_PREP") == nullptr;
    r->tiles = r->wave ? (pl->T + r->fpt - 1) / r->fpt : 0;
    const long long span = r->wave ? (long long)(r->fpt - 1) * pl->cfg.hop_length + N : 0;
    r->span = (int)span;
    r->ts = r->wave ? r->fpt * pl->cfg.hop_length : 0;
    const size_t rows = r->wave ? (size_t)r->tiles : (size_t)pl->T, row_len = r->wave ? (size_t)span : (size_t)N;
    r->frame_floats = ((size_t)batch * rows * row_len + 63) / 64 * 64;
    r->csum_doubles = (size_t)batch * rows;                 // one fp64 sum per frame / tile
    return span <= 0x3fffffffLL;
}

// gradient w.r.t. the waveform: the mel layer (spec_mode 0; n_over / win_half describe the optimized=False branch) and the spectrogram layer (spec_mode 1:
// grad_out is the gradient of the power spectrogram).  lambd_dev: lambd is read by the kernels; the transform length then comes from the caller (n_over)
struct XgradCall {
    const float* x = nullptr; int batch = 0; uint32_t flags = 0; const float* grad_out = nullptr; const float* out = nullptr; float* grad_x = nullptr;
    float lambd = 0.f; const float* lambd_dev = nullptr; int n_over = 0, win_half = 0, spec_mode = 0; const int32_t* lengths = nullptr;   // the scalar layers
    int channels = 0; const int32_t* edges = nullptr; const char* who = "";          // the K-window layers: validated band edges or nullptr, the entry point's name
    bool lens = false;                                                               // ... and whether it is a *_lengths form (then lengths must not be NULL)
    XgradCall(const float* x_, int batch_, uint32_t flags_, const float* grad_out_, const float* out_, float* grad_x_)      // what every entry point fills alike
        : x(x_), batch(batch_), flags(flags_), grad_out(grad_out_), out(out_), grad_x(grad_x_) {}
    bool log() const { return (flags & DMEL_FLAG_LOG) != 0; }
    bool check_nfft() const { return (flags & DMEL_FLAG_CHECK_NFFT) != 0; }
};

dmel_status backward_x_impl(dmel_plan* plan, const XgradCall& c, void* stream)
{
    const int batch = c.batch, win_half = c.win_half;
    if (c.lambd_dev && c.n_over <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd on the device needs an explicit n_fft");
    { dmel_status sa = check_store_aligned(c.lengths ? "dmel_backward_x_lengths" : "dmel_backward_x", {{"grad_x", c.grad_x}}); if (sa != DMEL_OK) return sa; }
    const int N = c.n_over > 0 ? c.n_over : dmel_n_fft(c.lambd);
    const bool big = N > dmel::kMaxNfft || (N & (N - 1));              // dmel_big.hip: chirp-z / global-memory FFT, both directions
    // per-clip lengths (dmel_xgrad_len.hip): the range of the lengths forward, the mel layer's Gaussian window
    if (c.lengths && (big || N < dmel::kMinFastNfft || c.spec_mode || win_half))
        return fail(DMEL_ERR_UNSUPPORTED, "gradient w.r.t. the waveform with per-clip lengths: n_fft 32 ... 16384 (n_fft = " + std::to_string(N) + ")");
    if (N < 1 || N > dmel::kMaxBigFft || (big && (N & 1)))
        return fail(DMEL_ERR_UNSUPPORTED, "gradient w.r.t. the waveform: n_fft = " + std::to_string(N) + " (even lengths up to " +
                    std::to_string(dmel::kMaxBigFft) + ")");
    { dmel_status sd = check_device(plan); if (sd != DMEL_OK) return sd; }
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    NfftTables* tb = nullptr;
    dmel_status st = build_tables(plan, N, &tb);
    if (st != DMEL_OK) return st;
    if ((st = order_after_last_stream(plan, s)) != DMEL_OK) return st;
    Scratch sc;
    if ((st = ensure_own_scratch(plan, batch, s, &sc)) != DMEL_OK) return st;
    dmel_plan::BigTab bt;
    const float2* big_tw = nullptr;
    if (big && (st = big_tables_for(plan, N, &bt, &big_tw)) != DMEL_OK) return st;
    const int mels = c.spec_mode ? 0 : plan->cfg.n_mels;
    XgShape sh;
    if (!xgrad_shape(plan, N, batch, mels, win_half, &sh)) return fail(DMEL_ERR_UNSUPPORTED, "gradient w.r.t. the waveform: hop_length too large");
    size_t need = sh.frame_floats + 2 * sh.csum_doubles + 16;
    if (c.check_nfft() && !is_capturing(s)) {
        // One call per candidate n_fft of a tracked forward (DMEL_FLAG_CHECK_NFFT): a step captured later may hold a neighbour -- 2 n_fft
        // or n_fft / 2 -- that no eager call has run yet (GraphedStep captures with the launches lambd can reach, not the ones the warm-up
        // happened to issue), and a workspace cannot grow under capture.  Size it here for the neighbours too (a re-capture
        // near an n_fft boundary raised in the middle of training).
        for (int nn : {N / 2, 2 * N}) {
            XgShape s2;
            if (nn < 2 || nn > dmel::kMaxNfft || (nn & (nn - 1))) continue;
            xgrad_shape(plan, nn, batch, mels, win_half, &s2);
            need = std::max(need, s2.frame_floats + 2 * s2.csum_doubles + 16);
        }
    }
    if ((st = grow_floats(&plan->fbw, &plan->fbw_floats, need, s, "")) != DMEL_OK) return st;
    // the big path's window table and (sequences longer than LDS) per-workgroup workspace are plan-owned, like the forward's
    const long long units = (long long)batch * ((plan->T + 1) / 2);
    const int big_grid = big ? dmel::big_grid(units, bt.M) : 0;
    if (big && (st = grow_big_workspace(plan, N, dmel::big_uses_global(bt.M) ? (size_t)big_grid * bt.M : 0, s)) != DMEL_OK) return st;
    // clip sums + window table (the tangent half of the table is not used here)
    dmel::PrepParams pp{};
    pp.x = c.x; pp.psum = sc.psum; pp.win2 = big ? plan->big_win : sc.win;
    pp.B = batch; pp.L = plan->cfg.n_points; pp.nchunks = plan->nchunks; pp.chunk = plan->chunk;
    pp.N = N; pp.normalize = plan->cfg.normalize_window; pp.win_half = win_half;
    pp.center = window_center(N, win_half);
    pp.lam.dev = c.lambd_dev; pp.lam.val = c.lambd_dev ? 0.f : c.lambd; pp.lam.role = dmel::kLamQuiet;
    pp.lengths = c.lengths;                                 // the partial sums then stop at the clip's end, as in the forward
    if (!sh.own_prep) DMEL_HIP(dmel::launch_prep(pp, s));
    dmel::XgradParams xp{};
    xp.own_prep = sh.own_prep ? 1 : 0; xp.win_denom = std::fabs(c.lambd) + 1e-15f; xp.lam_dev = c.lambd_dev;
    xp.check_nfft = (c.check_nfft() && c.lambd_dev && !big) ? 1 : 0;
    xp.x = c.x; xp.psum = sc.psum; xp.win2 = big ? plan->big_win : sc.win; xp.tw = big ? big_tw : tb->tw_long;
    xp.chirp = big ? bt.chirp : nullptr; xp.hbr = big ? bt.hbr : nullptr; xp.zws = plan->big_z; xp.Mfft = big ? bt.M : 0; xp.logM = big ? bt.logM : 0;
    xp.fb = tb->fb_dense; xp.rowband = tb->rowband; xp.rowpk = tb->rowpk; xp.long_rows = tb->long_rows ? 1 : 0; xp.grad_out = c.grad_out; xp.out = c.log() ? c.out : nullptr;
    xp.frames = plan->fbw; xp.grad_x = c.grad_x;
    xp.csum = reinterpret_cast<double*>(plan->fbw + sh.frame_floats);      // 256-byte aligned: frame_floats is a multiple of 64
    xp.B = batch; xp.L = plan->cfg.n_points; xp.T = plan->T; xp.hop = plan->cfg.hop_length; xp.M = plan->cfg.n_mels;
    xp.nchunks = plan->nchunks; xp.N = N; xp.F = tb->F; xp.remove_dc = 1; xp.spec_mode = c.spec_mode;
    xp.logN = 0; while ((1 << xp.logN) < N) ++xp.logN;
    xp.inv_L = 1.0f / (float)plan->cfg.n_points;
    xp.tw1 = tb->tw1p; xp.tw2 = tb->tw2p;
    xp.win_n = win_half ? N : N / 2 + 1; xp.tiles = sh.tiles; xp.span = sh.span; xp.tile_step = sh.ts;
    const size_t m0 = prof_mark(plan, s);
    if (big) {
        DMEL_HIP(dmel::launch_xgrad_big(xp, big_grid, s));
        DMEL_HIP(dmel::launch_xgrad_gather(xp, s));
    } else if (c.lengths) {
        dmel::XgradLenParams lp{};
        static_cast<dmel::XgradParams&>(lp) = xp;
        lp.lengths = c.lengths; lp.fpt = sh.wave ? sh.fpt : 0;
        DMEL_HIP(dmel::launch_xgrad_len(lp, s));
    } else {
        DMEL_HIP(dmel::launch_xgrad(xp, s));
    }
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}

// dmel_backward_x, _dev, _lengths, _dev_lengths: the same checks in the same order under four names.  dev: lambd on the device, c.n_over the n_fft
// this step's forward was issued for; lens: the per-clip-lengths forms (their flags are checked: they have no DMEL_FLAG_FULL_WINDOW)
dmel_status backward_x_mel(const char* who, dmel_plan* plan, XgradCall c, bool dev, bool lens, void* stream)
{
    const std::string w = who;
    const int n_fft = c.n_over;
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (dev && !c.lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    if (c.batch < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch < 0");
    if (c.batch == 0) return DMEL_OK;
    if (!c.x || (lens && !c.lengths) || !c.grad_out || !c.grad_x)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + (lens ? ": x / lengths / grad_out / grad_x is NULL" : ": x / grad_out / grad_x is NULL"));
    if (lens && (c.flags & ~(DMEL_FLAG_LOG | (dev ? DMEL_FLAG_CHECK_NFFT : 0u))))
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + (dev ? ": flags other than LOG, CHECK_NFFT" : ": flags other than LOG"));
    if (c.log() && !c.out) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": DMEL_FLAG_LOG needs the saved log output");
    if (!dev && !std::isfinite(c.lambd)) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
    const bool full = !lens && (c.flags & DMEL_FLAG_FULL_WINDOW) != 0;               // optimized=False: n_fft = 2 L, window = the clip
    if (dev && lens && (n_fft < 1 || (n_fft & (n_fft - 1))))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be a power of two (the n_fft this step's forward was issued for)");
    if (dev && !lens && !full && (n_fft < 1 || n_fft > dmel::kMaxNfft || (n_fft & (n_fft - 1))))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "n_fft must be a power of two in [1, 16384] (the n_fft this step's forward was issued for)");
    if (dev && full && c.check_nfft())
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": DMEL_FLAG_CHECK_NFFT has no meaning with DMEL_FLAG_FULL_WINDOW (n_fft = 2 n_points)");
    if (!dev) c.flags &= DMEL_FLAG_LOG;                                             // (DMEL_FLAG_CHECK_NFFT belongs to the device forms)
    c.n_over = full ? 2 * plan->cfg.n_points : (dev ? n_fft : 0); c.win_half = full ? 1 : 0;
    return backward_x_impl(plan, c, stream);
}
}  // namespace

dmel_status dmel_backward_x(dmel_plan* plan, const float* x, int32_t batch, float lambd, uint32_t flags,
                            const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.lambd = lambd;
    return backward_x_mel("dmel_backward_x", plan, c, false, false, stream);
}

dmel_status dmel_backward_x_spec(dmel_plan* plan, const float* x, int32_t batch, float lambd, int32_t n_fft, uint32_t flags,
                                 const float* grad_spec, float* grad_x, void* stream)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (batch < 0 || n_fft < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch / n_fft < 0");
    if (batch == 0) return DMEL_OK;
    if (!x || !grad_spec || !grad_x) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_x_spec: x / grad_spec / grad_x is NULL");
    if (!(flags & DMEL_SPEC_REMOVE_DC)) return fail(DMEL_ERR_UNSUPPORTED, "dmel_backward_x_spec: only the DC-removed spectrogram (models.py:187) is differentiated");
    if (!std::isfinite(lambd)) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd is not finite");
    XgradCall c(x, batch, 0u, grad_spec, nullptr, grad_x);
    c.lambd = lambd; c.n_over = n_fft; c.win_half = (flags & DMEL_SPEC_HALF_WINDOW) ? 1 : 0; c.spec_mode = 1;
    return backward_x_impl(plan, c, stream);
}

dmel_status dmel_backward_x_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.lambd_dev = lambd_dev; c.n_over = n_fft;
    return backward_x_mel("dmel_backward_x_dev", plan, c, true, false, stream);
}

dmel_status dmel_backward_x_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, float lambd, uint32_t flags,
                                    const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.lambd = lambd; c.lengths = lengths;
    return backward_x_mel("dmel_backward_x_lengths", plan, c, false, true, stream);
}

dmel_status dmel_backward_x_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                        int32_t n_fft, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.lambd_dev = lambd_dev; c.n_over = n_fft; c.lengths = lengths;
    return backward_x_mel("dmel_backward_x_dev_lengths", plan, c, true, true, stream);
}

dmel_status dmel_backward_x_spec_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t n_fft, uint32_t flags,
                                     const float* grad_spec, float* grad_x, void* stream)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, "lambd_dev is NULL");
    if (batch < 0 || n_fft <= 0) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch < 0 or n_fft not given");
    if (batch == 0) return DMEL_OK;
    if (!x || !grad_spec || !grad_x) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_backward_x_spec_dev: x / grad_spec / grad_x is NULL");
    if (!(flags & DMEL_SPEC_REMOVE_DC)) return fail(DMEL_ERR_UNSUPPORTED, "dmel_backward_x_spec_dev: only the DC-removed spectrogram (models.py:187) is differentiated");
    XgradCall c(x, batch, 0u, grad_spec, nullptr, grad_x);
    c.lambd_dev = lambd_dev; c.n_over = n_fft; c.win_half = (flags & DMEL_SPEC_HALF_WINDOW) ? 1 : 0; c.spec_mode = 1;
    return backward_x_impl(plan, c, stream);
}

namespace {
// The K-window layers' gradient w.r.t. the waveform: c.edges == nullptr: grad_out / out are (B, K, M, T); else ONE (B, 1, M, T) image -- channel c's mel
// gradient is its rows [edges[c], edges[c + 1]) and +0.0 elsewhere.  At n_fft N every channel takes the path backward_x_impl takes for the scalar layer
dmel_status check_x_multi_args(dmel_plan* pl, const XgradCall& c)
{
    const std::string who = c.who;
    if (!pl) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    if (c.batch < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": batch < 0");
    if (c.channels < 1 || c.channels > dmel::kMaxChannels) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": channels must be 1 ... 8");
    if (c.flags & ~(uint32_t)DMEL_FLAG_LOG) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": only DMEL_FLAG_LOG is accepted");
    if (c.batch > 0 && (!c.x || !c.grad_out || !c.grad_x)) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": x / grad_out / grad_x is NULL");
    if (c.batch > 0 && c.lens && !c.lengths) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": lengths is NULL");
    if (c.batch > 0 && (c.flags & DMEL_FLAG_LOG) && !c.out) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": DMEL_FLAG_LOG needs the saved log output");
    if ((long long)c.batch * c.channels > 65534) return fail(DMEL_ERR_INVALID_ARGUMENT, "batch x channels > 65534 (split the call)");
    return DMEL_OK;
}

// ll: the launch list (checked by the caller); lam_host (K values) or lam_dev (K device words) -- exactly one of them
dmel_status backward_x_multi_impl(dmel_plan* plan, const XgradCall& xc, const float* lam_host, const float* lam_dev, const LaunchList& ll, void* stream)
{
    const int batch = xc.batch, channels = xc.channels, nl = ll.nl;
    const int* ns = ll.ns; const uint32_t* mask = ll.mask;
    const int32_t* edges = xc.edges;
    const int32_t* lengths = xc.lengths;                          // per-clip lengths (dmel_xgrad_klen.hip) or nullptr
    const std::string who = lengths ? xc.who : edges ? "dmel_backward_x_band" : "dmel_backward_x_multi";
    { dmel_status sa = check_store_aligned(who.c_str(), {{"grad_x", xc.grad_x}}); if (sa != DMEL_OK) return sa; }
    { dmel_status sd = check_device(plan); if (sd != DMEL_OK) return sd; }
    std::lock_guard<std::mutex> lock(plan->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool capturing = is_capturing(s);
    // each channel's candidates (its launches, ascending) and their shapes
    int ncand[dmel::kMaxChannels] = {}, cand[dmel::kMaxChannels][dmel::kXgMaxCand] = {};
    for (int i = 0; i < nl; ++i)
        for (int c = 0; c < channels; ++c)
            if (mask[i] >> c & 1u) cand[c][ncand[c]++] = ns[i];
    std::map<int, XgShape> shape;
    dmel_status st = DMEL_OK;
    for (int i = 0; i < nl; ++i)
        for (int n : {ns[i], ns[i] / 2, 2 * ns[i]}) {
            if (!multi_in_range(n) || shape.count(n) || (capturing && n != ns[i])) continue;      // eager: the neighbours too (see below)
            XgShape sh;
            if (!xgrad_shape(plan, n, batch, plan->cfg.n_mels, 0, &sh)) return fail(DMEL_ERR_UNSUPPORTED, "gradient w.r.t. the waveform: hop_length too large");
            shape[n] = sh;
        }
    NfftTables* tb[3 * dmel::kMaxChannels] = {};
    for (int i = 0; i < nl; ++i) if ((st = build_tables(plan, ns[i], &tb[i])) != DMEL_OK) return st;
    if ((st = order_after_last_stream(plan, s)) != DMEL_OK) return st;
    Scratch sc;
    if ((st = ensure_own_scratch(plan, batch, s, &sc)) != DMEL_OK) return st;
    // workspace: per channel a region of the largest shape it may take -- eagerly also at n_fft / 2 and 2 n_fft of every launch, so that a
    // capture after the lambd of a channel crossed a boundary needs no growth -- then the window tables (channel x candidate) of the
    // launches that do not evaluate their own window, then grad_out / out of one channel staged as (B, M, T) for the LDS frames kernel
    size_t fr_stride = 0, cs_floats = 0;
    bool any_prep = false, any_lds = false;
    for (const auto& kv : shape) {
        fr_stride = std::max(fr_stride, kv.second.frame_floats);
        cs_floats = std::max(cs_floats, (2 * kv.second.csum_doubles + 63) / 64 * 64);
        any_prep |= !kv.second.own_prep;
        any_lds |= !kv.second.wave;
    }
    const size_t region = fr_stride + cs_floats;
    const size_t bmt = (size_t)batch * plan->cfg.n_mels * plan->T;
    const size_t win_floats = any_prep ? (size_t)channels * dmel::kXgMaxCand * dmel::kMaxNfft * 2 : 0;
    const size_t stage_floats = any_lds ? (2 * bmt + 63) / 64 * 64 : 0;
    const size_t need = (size_t)channels * region + win_floats + stage_floats + 16;
    if ((st = grow_floats(&plan->xmw, &plan->xmw_floats, need, s, who + ": the ")) != DMEL_OK) return st;
    float* frames[dmel::kMaxChannels] = {};
    double* csum[dmel::kMaxChannels] = {};
    for (int c = 0; c < channels; ++c) {
        frames[c] = plan->xmw + (size_t)c * region;
        csum[c] = reinterpret_cast<double*>(frames[c] + fr_stride);           // 256-byte aligned: region and fr_stride are multiples of 64
    }
    float2* wins = any_prep ? reinterpret_cast<float2*>(plan->xmw + (size_t)channels * region) : nullptr;
    float* stage = any_lds ? plan->xmw + (size_t)channels * region + win_floats : nullptr;
    auto table = [&](int c, int n) -> float2* {
        for (int j = 0; j < ncand[c]; ++j) if (cand[c][j] == n) return wins ? wins + (size_t)(c * dmel::kXgMaxCand + j) * dmel::kMaxNfft : nullptr;
        return nullptr;
    };
    const int L = plan->cfg.n_points, M = plan->cfg.n_mels, T = plan->T;
    const size_t m0 = prof_mark(plan, s);
    for (int i = 0; i < nl; ++i) {
        const int N = ns[i];
        const XgShape& sh = shape[N];
        // window tables (and the partial clip sums) where the kernel does not evaluate its own: one dmel_prep_kernel per channel
        if (!sh.own_prep)
            for (int c = 0; c < channels; ++c) {
                if (!(mask[i] >> c & 1u)) continue;
                dmel::PrepParams pp{};
                pp.x = xc.x; pp.psum = sc.psum; pp.win2 = table(c, N);
                pp.B = batch; pp.L = L; pp.nchunks = plan->nchunks; pp.chunk = plan->chunk;
                pp.N = N; pp.normalize = plan->cfg.normalize_window; pp.win_half = 0; pp.center = (float)N / 2.0f;
                pp.lam.dev = lam_dev ? lam_dev + c : nullptr; pp.lam.val = lam_dev ? 0.f : lam_host[c]; pp.lam.role = dmel::kLamQuiet;
                pp.lengths = lengths;                               // the partial sums then stop at the clip's end, as backward_x_impl
                DMEL_HIP(dmel::launch_prep(pp, s));
            }
        dmel::XgradParams xp{};
        xp.own_prep = sh.own_prep ? 1 : 0; xp.lam_dev = lam_dev; xp.check_nfft = lam_dev ? 1 : 0;
        xp.x = xc.x; xp.psum = sc.psum; xp.tw = tb[i]->tw_long;
        xp.fb = tb[i]->fb_dense; xp.rowband = tb[i]->rowband; xp.rowpk = tb[i]->rowpk; xp.long_rows = tb[i]->long_rows ? 1 : 0;
        xp.grad_out = xc.grad_out; xp.out = xc.log() ? xc.out : nullptr; xp.grad_x = xc.grad_x;
        xp.B = batch; xp.L = L; xp.T = T; xp.hop = plan->cfg.hop_length; xp.M = M;
        xp.nchunks = plan->nchunks; xp.N = N; xp.F = tb[i]->F; xp.remove_dc = 1; xp.spec_mode = 0;
        xp.logN = 0; while ((1 << xp.logN) < N) ++xp.logN;
        xp.inv_L = 1.0f / (float)L;
        xp.tw1 = tb[i]->tw1p; xp.tw2 = tb[i]->tw2p;
        xp.win_n = N / 2 + 1; xp.tiles = sh.tiles; xp.span = sh.span; xp.tile_step = sh.ts;
        if (sh.wave) {
            // one launch for every channel of this n_fft
            dmel::XgradBandLenParams mp{};                                    // (every launcher takes the part of it that is its own)
            mp.p = xp; mp.lengths = lengths; mp.fpt = sh.fpt;
            for (int c = 0; c < channels; ++c) {
                mp.win2[c] = table(c, N); mp.frames[c] = frames[c]; mp.csum[c] = csum[c];
                mp.win_denom[c] = lam_host ? std::fabs(lam_host[c]) + 1e-15f : 0.f;
                if (mask[i] >> c & 1u) { mp.ch_list |= (unsigned)c << (4 * mp.count); ++mp.count; }
            }
            mp.ch_grid = batch * sh.tiles; mp.ch_out = edges ? 1 : channels;
            for (int c = 0; edges && c <= dmel::kMaxChannels; ++c) mp.band_edges[c] = edges[std::min(c, channels)];
            if ((long long)batch * sh.tiles * mp.count > 0x7fffffffLL) return fail(DMEL_ERR_UNSUPPORTED, "gradient w.r.t. the waveform: grid too large");
            if (lengths) {
                dmel::XgradMultiLenParams ml{};                               // (no base of mp: there the lengths lie behind the edges)
                static_cast<dmel::XgradMultiParams&>(ml) = mp; ml.lengths = lengths; ml.fpt = sh.fpt;
                DMEL_HIP(edges ? dmel::launch_xgrad_wave_band_len(mp, s) : dmel::launch_xgrad_wave_multi_len(ml, s));
            } else {
                DMEL_HIP(edges ? dmel::launch_xgrad_wave_band(mp, s) : dmel::launch_xgrad_wave_multi(mp, s));
            }
        } else {
            // the LDS path (cold): per channel, its rows of grad_out / out staged as (B, M, T) -- strided copy or the band layer's masking kernel -- then the frames kernel
            for (int c = 0; c < channels; ++c) {
                if (!(mask[i] >> c & 1u)) continue;
                const size_t row = (size_t)M * T * sizeof(float);
                if (edges) {
                    dmel::XgradBandStageParams sp{};
                    sp.grad_out = xc.grad_out; sp.out = xc.log() ? xc.out : nullptr; sp.stage_grad = stage; sp.stage_out = stage + bmt;
                    sp.M = M; sp.T = T; sp.e_lo = edges[c]; sp.e_hi = edges[c + 1]; sp.n = (long long)bmt;
                    DMEL_HIP(dmel::launch_xgrad_band_stage(sp, s));
                } else {
                    DMEL_HIP(hipMemcpy2DAsync(stage, row, xc.grad_out + (size_t)c * M * T, row * channels, row, batch, hipMemcpyDeviceToDevice, s));
                    if (xc.log()) DMEL_HIP(hipMemcpy2DAsync(stage + bmt, row, xc.out + (size_t)c * M * T, row * channels, row, batch, hipMemcpyDeviceToDevice, s));
                }
                dmel::XgradParams q = xp;
                q.grad_out = stage; q.out = xc.log() ? stage + bmt : nullptr;
                q.win2 = table(c, N); q.frames = frames[c]; q.csum = csum[c];
                q.lam_dev = lam_dev ? lam_dev + c : nullptr;
                if (lengths) {
                    dmel::XgradLenParams lq{};
                    static_cast<dmel::XgradParams&>(lq) = q; lq.lengths = lengths; lq.fpt = 0;
                    DMEL_HIP(dmel::launch_xgrad_frames_len(lq, s));
                } else {
                    DMEL_HIP(dmel::launch_xgrad_frames(q, s));
                }
            }
        }
    }
    // one combine: the channels' terms in ascending channel order
    dmel::XgradCombineMultiLenParams cp{};                        // (without lengths: its XgradCombineMultiParams part)
    cp.lengths = lengths;
    cp.grad_x = xc.grad_x; cp.lam_dev = lam_dev; cp.L = L; cp.T = T; cp.hop = plan->cfg.hop_length; cp.channels = channels;
    for (int c = 0; c < channels; ++c) {
        cp.ncand[c] = ncand[c]; cp.frames[c] = frames[c]; cp.csum[c] = csum[c];
        for (int j = 0; j < ncand[c]; ++j) {
            const XgShape& sh = shape[cand[c][j]];
            cp.n[c][j] = cand[c][j]; cp.tiles[c][j] = sh.tiles; cp.span[c][j] = sh.span; cp.tile_step[c][j] = sh.ts;
            cp.fpt[c][j] = sh.wave ? sh.fpt : 0;
        }
    }
    DMEL_HIP(lengths ? dmel::launch_xgrad_combine_multi_len(cp, batch, s) : dmel::launch_xgrad_combine_multi(cp, batch, s));
    prof_span(plan, m0, prof_mark(plan, s), 2);
    return DMEL_OK;
}

// dmel_backward_x_multi / dmel_backward_x_band (c.edges: validated, or nullptr)
dmel_status backward_x_multi_host(dmel_plan* plan, const XgradCall& c, const float* lambd_host, void* stream)
{
    dmel_status st = check_x_multi_args(plan, c);
    if (st != DMEL_OK) return st;
    if (!lambd_host) return fail(DMEL_ERR_INVALID_ARGUMENT, std::string(c.who) + ": lambd_host is NULL");
    if ((st = check_lambd_multi(lambd_host, c.channels)) != DMEL_OK) return st;
    if (c.batch == 0) return DMEL_OK;
    return backward_x_multi_impl(plan, c, lambd_host, nullptr, group_host_values(lambd_host, c.channels), stream);
}

// dmel_backward_x_multi_dev / dmel_backward_x_band_dev (c.edges: validated, or nullptr)
dmel_status backward_x_multi_devlist(dmel_plan* plan, const XgradCall& c, const float* lambd_dev, const int32_t* n_ffts,
                                     const uint32_t* channel_masks, int32_t count, void* stream)
{
    const std::string who = c.who;
    const int channels = c.channels;
    dmel_status st = check_x_multi_args(plan, c);
    if (st != DMEL_OK) return st;
    if (!lambd_dev) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": lambd_dev is NULL");
    if (!n_ffts || !channel_masks || count < 1 || count > 3 * dmel::kMaxChannels)
        return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": the launch list (n_ffts, channel_masks, count) is missing or empty");
    uint32_t seen = 0;
    int per[dmel::kMaxChannels] = {};
    LaunchList ll;
    for (int i = 0; i < count; ++i) {
        const int n = n_ffts[i];
        if (!multi_in_range(n) || (n & (n - 1)))
            return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": n_ffts[" + std::to_string(i) + "] = " + std::to_string(n) +
                        " is not a power of two in 32 ... 16384");
        if (i > 0 && n <= n_ffts[i - 1]) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": n_ffts must be strictly ascending");
        if (channel_masks[i] == 0 || (channels < 32 && (channel_masks[i] >> channels) != 0))
            return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": channel_masks[" + std::to_string(i) + "] is empty or names a channel >= channels");
        seen |= channel_masks[i];
        for (int ch = 0; ch < channels; ++ch)
            if ((channel_masks[i] >> ch & 1u) && ++per[ch] > dmel::kXgMaxCand)
                return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": channel " + std::to_string(ch) + " is in more than 3 launches");
        ll.ns[i] = n; ll.mask[i] = channel_masks[i]; ll.nl = i + 1;
    }
    if (seen != (1u << channels) - 1u) return fail(DMEL_ERR_INVALID_ARGUMENT, who + ": a channel is in no launch");
    if (c.batch == 0) return DMEL_OK;
    return backward_x_multi_impl(plan, c, nullptr, lambd_dev, ll, stream);
}

}  // namespace

dmel_status dmel_backward_x_multi(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels,
                                  uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_multi";
    return backward_x_multi_host(plan, c, lambd_host, stream);
}

dmel_status dmel_backward_x_multi_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels,
                                      const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count, uint32_t flags,
                                      const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_multi_dev";
    return backward_x_multi_devlist(plan, c, lambd_dev, n_ffts, channel_masks, count, stream);
}

// the band-split layer's gradient w.r.t. the waveform: dmel_backward_x_multi(_dev) over ONE (B, 1, M, T) cotangent (and saved log output),
// channel c taking its rows [band_edges[c], band_edges[c + 1]) of it.  Pass the launch list of the dmel_forward_band_dev whose gradient this is.
dmel_status dmel_backward_x_band(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_host, int32_t channels,
                                 const int32_t* band_edges, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    BandEdges be;
    const dmel_status st = take_band_edges(plan, band_edges, channels, "dmel_backward_x_band", &be);
    if (st != DMEL_OK) return st;
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_band";
    c.edges = be.e;
    return backward_x_multi_host(plan, c, lambd_host, stream);
}

dmel_status dmel_backward_x_band_dev(dmel_plan* plan, const float* x, int32_t batch, const float* lambd_dev, int32_t channels,
                                     const int32_t* band_edges, const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count,
                                     uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    BandEdges be;
    const dmel_status st = take_band_edges(plan, band_edges, channels, "dmel_backward_x_band_dev", &be);
    if (st != DMEL_OK) return st;
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_band_dev";
    c.edges = be.e;
    return backward_x_multi_devlist(plan, c, lambd_dev, n_ffts, channel_masks, count, stream);
}

namespace {
// the *_lengths band forms: the edges' own shape, then every argument check that needs no plan's contents, then the edges against the plan's n_mels
dmel_status take_band_edges_x(dmel_plan* plan, const XgradCall& c, const int32_t* band_edges, BandEdges* be)
{
    dmel_status st = band_edges_shape(band_edges, c.channels, c.who);
    if (st == DMEL_OK) st = check_x_multi_args(plan, c);
    return st != DMEL_OK ? st : take_band_edges(plan, band_edges, c.channels, c.who, be);
}
}  // namespace

// the four forms above over clips of per-clip lengths (dmel_xgrad_klen.hip): clip b is x[b, :lengths[b]], read by the kernels when they run
dmel_status dmel_backward_x_multi_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                          int32_t channels, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_multi_lengths"; c.lengths = lengths; c.lens = true;
    return backward_x_multi_host(plan, c, lambd_host, stream);
}

dmel_status dmel_backward_x_multi_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                              int32_t channels, const int32_t* n_ffts, const uint32_t* channel_masks, int32_t count,
                                              uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_multi_dev_lengths"; c.lengths = lengths; c.lens = true;
    return backward_x_multi_devlist(plan, c, lambd_dev, n_ffts, channel_masks, count, stream);
}

dmel_status dmel_backward_x_band_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_host,
                                         int32_t channels, const int32_t* band_edges, uint32_t flags, const float* grad_out, const float* out,
                                         float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_band_lengths"; c.lengths = lengths; c.lens = true;
    BandEdges be;
    const dmel_status st = take_band_edges_x(plan, c, band_edges, &be);
    if (st != DMEL_OK) return st;
    c.edges = be.e;
    return backward_x_multi_host(plan, c, lambd_host, stream);
}

dmel_status dmel_backward_x_band_dev_lengths(dmel_plan* plan, const float* x, const int32_t* lengths, int32_t batch, const float* lambd_dev,
                                             int32_t channels, const int32_t* band_edges, const int32_t* n_ffts, const uint32_t* channel_masks,
                                             int32_t count, uint32_t flags, const float* grad_out, const float* out, float* grad_x, void* stream)
{
    XgradCall c(x, batch, flags, grad_out, out, grad_x);
    c.channels = channels; c.who = "dmel_backward_x_band_dev_lengths"; c.lengths = lengths; c.lens = true;
    BandEdges be;
    const dmel_status st = take_band_edges_x(plan, c, band_edges, &be);
    if (st != DMEL_OK) return st;
    c.edges = be.e;
    return backward_x_multi_devlist(plan, c, lambd_dev, n_ffts, channel_masks, count, stream);
}

dmel_status dmel_plan_last_multi_launch(dmel_plan* plan, int32_t* n_ffts, uint32_t* channel_masks, int32_t* count)
{
    if (!plan || !n_ffts || !channel_masks || !count) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_plan_last_multi_launch: bad arguments");
    std::lock_guard<std::mutex> lock(plan->mu);
    for (int i = 0; i < plan->last_multi_nl; ++i) { n_ffts[i] = plan->last_multi_ns[i]; channel_masks[i] = plan->last_multi_mask[i]; }
    *count = plan->last_multi_nl;
    return DMEL_OK;
}

dmel_status dmel_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* step, uint32_t* ticket, int64_t n,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int32_t maximize, void* stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_adam_step: NULL pointer");
    if (n < 0 || n > (1LL << 31)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_adam_step: n out of range");
    // the same ranges torch.optim.Adam and dmel_amd.LambdAdam accept
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(lr) || !(lr >= 0.0) ||
        !std::isfinite(weight_decay) || !(weight_decay >= 0.0))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_adam_step: lr / betas / eps / weight_decay out of range");
    if (n == 0) return DMEL_OK;
    if (!ticket && dmel::adam_grid(n) > 1) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_adam_step: more than 1024 elements need the ticket word");
    dmel::AdamParams ap{};
    ap.param = param; ap.grad = grad; ap.exp_avg = exp_avg; ap.exp_avg_sq = exp_avg_sq; ap.step = step; ap.ticket = ticket;
    ap.n = n; ap.maximize = maximize ? 1 : 0;
    ap.lr = lr; ap.beta1 = beta1; ap.beta2 = beta2; ap.eps = eps; ap.weight_decay = weight_decay;
    DMEL_HIP(dmel::launch_adam(ap, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

namespace {
// the stages behind the mel layers (PCEN, BandNorm, SpecMask, Deltas, StatsPool, AttentivePool): what their entry points check alike

// p is not a multiple of `bytes` (a power of two); false for NULL
bool misaligned(const void* p, int bytes)
{
    return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) != 0;
}

// a stage launches on the calling thread's current device: there must be one
dmel_status hip_device(const char* who)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return fail(DMEL_ERR_NO_DEVICE, std::string(who) + ": no HIP device"); }
    return DMEL_OK;
}

// rows of T frames, rows_per_clip of them per clip (Deltas, StatsPool, AttentivePool: one text)
dmel_status stage_rows_check(const std::string& w, int64_t rows, int64_t rows_per_clip, int32_t T)
{
    if (rows < 0 || T < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows / n_time out of range");
    if (rows_per_clip < 1 || rows % rows_per_clip != 0)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows_per_clip must be positive and divide rows (clip = row / rows_per_clip)");
    return DMEL_OK;
}

// (after the stage's own arguments, where each entry point has always looked at it)
dmel_status stage_lengths_check(const std::string& w, const int32_t* lengths)
{
    if (misaligned(lengths, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": frame_lengths must be int32 values");
    return DMEL_OK;
}

// what dmel_pcen_forward and dmel_pcen_backward check alike; DMEL_OK with *noop set: nothing to launch
dmel_status pcen_check(const char* who, int64_t rows, int32_t n_mels, int32_t T, const float* alpha, const float* delta, const float* r,
                       const float* s, float eps, bool* noop)
{
    const std::string w(who);
    *noop = false;
    if (!alpha || !delta || !r || !s) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": NULL parameter pointer");
    if (n_mels < 1 || rows < 0 || T < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows / n_mels / T out of range");
    if (rows % n_mels != 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows must be a multiple of n_mels (band = row % n_mels)");
    if (!std::isfinite(eps) || !(eps > 0.f)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": eps must be finite and > 0");
    if (rows == 0 || T == 0) { *noop = true; return DMEL_OK; }
    if (dmel::stage_row_blocks(rows, T) > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    return DMEL_OK;
}
}  // namespace

size_t dmel_pcen_scratch_bytes(int64_t rows)
{
    return rows > 0 ? (size_t)rows * 4 * sizeof(float) : 0;
}

dmel_status dmel_pcen_forward(const float* E, int64_t rows, int32_t n_mels, int32_t T, const float* alpha, const float* delta,
                              const float* r, const float* s, float eps, float* y, float* M_or_null, void* stream)
{
    bool noop = false;
    const dmel_status st = pcen_check("dmel_pcen_forward", rows, n_mels, T, alpha, delta, r, s, eps, &noop);
    if (st != DMEL_OK) return st;
    if (!E || !y) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_pcen_forward: NULL pointer (E / y)");
    if (noop) return DMEL_OK;
    const dmel_status sd = hip_device("dmel_pcen_forward");
    if (sd != DMEL_OK) return sd;
    dmel::PcenParams p{};
    p.E = E; p.y = y; p.M = M_or_null; p.alpha = alpha; p.delta = delta; p.r = r; p.s = s;
    p.rows = rows; p.n_mels = n_mels; p.T = T; p.eps = eps;
    DMEL_HIP(dmel::launch_pcen_fwd(p, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_pcen_backward(const float* g, const float* E, const float* M, int64_t rows, int32_t n_mels, int32_t T,
                               const float* alpha, const float* delta, const float* r, const float* s, float eps,
                               float* dE_or_null, float* dparams_or_null, float* scratch, void* stream)
{
    bool noop = false;
    const dmel_status st = pcen_check("dmel_pcen_backward", rows, n_mels, T, alpha, delta, r, s, eps, &noop);
    if (st != DMEL_OK) return st;
    if (!g || !E || !M) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_pcen_backward: NULL pointer (g / E / M)");
    if (dparams_or_null && (!scratch || misaligned(scratch, 16)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_pcen_backward: the parameter gradients need 16-byte aligned scratch of dmel_pcen_scratch_bytes(rows)");
    if (noop || (!dE_or_null && !dparams_or_null)) return DMEL_OK;      // nothing is written (not dparams either)
    const dmel_status sd = hip_device("dmel_pcen_backward");
    if (sd != DMEL_OK) return sd;
    dmel::PcenParams p{};
    p.g = g; p.E = E; p.Min = M; p.dE = dE_or_null; p.partials = dparams_or_null ? scratch : nullptr;
    p.alpha = alpha; p.delta = delta; p.r = r; p.s = s;
    p.rows = rows; p.n_mels = n_mels; p.T = T; p.eps = eps;
    DMEL_HIP(dmel::launch_pcen_bwd(p, dparams_or_null, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

namespace {
// what dmel_bandnorm_forward and dmel_bandnorm_backward check alike; DMEL_OK with *noop set: nothing to launch
dmel_status bandnorm_check(const char* who, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T, int32_t batch_stats, int32_t training,
                           const void* stats, bool* noop)
{
    const std::string w(who);
    *noop = false;
    if (n_mels < 1 || rows < 0 || T < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows / n_mels / T out of range");
    if (rows_per_clip < 1 || rows_per_clip % n_mels != 0)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows_per_clip must be a positive multiple of n_mels (band = row % n_mels)");
    if (rows % rows_per_clip != 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows must be a multiple of rows_per_clip (clip = row / rows_per_clip)");
    if ((batch_stats != 0 && batch_stats != 1) || (training != 0 && training != 1))
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": batch_stats and training are 0 or 1");
    if (!stats || misaligned(stats, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stats must be a 16-byte aligned buffer");
    if (rows == 0 || T == 0) { *noop = true; return DMEL_OK; }
    if (dmel::stage_row_blocks(rows, T) > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    return DMEL_OK;
}
}  // namespace

size_t dmel_bandnorm_scratch_bytes(int64_t rows, int32_t n_mels)
{
    return (rows > 0 ? (size_t)rows * 2 * sizeof(double) : 0) + (n_mels > 0 ? (size_t)n_mels * 2 * sizeof(double) : 0);
}

dmel_status dmel_bandnorm_forward(const float* s, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T, const int32_t* frame_lengths_or_null,
                                  const float* weight_or_null, const float* bias_or_null, int32_t batch_stats, int32_t training, double eps,
                                  double momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked_or_null, float* y,
                                  double* stats, void* scratch, void* stream)
{
    bool noop = false;
    const dmel_status st = bandnorm_check("dmel_bandnorm_forward", rows, n_mels, rows_per_clip, T, batch_stats, training, stats, &noop);
    if (st != DMEL_OK) return st;
    if (!s || !y) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: NULL pointer (s / y)");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: eps must be finite and > 0");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: momentum must lie in 0 ... 1");
    if (batch_stats && !training && (!running_mean || !running_var))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: eval mode of the batch statistics reads running_mean and running_var");
    if (!batch_stats && (running_mean || running_var || num_batches_tracked_or_null))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: clip statistics keep no running_mean / running_var / num_batches_tracked");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: running_mean and running_var come together");
    if (batch_stats && training && (!scratch || misaligned(scratch, 16)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_forward: the batch statistics need 16-byte aligned scratch of dmel_bandnorm_scratch_bytes(rows, n_mels)");
    if (noop) return DMEL_OK;
    const dmel_status sd = hip_device("dmel_bandnorm_forward");
    if (sd != DMEL_OK) return sd;
    dmel::BandNormParams p{};
    p.s = s; p.y = y; p.lengths = frame_lengths_or_null; p.gamma = weight_or_null; p.beta = bias_or_null;
    p.stats = stats; p.partials = static_cast<double*>(scratch);
    p.running_mean = running_mean; p.running_var = running_var; p.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked_or_null);
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.n_mels = n_mels; p.T = T;
    p.batch_stats = batch_stats; p.eval = (batch_stats && !training) ? 1 : 0; p.eps = eps; p.momentum = momentum;
    DMEL_HIP(dmel::launch_bandnorm_fwd(p, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_bandnorm_backward(const float* g, const float* s, const double* stats, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T,
                                   const int32_t* frame_lengths_or_null, const float* weight_or_null, int32_t batch_stats, int32_t training,
                                   float* ds_or_null, float* dweight_or_null, float* dbias_or_null, void* scratch, void* stream)
{
    bool noop = false;
    const dmel_status st = bandnorm_check("dmel_bandnorm_backward", rows, n_mels, rows_per_clip, T, batch_stats, training, stats, &noop);
    if (st != DMEL_OK) return st;
    if (!g || !s) return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_backward: NULL pointer (g / s)");
    if (!scratch || misaligned(scratch, 16))
        return fail(DMEL_ERR_INVALID_ARGUMENT, "dmel_bandnorm_backward: needs 16-byte aligned scratch of dmel_bandnorm_scratch_bytes(rows, n_mels)");
    if (noop || (!ds_or_null && !dweight_or_null && !dbias_or_null)) return DMEL_OK;      // nothing is written
    const dmel_status sd = hip_device("dmel_bandnorm_backward");
    if (sd != DMEL_OK) return sd;
    dmel::BandNormParams p{};
    p.g = g; p.s = s; p.ds = ds_or_null; p.lengths = frame_lengths_or_null; p.gamma = weight_or_null;
    p.stats = const_cast<double*>(stats); p.partials = static_cast<double*>(scratch); p.band_means = p.partials + 2 * rows;
    p.dweight = dweight_or_null; p.dbias = dbias_or_null;
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.n_mels = n_mels; p.T = T;
    p.batch_stats = batch_stats; p.eval = (batch_stats && !training) ? 1 : 0;
    DMEL_HIP(dmel::launch_bandnorm_bwd(p, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

namespace {
// the element's bits of `fill`: fp32 as it is, bf16 rounded to nearest even (a NaN stays one)
unsigned specmask_fill_bits(float fill, bool bf16)
{
    unsigned u;
    std::memcpy(&u, &fill, sizeof(u));
    if (!bf16) return u;
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
}  // namespace

dmel_status dmel_specmask_draw(int64_t images, int32_t channels, int32_t n_mels, int32_t T, const int32_t* frame_lengths_or_null,
                               int32_t time_param, int32_t time_permille, int32_t n_time, int32_t freq_param, int32_t n_freq,
                               int64_t* rng_state, int32_t advance, int32_t* stripes, void* stream)
{
    const std::string w("dmel_specmask_draw");
    if (images < 0 || images > 0xFFFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": images out of range (the Philox counter holds 32 bits of it)");
    if (channels < 1 || images % channels != 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": channels must be positive and divide images (clip = image / channels)");
    if (n_mels < 1 || T < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": n_mels / T out of range");
    if (n_time < 0 || n_freq < 0 || n_time + n_freq > 8) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": n_time and n_freq must be >= 0 and n_time + n_freq <= 8");
    if (time_param < 0 || freq_param < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": time_param and freq_param must be >= 0");
    if (time_permille < 0 || time_permille > 1000) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": time_permille must lie in 0 ... 1000");
    if (advance != 0 && advance != 1) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": advance is 0 or 1");
    if (!rng_state || misaligned(rng_state, 8)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rng_state must be two 8-byte aligned int64 values (seed, calls)");
    if (n_time + n_freq > 0 && (!stripes || misaligned(stripes, 4)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stripes must be a buffer of images * (n_time + n_freq) * 2 int32 values");
    if (images == 0 || T == 0 || n_time + n_freq == 0) return DMEL_OK;                 // nothing to draw: `calls` stays
    const dmel_status sd = hip_device("dmel_specmask_draw");
    if (sd != DMEL_OK) return sd;
    dmel::SpecMaskDrawParams p{};
    p.lengths = frame_lengths_or_null; p.rng_state = reinterpret_cast<unsigned long long*>(rng_state); p.stripes = stripes;
    p.images = images; p.channels = channels; p.n_mels = n_mels; p.T = T;
    p.time_param = time_param; p.time_permille = time_permille; p.n_time = n_time; p.freq_param = freq_param; p.n_freq = n_freq;
    p.advance = advance;
    DMEL_HIP(dmel::launch_specmask_draw(p, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_specmask_apply(const void* s, int64_t rows, int32_t n_mels, int64_t rows_per_clip, int32_t T,
                                const int32_t* frame_lengths_or_null, const int32_t* stripes, int32_t n_time, int32_t n_freq,
                                int32_t elem_bf16, float fill, void* y, void* stream)
{
    const std::string w("dmel_specmask_apply");
    if (n_mels < 1 || rows < 0 || T < 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows / n_mels / T out of range");
    if (rows_per_clip < 1 || rows_per_clip % n_mels != 0)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows_per_clip must be a positive multiple of n_mels (an image is n_mels rows)");
    if (rows % rows_per_clip != 0) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": rows must be a multiple of rows_per_clip (clip = row / rows_per_clip)");
    if (n_time < 0 || n_freq < 0 || n_time + n_freq > 8) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": n_time and n_freq must be >= 0 and n_time + n_freq <= 8");
    if (elem_bf16 != 0 && elem_bf16 != 1) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": elem_bf16 is 0 (fp32) or 1 (bf16)");
    const int elem_bytes = elem_bf16 ? 2 : 4;
    if (!s || misaligned(s, elem_bytes)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": s must be a buffer aligned to its element");
    if (!y || misaligned(y, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": y must be a 16-byte aligned buffer");
    if (n_time + n_freq > 0 && (!stripes || misaligned(stripes, 4)))
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stripes must be the table dmel_specmask_draw wrote");
    if (rows == 0 || T == 0) return DMEL_OK;
    const int64_t images = rows / n_mels;
    if ((int64_t)n_mels * T > (1LL << 30)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": n_mels * T is too large (an image has at most 2^30 elements)");
    if (images * dmel::specmask_waves_per_image(n_mels, T, elem_bytes) > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    const dmel_status sd = hip_device("dmel_specmask_apply");
    if (sd != DMEL_OK) return sd;
    dmel::SpecMaskParams p{};
    p.s = s; p.y = y; p.lengths = frame_lengths_or_null; p.stripes = stripes;
    p.images = images; p.channels = (int)(rows_per_clip / n_mels); p.n_mels = n_mels; p.T = T; p.n_time = n_time; p.n_freq = n_freq;
    p.fill_bits = specmask_fill_bits(fill, elem_bf16 != 0);
    DMEL_HIP(dmel::launch_specmask_apply(p, elem_bytes, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

namespace {
// both directions of Deltas: `in` / `out` are (s, y) forward and (g, ds) backward
dmel_status deltas_call(const char* what, const char* in_name, const char* out_name, const float* in, int64_t rows, int64_t rows_per_clip,
                        int32_t T, const int32_t* lengths, int32_t win_length, int32_t order, int32_t include_static, float* out, bool backward,
                        void* stream)
{
    const std::string w(what);
    if (const dmel_status st = stage_rows_check(w, rows, rows_per_clip, T); st != DMEL_OK) return st;
    if (win_length != 3 && win_length != 5 && win_length != 7 && win_length != 9)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": win_length must be 3, 5, 7 or 9");
    if (order != 1 && order != 2) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": order must be 1 or 2");
    if (include_static != 0 && include_static != 1) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": include_static is 0 or 1");
    if (!in || misaligned(in, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": " + in_name + " must be a buffer of fp32 values");
    if (!out || misaligned(out, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": " + out_name + " must be a 16-byte aligned buffer");
    if (const dmel_status st = stage_lengths_check(w, lengths); st != DMEL_OK) return st;
    if (rows == 0 || T == 0) return DMEL_OK;
    const int n = (win_length - 1) / 2;
    if (rows > 0x7FFFFFFFLL || dmel::deltas_waves(rows, T, n) > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    const dmel_status sd = hip_device(what);
    if (sd != DMEL_OK) return sd;
    dmel::DeltasParams p{};
    p.in = in; p.out = out; p.lengths = lengths; p.rows = rows; p.rows_per_clip = rows_per_clip;
    p.T = T; p.n = n; p.order = order; p.include_static = include_static; p.groups = include_static + order;
    p.inv_denom = 3.0 / (double)(n * (n + 1) * (2 * n + 1));
    DMEL_HIP(dmel::launch_deltas(p, backward, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}
}  // namespace

dmel_status dmel_deltas_forward(const float* s, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                int32_t win_length, int32_t order, int32_t include_static, float* y, void* stream)
{
    return deltas_call("dmel_deltas_forward", "s", "y", s, rows, rows_per_clip, n_time, frame_lengths_or_null, win_length, order, include_static, y,
                       false, stream);
}

dmel_status dmel_deltas_backward(const float* g, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                 int32_t win_length, int32_t order, int32_t include_static, float* ds, void* stream)
{
    return deltas_call("dmel_deltas_backward", "g", "ds", g, rows, rows_per_clip, n_time, frame_lengths_or_null, win_length, order, include_static,
                       ds, true, stream);
}

namespace {
// what both directions of StatsPool check alike; *noop: nothing to do
dmel_status statspool_check(const std::string& w, int64_t rows, int64_t rows_per_clip, int32_t T, const int32_t* lengths, int32_t which,
                            const double* stats, const int32_t* argmax, bool* noop)
{
    if (const dmel_status st = stage_rows_check(w, rows, rows_per_clip, T); st != DMEL_OK) return st;
    if (which < 1 || which > 7) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": which must lie in 1 ... 7 (bit 0 mean, bit 1 std, bit 2 max)");
    if (const dmel_status st = stage_lengths_check(w, lengths); st != DMEL_OK) return st;
    if (misaligned(stats, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stats must be a 16-byte aligned buffer of 2 * rows doubles");
    if (misaligned(argmax, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": argmax must be int32 values");
    *noop = rows == 0 || T == 0;
    if (!*noop && rows > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    return DMEL_OK;
}
}  // namespace

dmel_status dmel_statspool_forward(const float* s, int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                   int32_t which, double eps, float* y, double* stats_or_null, int32_t* argmax_or_null, void* stream)
{
    const std::string w("dmel_statspool_forward");
    bool noop = false;
    const dmel_status st = statspool_check(w, rows, rows_per_clip, n_time, frame_lengths_or_null, which, stats_or_null, argmax_or_null, &noop);
    if (st != DMEL_OK) return st;
    if (!s || misaligned(s, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": s must be a buffer of fp32 values");
    if (!y || misaligned(y, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": y must be a buffer of fp32 values");
    if ((which & 2) && (!std::isfinite(eps) || !(eps > 0.0))) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": eps must be finite and > 0 when std is selected");
    if (noop) return DMEL_OK;
    const dmel_status sd = hip_device("dmel_statspool_forward");
    if (sd != DMEL_OK) return sd;
    dmel::StatsPoolParams p{};
    p.s = s; p.y = y; p.lengths = frame_lengths_or_null; p.stats = stats_or_null; p.argmax = argmax_or_null;
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.T = n_time; p.which = which; p.S = __builtin_popcount((unsigned)which);
    p.eps = (std::isfinite(eps) && eps > 0.0) ? eps : 0.0;        // (without std an eps that was not checked can still reach `stats`: it must not be a NaN there)
    DMEL_HIP(dmel::launch_statspool(p, false, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_statspool_backward(const float* g, const float* s_or_null, const double* stats_or_null, const int32_t* argmax_or_null,
                                    int64_t rows, int64_t rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null, int32_t which,
                                    float* ds, void* stream)
{
    const std::string w("dmel_statspool_backward");
    bool noop = false;
    const dmel_status st = statspool_check(w, rows, rows_per_clip, n_time, frame_lengths_or_null, which, stats_or_null, argmax_or_null, &noop);
    if (st != DMEL_OK) return st;
    if (!g || misaligned(g, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": g must be a buffer of fp32 values");
    if (!ds || misaligned(ds, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": ds must be a buffer of fp32 values");
    if (misaligned(s_or_null, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": s must be a buffer of fp32 values");
    if ((which & 2) && (!s_or_null || !stats_or_null))
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": std is selected: s and the stats the forward wrote are needed");
    if ((which & 4) && !argmax_or_null) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": max is selected: the argmax the forward wrote is needed");
    if (noop) return DMEL_OK;
    const dmel_status sd = hip_device("dmel_statspool_backward");
    if (sd != DMEL_OK) return sd;
    dmel::StatsPoolParams p{};
    p.g = g; p.s = s_or_null; p.ds = ds; p.lengths = frame_lengths_or_null;
    p.stats = const_cast<double*>(stats_or_null); p.argmax = const_cast<int32_t*>(argmax_or_null);
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.T = n_time; p.which = which; p.S = __builtin_popcount((unsigned)which);
    DMEL_HIP(dmel::launch_statspool(p, true, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

namespace {
// what both directions of AttentivePool check alike; *noop: nothing to do
dmel_status attnpool_check(const std::string& w, const float* s, const float* a, int64_t rows, int64_t rows_per_clip, int64_t logit_rows,
                           int32_t T, const int32_t* lengths, int32_t which, double eps, const double* stats, const double* norm, bool* noop)
{
    if (const dmel_status st = stage_rows_check(w, rows, rows_per_clip, T); st != DMEL_OK) return st;
    if (logit_rows < 1 || rows_per_clip % logit_rows != 0)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": logit_rows_per_clip must be positive and divide rows_per_clip (row r reads logit row r / (rows_per_clip / logit_rows_per_clip))");
    if (which < 1 || which > 3) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": which must lie in 1 ... 3 (bit 0 mean, bit 1 std)");
    if ((which & 2) && (!std::isfinite(eps) || !(eps > 0.0))) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": eps must be finite and > 0 when std is selected");
    if (const dmel_status st = stage_lengths_check(w, lengths); st != DMEL_OK) return st;
    if (!s || misaligned(s, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": s must be a buffer of fp32 values");
    if (!a || misaligned(a, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": a must be a buffer of fp32 logits");
    if (misaligned(stats, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stats must be a 16-byte aligned buffer of 2 * rows doubles");
    if (misaligned(norm, 16)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": norm must be a 16-byte aligned buffer of 2 doubles per logit row");
    if (!stats != !norm) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": stats and norm must both be given or both be NULL");
    *noop = rows == 0 || T == 0;
    if (!*noop && rows > 0x7FFFFFFFLL) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    return DMEL_OK;
}

dmel::AttnPoolParams attnpool_params(const float* s, const float* a, int64_t rows, int64_t rows_per_clip, int64_t logit_rows, int32_t T,
                                     const int32_t* lengths, int32_t which, double eps, const double* stats, const double* norm)
{
    dmel::AttnPoolParams p{};
    p.s = s; p.a = a; p.lengths = lengths; p.stats = const_cast<double*>(stats); p.norm = const_cast<double*>(norm);
    p.rows = rows; p.rows_per_clip = rows_per_clip; p.logit_rows = logit_rows; p.T = T; p.which = which;
    p.S = __builtin_popcount((unsigned)which);
    p.eps = (std::isfinite(eps) && eps > 0.0) ? eps : 0.0;        // (without std an eps that was not checked must not be a NaN in the kernels)
    return p;
}
}  // namespace

dmel_status dmel_attnpool_forward(const float* s, const float* a, int64_t rows, int64_t rows_per_clip, int64_t logit_rows_per_clip,
                                  int32_t n_time, const int32_t* frame_lengths_or_null, int32_t which, double eps, float* y,
                                  double* stats_or_null, double* norm_or_null, void* stream)
{
    const std::string w("dmel_attnpool_forward");
    bool noop = false;
    const dmel_status st = attnpool_check(w, s, a, rows, rows_per_clip, logit_rows_per_clip, n_time, frame_lengths_or_null, which, eps,
                                          stats_or_null, norm_or_null, &noop);
    if (st != DMEL_OK) return st;
    if (!y || misaligned(y, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": y must be a buffer of fp32 values");
    if (noop) return DMEL_OK;
    const dmel_status sd = hip_device("dmel_attnpool_forward");
    if (sd != DMEL_OK) return sd;
    dmel::AttnPoolParams p = attnpool_params(s, a, rows, rows_per_clip, logit_rows_per_clip, n_time, frame_lengths_or_null, which, eps,
                                             stats_or_null, norm_or_null);
    p.y = y;
    DMEL_HIP(dmel::launch_attnpool(p, false, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_attnpool_backward(const float* g, const float* s, const float* a, const double* stats, const double* norm, int64_t rows,
                                   int64_t rows_per_clip, int64_t logit_rows_per_clip, int32_t n_time, const int32_t* frame_lengths_or_null,
                                   int32_t which, double eps, float* ds, float* da, void* stream)
{
    const std::string w("dmel_attnpool_backward");
    bool noop = false;
    const dmel_status st = attnpool_check(w, s, a, rows, rows_per_clip, logit_rows_per_clip, n_time, frame_lengths_or_null, which, eps,
                                          stats, norm, &noop);
    if (st != DMEL_OK) return st;
    if (!g || misaligned(g, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": g must be a buffer of fp32 values");
    if (!ds || misaligned(ds, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": ds must be a buffer of fp32 values");
    if (!da || misaligned(da, 4)) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": da must be a buffer of fp32 values");
    if (!stats || !norm) return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": the stats and norm the forward wrote are needed");
    if (noop) return DMEL_OK;
    if (dmel::attnpool_blocks(rows, rows_per_clip, logit_rows_per_clip, n_time, true) > 0x7FFFFFFFLL)
        return fail(DMEL_ERR_INVALID_ARGUMENT, w + ": too many rows for one launch");
    const dmel_status sd = hip_device("dmel_attnpool_backward");
    if (sd != DMEL_OK) return sd;
    dmel::AttnPoolParams p = attnpool_params(s, a, rows, rows_per_clip, logit_rows_per_clip, n_time, frame_lengths_or_null, which, eps, stats, norm);
    p.g = g; p.ds = ds; p.da = da;
    DMEL_HIP(dmel::launch_attnpool(p, true, reinterpret_cast<hipStream_t>(stream)));
    return DMEL_OK;
}

dmel_status dmel_plan_set_profiling(dmel_plan* plan, int32_t enable)
{
    if (!plan) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    plan->profiling = enable != 0;
    return DMEL_OK;
}

dmel_status dmel_plan_get_profile(dmel_plan* plan, dmel_profile* profile)
{
    if (!plan || !profile) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan / profile is NULL");
    std::lock_guard<std::mutex> lock(plan->mu);
    dmel_profile pr{};
    for (const auto& sp : plan->spans) {
        DMEL_HIP(hipEventSynchronize(plan->ev_pool[sp.b]));
        float ms = 0.f;
        DMEL_HIP(hipEventElapsedTime(&ms, plan->ev_pool[sp.a], plan->ev_pool[sp.b]));
        if (sp.kind == 0) { pr.prep_ms += ms; ++pr.prep_launches; }
        else if (sp.kind == 1) { pr.fwd_ms += ms; ++pr.fwd_launches; }
        else { pr.bwd_ms += ms; ++pr.bwd_launches; }
    }
    plan->spans.clear();
    plan->ev_used = 0;
    *profile = pr;
    return DMEL_OK;
}

dmel_status dmel_plan_get_info(const dmel_plan* plan, dmel_plan_info* info)
{
    if (!plan || !info) return fail(DMEL_ERR_INVALID_ARGUMENT, "plan / info is NULL");
    *info = plan->info;
    return DMEL_OK;
}

}  // extern "C"
