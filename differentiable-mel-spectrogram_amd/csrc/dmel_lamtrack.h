// dmel_lamtrack.h -- the host's picture of one device-resident lambd, free of HIP: arithmetic over a pinned ring of n words
// (number << 32) | bits(lambd), one per executed forward in slot number % n, and the sticky error word ring[n] behind it (dmel_kernels.h).
// Sequence numbers wrap: every comparison is the sign of a 32-bit difference.  Run without a GPU by tests/test_lamtrack_cpu.py.
#pragma once
#include "../../include/dmel.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace dmel {
struct LamTrack {
    unsigned issued = 0;           // the host's estimate of the number its most recent eager forward drew (caught up with the reports: replays)
    unsigned seq_seen = 0;         // execution number the observation belongs to
    unsigned seq_floor = 0;        // reports with a smaller number predate the last reset
    bool lam_known = false;        // lam_seen / seq_seen hold an observation
    float lam_seen = 0.f;
    float lam_rate = 0.f;          // decayed maximum of |d lambd| per execution
    int n_obs = 0;                 // observations since the last reset
    int last_guards = 0;           // bit 0: n_fft/2 launched, bit 1: 2 n_fft launched (most recent call)
};

namespace lamtrack {
constexpr int kMaxGuardNfft = 1 << 20;      // no guard launch beyond the longest transform of the HIP path (dmel::kMaxBigFft)

// n_fft of lambd (exported as dmel_n_fft)
inline int32_t n_fft(float lambd)
{
    const float a = std::fabs(lambd);       // models.py:38
    const float prod = a * 6.0f;            // time_frequency.py:39, fp32 tensor product
    if (!(prod < 9.0e15f)) return 0x40000000;
    long long x = (long long)prod;          // time_frequency.py:61 int(): truncation
    long long v = x - 1;
    int bits = 0;
    if (v < 0) bits = 1;                    // python: (-1).bit_length() == 1
    else while (v > 0) { ++bits; v >>= 1; }
    if (bits > 30) return 0x40000000;
    return (int32_t)(1LL << bits);          // time_frequency.py:62
}

// exported as dmel_decide_launch: n_fft, and the neighbours within reach when lambd moves by `rate` per forward for `stale` forwards (margin 2)
inline void decide_launch(float lambd, float rate, float stale, int* n_fft_out, int* guards)
{
    const float a = std::fabs(lambd);
    const int N = n_fft(lambd);
    int g = 0;
    const float reach = 2.0f * rate * stale + 1e-5f * a;
    if ((a - reach) * 6.0f < (float)(N / 2 + 1)) g |= 1;
    if ((a + reach) * 6.0f >= (float)N + 1.0f) g |= 2;
    if (2 * N > kMaxGuardNfft) g &= ~2;
    if (N < 2) g &= ~1;
    *n_fft_out = N; *guards = g;
}

// forget what was seen: reports numbered up to `issued` predate the reset
inline void reset(LamTrack* t) { t->lam_known = false; t->n_obs = 0; t->lam_rate = 0.f; t->seq_seen = t->issued; t->seq_floor = t->issued + 1; }

// fold the latest report (the highest number past the last one seen and past the last reset: eager call or replay) in; false if nothing new
inline bool observe(LamTrack* t, const unsigned long long* ring, unsigned n)
{
    bool any = false;
    unsigned best_seq = 0; unsigned best_bits = 0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned long long w = __atomic_load_n(&ring[i], __ATOMIC_RELAXED);
        const unsigned seq = (unsigned)(w >> 32);
        if (seq == 0 || (int)(seq - t->seq_floor) < 0) continue;                       // empty, or older than the last reset
        if (t->lam_known ? (int)(seq - t->seq_seen) <= 0 : false) continue;            // not newer than what is known
        if (!any || (int)(seq - best_seq) > 0) { best_seq = seq; best_bits = (unsigned)w; any = true; }
    }
    if (!any) return false;
    float lam; std::memcpy(&lam, &best_bits, 4);
    if (t->lam_known && t->n_obs >= 1) {
        const unsigned dseq = best_seq - t->seq_seen;
        const float r = std::fabs(lam - t->lam_seen) / (float)(dseq ? dseq : 1);
        t->lam_rate = std::max(0.98f * t->lam_rate, r);
    }
    t->lam_seen = lam; t->seq_seen = best_seq; t->lam_known = true; ++t->n_obs;
    if ((int)(best_seq - t->issued) > 0) t->issued = best_seq;                        // replays executed forwards the host never counted
    return true;
}

// the next forward's n_fft and guards (bit 0: n_fft / 2, bit 1: 2 n_fft): both while the drift is unknown, in mode 1, and under a capture nobody
// manages (modes 0, 1); never in mode 2; otherwise the ones within reach of a boundary before the host would notice
inline void decide(const LamTrack& t, int guard_mode, int max_ahead, bool capturing, int* n_fft_out, int* guards)
{
    const int N = n_fft(t.lam_seen);
    int g = 0;
    if (guard_mode == 1 || (capturing && guard_mode != 3 && guard_mode != 2)) g = 3;
    else if (guard_mode == 0 || guard_mode == 3) {
        if (t.n_obs < 2) g = 3;
        else {
            const float stale = (float)(t.issued - t.seq_seen) + 2.0f + (capturing ? (float)max_ahead : 0.f);
            int n2 = 0;
            decide_launch(t.lam_seen, t.lam_rate, stale, &n2, &g);
        }
    }
    if (2 * N > kMaxGuardNfft) g &= ~2;
    if (N < 2) g &= ~1;
    *n_fft_out = N; *guards = g;
}

// cold start, after the one blocking read gave `lam` on an idle stream: every earlier report is in the ring, so uncounted replays are caught up with
inline void cold_start(LamTrack* t, const unsigned long long* ring, unsigned n, float lam)
{
    for (unsigned i = 0; i < n; ++i) {
        const unsigned q = (unsigned)(__atomic_load_n(&ring[i], __ATOMIC_RELAXED) >> 32);
        if (q != 0 && (int)(q - t->issued) > 0) t->issued = q;
    }
    t->lam_seen = lam; t->seq_seen = t->issued; t->lam_known = true; t->n_obs = 0; t->lam_rate = 0.f;
}

// reads and clears the sticky error word ring[n]; true if it was set: *seq is the execution that no launch covered, *lam the lambd it read
inline bool take_error(unsigned long long* ring, unsigned n, unsigned* seq, float* lam)
{
    const unsigned long long err = __atomic_load_n(&ring[n], __ATOMIC_RELAXED);
    if (err == 0) return false;
    __atomic_store_n(&ring[n], 0ull, __ATOMIC_RELAXED);
    const unsigned bits = (unsigned)err; std::memcpy(lam, &bits, 4); *seq = (unsigned)(err >> 32);
    return true;
}

// the fields of dmel_lambd_status that the picture and its words hold (the error word is looked at, not cleared); next_* and calls are the caller's
inline void fill_status(const LamTrack& t, const unsigned long long* ring, unsigned n, dmel_lambd_status* r)
{
    r->known = t.lam_known ? 1 : 0; r->lambd_seen = t.lam_seen; r->n_fft_seen = t.lam_known ? n_fft(t.lam_seen) : 0;
    r->seq_issued = t.issued; r->seq_seen = t.seq_seen; r->rate = t.lam_rate; r->guards = t.last_guards;
    const unsigned long long err = __atomic_load_n(&ring[n], __ATOMIC_RELAXED);
    const unsigned bits = (unsigned)err;
    r->error = err != 0 ? 1 : 0; r->error_seq = (uint32_t)(err >> 32); std::memcpy(&r->error_lambd, &bits, 4);
}
}  // namespace lamtrack
}  // namespace dmel
