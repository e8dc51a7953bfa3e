// Drives csrc/dmel_lamtrack.h over a synthetic ring (tests/test_lamtrack_cpu.py compiles this with the host compiler and the address
// and undefined-behaviour sanitizers; no HIP, no GPU).  Expected values are worked out by hand from the rule; the arithmetic is in the
// comments.  `lamtrack_driver nfft v ...` prints the n_fft of every value instead (compared with the oracle by the test).
#include "dmel_lamtrack.h"

#include <cstdio>
#include <cstdlib>

using dmel::LamTrack;
namespace lt = dmel::lamtrack;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

constexpr unsigned R = 8;                     // reports in the ring; word R is the sticky error word
struct Ring {
    unsigned long long w[R + 1] = {};
    static unsigned long long word(unsigned seq, float lam) { unsigned b; std::memcpy(&b, &lam, 4); return ((unsigned long long)seq << 32) | b; }
    void report(unsigned seq, float lam) { w[seq % R] = word(seq, lam); }
};

static bool near(float v, float want, float tol) { return std::fabs(v - want) <= tol; }

// reports (10, 84.0), (11, 84.05), (15, 84.25), (19, 84.45), observed one at a time
static void feed_four(LamTrack* t, Ring* r)
{
    r->report(10, 84.0f);  lt::observe(t, r->w, R);
    r->report(11, 84.05f); lt::observe(t, r->w, R);
    r->report(15, 84.25f); lt::observe(t, r->w, R);
    r->report(19, 84.45f); lt::observe(t, r->w, R);
}

static void decide_is(const LamTrack& t, int mode, int max_ahead, bool capturing, int n_want, int g_want, int line)
{
    int n = -1, g = -1;
    lt::decide(t, mode, max_ahead, capturing, &n, &g);
    if (n != n_want || g != g_want) { std::printf("FAILED line %d: decided (%d, %d), expected (%d, %d)\n", line, n, g, n_want, g_want); ++failures; }
}
#define DECIDE(t, mode, ahead, cap, n, g) decide_is(t, mode, ahead, cap, n, g, __LINE__)

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "nfft") == 0) {
        for (int i = 2; i < argc; ++i) std::printf("%d\n", (int)lt::n_fft((float)std::strtod(argv[i], nullptr)));
        return 0;
    }
    {   // an empty ring observes nothing
        LamTrack t; Ring r;
        CHECK(!lt::observe(&t, r.w, R));
        CHECK(!t.lam_known && t.n_obs == 0 && t.issued == 0 && t.lam_rate == 0.f);
    }
    {   // the four reports in order
        LamTrack t; Ring r;
        r.report(10, 84.0f);
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.n_obs == 1 && t.lam_known && t.lam_seen == 84.0f && t.seq_seen == 10 && t.issued == 10);
        CHECK(t.lam_rate == 0.f);                                  // one value: no difference yet
        r.report(11, 84.05f);
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.n_obs == 2 && near(t.lam_rate, 0.05f, 1e-4f));     // |84.05 - 84.0| / (11 - 10) = 0.05
        r.report(15, 84.25f);
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.n_obs == 3 && near(t.lam_rate, 0.05f, 1e-4f));     // max(0.98 * 0.05 = 0.049, |84.25 - 84.05| / (15 - 11) = 0.05) = 0.05
        r.report(19, 84.45f);                                      // (slot 19 % 8 = 3: overwrites report 11, as a full ring does)
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.n_obs == 4 && near(t.lam_rate, 0.05f, 1e-4f));     // max(0.049, |84.45 - 84.25| / 4 = 0.05) = 0.05
        CHECK(t.lam_seen == 84.45f && t.seq_seen == 19);
        CHECK(t.issued == 19);                                     // pulled up: the host had counted none of these executions
        // n_fft(84.45): int(84.45 * 6 = 506.7) = 506, (506 - 1).bit_length() = 9 -> 512.  Guards need (a - reach) * 6 < 257 or
        // (a + reach) * 6 >= 513 with reach = 2 * rate * stale + 1e-5 * a, stale = issued - seq_seen + 2
        DECIDE(t, 0, 8, false, 512, 0);                            // stale 2: reach 0.2 + 0.0008, (84.45 + 0.2008) * 6 = 507.9 < 513
        t.issued = 19 + 8;
        DECIDE(t, 0, 8, false, 512, 0);                            // stale 10: reach 1.0008, (84.45 + 1.0008) * 6 = 512.7 < 513
        t.issued = 19 + 10;
        DECIDE(t, 0, 8, false, 512, 2);                            // stale 12: (84.45 + 2 * 0.05 * 12 + 0.0008) * 6 = 513.9 >= 513
        t.issued = 19;
        // observing the same ring twice changes nothing
        const LamTrack before = t;
        CHECK(!lt::observe(&t, r.w, R));
        CHECK(t.issued == before.issued && t.seq_seen == before.seq_seen && t.seq_floor == before.seq_floor && t.lam_known == before.lam_known &&
              t.lam_seen == before.lam_seen && t.lam_rate == before.lam_rate && t.n_obs == before.n_obs && t.last_guards == before.last_guards);
        // guard mode 1 always gives both guards, mode 2 never does
        DECIDE(t, 1, 8, false, 512, 3);
        DECIDE(t, 1, 8, true, 512, 3);
        DECIDE(t, 2, 8, false, 512, 0);
        DECIDE(t, 2, 8, true, 512, 0);
        // under capture: mode 0 guards both (nobody manages the graph); mode 3 decides as eagerly with max_ahead more stale forwards
        DECIDE(t, 0, 8, true, 512, 3);
        DECIDE(t, 3, 8, true, 512, 0);                             // stale 0 + 2 + 8 = 10: 512.7 < 513, as above
        DECIDE(t, 3, 10, true, 512, 2);                            // stale 0 + 2 + 10 = 12: 513.9 >= 513
        DECIDE(t, 3, 10, false, 512, 0);                           // eager: max_ahead does not count
        // the status of this picture; the error word is looked at and stays
        t.last_guards = 2;
        r.w[R] = Ring::word(23, 170.5f);
        dmel_lambd_status st{};
        lt::fill_status(t, r.w, R, &st);
        CHECK(st.known == 1 && st.lambd_seen == 84.45f && st.n_fft_seen == 512 && st.seq_issued == 19 && st.seq_seen == 19);
        CHECK(st.rate == t.lam_rate && st.guards == 2 && st.next_n_fft == 0 && st.next_guards == 0);       // next_*: the caller's (decide)
        CHECK(st.error == 1 && st.error_seq == 23 && st.error_lambd == 170.5f && r.w[R] != 0);
        // take_error returns the number and the value and leaves the word zero
        unsigned seq = 0; float lam = 0.f;
        CHECK(lt::take_error(r.w, R, &seq, &lam) && seq == 23 && lam == 170.5f && r.w[R] == 0);
        CHECK(!lt::take_error(r.w, R, &seq, &lam));
        lt::fill_status(t, r.w, R, &st);
        CHECK(st.error == 0 && st.error_seq == 0);
        // after reset a report numbered at or below the old `issued` is ignored, one above it is taken
        lt::reset(&t);
        CHECK(!t.lam_known && t.n_obs == 0 && t.lam_rate == 0.f && t.seq_seen == 19 && t.seq_floor == 20 && t.issued == 19);
        CHECK(!lt::observe(&t, r.w, R));                           // 10, 15, 19 are still in the ring: all below the floor
        r.report(18, 50.0f);
        CHECK(!lt::observe(&t, r.w, R));
        lt::fill_status(t, r.w, R, &st);
        CHECK(st.known == 0 && st.n_fft_seen == 0);
        r.report(20, 50.0f);
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.lam_known && t.lam_seen == 50.0f && t.seq_seen == 20 && t.issued == 20 && t.n_obs == 1 && t.lam_rate == 0.f);
    }
    {   // fewer than two observations give both guards
        LamTrack t; Ring r;
        r.report(1, 84.0f);
        lt::observe(&t, r.w, R);
        DECIDE(t, 0, 8, false, 512, 3);                            // int(504) = 504, (503).bit_length() = 9 -> 512
        DECIDE(t, 3, 8, false, 512, 3);
        DECIDE(t, 2, 8, false, 512, 0);
    }
    {   // the cold start catches `issued` up with the ring and starts the picture from the value read
        LamTrack t; Ring r;
        LamTrack other;
        feed_four(&other, &r);
        t.issued = 3;
        lt::cold_start(&t, r.w, R, 33.0f);
        CHECK(t.issued == 19 && t.seq_seen == 19 && t.lam_known && t.lam_seen == 33.0f && t.n_obs == 0 && t.lam_rate == 0.f);
        CHECK(!lt::observe(&t, r.w, R));                           // nothing in the ring is newer than 19
    }
    {   // sequence numbers straddling 2^32
        LamTrack t; Ring r;
        t.issued = 0xfffffff0u;
        lt::reset(&t);                                             // floor 0xfffffff1
        r.report(0xffffffe9u, 19.0f);                              // older than the reset: (int)(0xffffffe9 - 0xfffffff1) = -8
        CHECK(!lt::observe(&t, r.w, R));
        r.report(0xfffffff8u, 20.0f);                              // 7 past the floor
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.seq_seen == 0xfffffff8u && t.issued == 0xfffffff8u && t.lam_seen == 20.0f);
        r.report(5u, 20.5f);                                       // 13 executions later, past the wrap: (int)(5 - 0xfffffff8) = 13 > 0
        r.report(0xfffffff2u, 7.0f);                               // a stale word: (int)(0xfffffff2 - 0xfffffff8) = -6, not newer
        CHECK(lt::observe(&t, r.w, R));
        CHECK(t.seq_seen == 5u && t.issued == 5u && t.lam_seen == 20.5f && t.n_obs == 2);
        CHECK(near(t.lam_rate, 0.5f / 13.0f, 1e-6f));              // |20.5 - 20.0| / 13
        t.issued = 9u;                                             // four eager calls in flight: stale = 9 - 5 + 2 = 6
        // n_fft(20.5) = 128 (int(123) = 123, (122).bit_length() = 7); reach = 2 * 0.03846 * 6 + 0.0002 = 0.4617: (20.5 + 0.4617) * 6 = 125.8 < 129,
        // (20.5 - 0.4617) * 6 = 120.2 >= 65
        DECIDE(t, 0, 8, false, 128, 0);
        LamTrack u;                                                // both sides of the wrap in the ring at the first look: the later one wins
        u.issued = 0xfffffff0u;
        lt::reset(&u);
        CHECK(lt::observe(&u, r.w, R) && u.seq_seen == 5u && u.n_obs == 1);
        LamTrack v;                                                // a floor just below the wrap
        v.issued = 0xfffffffeu;
        lt::reset(&v);                                             // floor 0xffffffff
        Ring q;
        q.report(0xfffffffdu, 1.0f);
        CHECK(!lt::observe(&v, q.w, R));
        q.report(2u, 2.0f);                                        // (int)(2 - 0xffffffff) = 3 >= 0
        CHECK(lt::observe(&v, q.w, R) && v.seq_seen == 2u && v.lam_seen == 2.0f);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("lamtrack: all checks passed\n");
    return 0;
}
