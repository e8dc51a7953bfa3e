// dmel_tables.cpp -- host arithmetic of the tables (dmel_tables.h): one function per table, no HIP runtime call.
#include "dmel_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

namespace dmel {

// ---- geometry queries of the fused kernel (declared in dmel_kernels.h): constexpr look-ups, here so that a program without kernels links them
bool forward_has_hsplit(int n_fft) { return n_fft >= kHsplitMinNfft && n_fft <= kHsplitMaxNfft && (n_fft & (n_fft - 1)) == 0; }
bool forward_has_wlc(int n_fft) { return wlc_size(n_fft); }
bool forward_wlc_one_frame(int n_fft) { return wlc_size(n_fft) && n_fft >= 2048; }      // (G = 64: the frame fills the wave)

// the geometry of the unpaired plan for a run-time n_fft, or the paired one's
template <class F> static bool with_geom(int n_fft, bool pair, F&& f)
{
    return with_nfft(n_fft, [&](auto nn) { constexpr int N = decltype(nn)::value; f(pair ? geom<N, true>() : geom<N, false>()); });
}

// (R, C) of the plan for n_fft: the host builds the twiddle tables from these
bool forward_plan_rc(int n_fft, bool pair, int* R, int* C)
{
    return with_geom(n_fft, pair, [&](const FftGeom& g) { *R = g.R; *C = g.C; });
}

// the layout of tile_ranges / ent_pre depends on these two; they are the same for both plans of a size
int forward_waves(int n_fft)
{
    int v = -1;
    with_geom(n_fft, false, [&](const FftGeom& g) { v = g.WAVES; });
    return v;
}

int forward_nbpre(int n_fft)
{
    int v = -1;
    with_geom(n_fft, false, [&](const FftGeom& g) { v = g.NBPRE; });
    return v;
}

// ---- the HTK bank ---------------------------------------------------------------------------------------------------------------------
// torch.linspace (fp32, CPU): symmetric evaluation around the midpoint
void linspace_f32(float start, float end, int steps, std::vector<float>& out)
{
    out.resize(steps);
    if (steps == 1) { out[0] = start; return; }
    const float step = (end - start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i)
        out[i] = i < half ? std::fmaf(step, (float)i, start) : std::fmaf(-step, (float)(steps - i - 1), end);   // (torch's CPU kernel fuses the multiply-add: tests/golden/g8_fbanks.npz)
}

void mel_fbanks_htk(int n_freqs, double f_min, double f_max, int n_mels, int sample_rate, float* fb)
{
    std::vector<float> all_freqs, m_pts, f_pts(n_mels + 2);
    linspace_f32(0.0f, (float)(sample_rate / 2), n_freqs, all_freqs);
    const double m_min = 2595.0 * std::log10(1.0 + f_min / 700.0);
    const double m_max = 2595.0 * std::log10(1.0 + f_max / 700.0);
    linspace_f32((float)m_min, (float)m_max, n_mels + 2, m_pts);
    // 10 ** (m / 2595) as torch evaluates it: the CORRECTLY ROUNDED fp32 power (measured against torch 2.10: all 130 points of the 128-band bank;
    // glibc's powf is 1 ulp off at 19 of them, which moved filterbank entries by up to 1.5e-5 -- tests/golden/g8_fbanks.npz)
    for (int i = 0; i < n_mels + 2; ++i) {
        const float e = m_pts[i] / 2595.0f;
        f_pts[i] = 700.0f * ((float)std::pow(10.0, (double)e) - 1.0f);
    }
    for (int f = 0; f < n_freqs; ++f)
        for (int m = 0; m < n_mels; ++m) {
            const float down = (-1.0f * (f_pts[m] - all_freqs[f])) / (f_pts[m + 1] - f_pts[m]);
            const float up = (f_pts[m + 2] - all_freqs[f]) / (f_pts[m + 2] - f_pts[m + 1]);
            fb[(size_t)f * n_mels + m] = std::max(0.0f, std::min(down, up));
        }
}

// ---- tables of every n_fft ------------------------------------------------------------------------------------------------------------
RowTables build_row_tables(const std::vector<float>& fb, int F, int M)
{
    RowTables rt;
    rt.rowband.resize(F);
    for (int f = 0; f < F; ++f) {
        int lo = M, hi = 0;
        for (int m = 0; m < M; ++m)
            if (fb[(size_t)f * M + m] != 0.f) { lo = std::min(lo, m); hi = m + 1; }
        rt.rowband[f] = make_int2(hi > lo ? lo : 0, hi > lo ? hi : 0);
    }
    rt.rowpk.resize(F);
    for (int f = 0; f < F; ++f) {
        const int b0 = rt.rowband[f].x, nb = rt.rowband[f].y - rt.rowband[f].x;
        float bits0, bitsn;
        std::memcpy(&bits0, &b0, 4); std::memcpy(&bitsn, &nb, 4);
        rt.rowpk[f] = make_float4(nb > 0 ? fb[(size_t)f * M + b0] : 0.f, nb > 1 ? fb[(size_t)f * M + b0 + 1] : 0.f, bits0, bitsn);
        if (nb > 2) rt.long_rows = true;
    }
    return rt;
}

TransposedBank build_transposed_bank(const std::vector<float>& fb, int F, int M)
{
    TransposedBank t;
    t.fbT.resize((size_t)M * F);
    t.band.resize(M);
    for (int m = 0; m < M; ++m) {
        int lo = F, hi = 0;
        for (int f = 0; f < F; ++f) {
            const float c = fb[(size_t)f * M + m];
            t.fbT[(size_t)m * F + f] = c;
            if (c != 0.f) { lo = std::min(lo, f); hi = f + 1; }
        }
        t.band[m] = make_int2(hi > lo ? lo : 0, hi > lo ? hi : 0);
    }
    return t;
}

std::vector<float2> build_long_twiddles(int N)
{
    std::vector<float2> tw((size_t)(N / 2));
    for (int k = 0; k < N / 2; ++k) {
        const double th = -2.0 * M_PI * (double)k / (double)N;
        tw[k] = make_float2((float)std::cos(th), (float)std::sin(th));
    }
    return tw;
}

PlanTwiddles build_plan_twiddles(int N, int R, int C)
{
    const int G = N / R;
    PlanTwiddles t;
    t.tw1.resize((size_t)R * G); t.tw2.resize((size_t)R * C);
    for (int q = 0; q < R; ++q)
        for (int lg = 0; lg < G; ++lg) {
            const double th = -2.0 * M_PI * (double)((long long)lg * q % N) / (double)N;
            t.tw1[(size_t)q * G + lg] = make_float2((float)std::cos(th), (float)std::sin(th));
        }
    for (int p1 = 0; p1 < R; ++p1)
        for (int r = 0; r < C; ++r) {
            const double th = -2.0 * M_PI * (double)(r * p1 % G) / (double)G;
            t.tw2[(size_t)p1 * C + r] = make_float2((float)std::cos(th), (float)std::sin(th));
        }
    return t;
}

// ---- the MFMA B-fragment stream -------------------------------------------------------------------------------------------------------
// The contraction phase of an 8-wave plan (and of a 4-wave plan with up to four mel tiles per group): wave tl owns tile tl; the
// units (4 k-steps = 16 bins) of a tile beyond a common limit L go, in contiguous pieces, to the run 1 of other waves (one piece per
// wave).  L = the smallest limit for which "largest remainder first onto largest spare first" fits.  own[w]: units wave w takes of its
// own tile; pieces: (helper wave, tile, first unit, units).  Pure host arithmetic (dmel_contraction_partition_host exposes it to tests).
void deal_ksteps(const int* units, int ntg, int W, int* own, std::vector<Piece>* pieces)
{
    int total = 0, umax = 0;
    for (int tl = 0; tl < ntg; ++tl) { total += units[tl]; umax = std::max(umax, units[tl]); }
    for (int L = std::max(1, (total + W - 1) / W); ; ++L) {
        pieces->clear();
        int spare[8], rem[8];
        bool used[8] = {false, false, false, false, false, false, false, false};
        for (int w = 0; w < 8; ++w) {
            if (w >= W) { own[w] = 0; rem[w] = 0; spare[w] = 0; used[w] = true; continue; }
            own[w] = w < ntg ? std::min(units[w], L) : 0;
            rem[w] = w < ntg ? units[w] - own[w] : 0;
            spare[w] = L - own[w];
        }
        bool ok = true;
        for (;;) {
            int t = -1;
            for (int tl = 0; tl < ntg; ++tl) if (rem[tl] > 0 && (t < 0 || rem[tl] > rem[t])) t = tl;
            if (t < 0) break;
            int h = -1;
            for (int w = 0; w < 8; ++w) if (!used[w] && w != t && spare[w] > 0 && (h < 0 || spare[w] > spare[h])) h = w;
            if (h < 0) { ok = false; break; }
            const int n = std::min(spare[h], rem[t]);
            pieces->push_back({h, t, units[t] - rem[t], n});
            used[h] = true; rem[t] -= n;
        }
        if (ok) return;
        if (L >= umax) {                      // (not reached: at L = umax nothing is left over)
            pieces->clear();
            for (int w = 0; w < 8; ++w) own[w] = w < ntg ? units[w] : 0;
            return;
        }
    }
}

BStream build_b_stream(const std::vector<float>& fb, int F, int M, int waves)
{
    // Non-zero 4 x 16 blocks of the filterbank as MFMA B-fragments.  Mel tiles are handled in
    // groups of 8 (128 mel bands); inside a group a 4-wave plan gives wave w tiles w and 7-w (the HTK bands
    // widen with frequency, so pairing a narrow and a wide tile balances the four waves), an 8-wave plan
    // deals the k-steps themselves (below).
    BStream bs;
    bs.KS = (F + 3) / 4;
    bs.NT = (M + 15) / 16;
    bs.groups = (bs.NT + 7) / 8;
    bs.n_dense = bs.KS * bs.NT;
    std::vector<int4>& ranges = bs.tile_ranges;
    ranges.assign((size_t)bs.groups * waves * 2, make_int4(0, 0, 0, -1));
    std::vector<float>& bfr = bs.ent_b;
    bs.n_entries = 0;
    // run of k-steps [ks_a, ks_b) of mel tile `tile` appended to the B-fragment stream
    auto emit = [&](int tile, int ks_a, int ks_b) {
        int4 tr = make_int4(ks_a, ks_b - ks_a, (int)bfr.size(), tile);
        for (int ks = ks_a; ks < ks_b; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int f = 4 * ks + (l >> 4), m = 16 * tile + (l & 15);
                bfr.push_back((f < F && m < M) ? fb[(size_t)f * M + m] : 0.f);
            }
        return tr;
    };
    for (int g = 0; g < bs.groups; ++g) {
        const int ntg = std::min(8, bs.NT - 8 * g);
        // the band of a mel tile is one contiguous run of k-steps: [first, first + nks) in units of 4 k-steps (16 bins)
        int first_of[8], units[8];
        for (int tl = 0; tl < ntg; ++tl) {
            const int tile = 8 * g + tl;
            int first = bs.KS, last = -1;
            for (int ks = 0; ks < bs.KS; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int f = 4 * ks + (l >> 4), m = 16 * tile + (l & 15);
                    if (f < F && m < M && fb[(size_t)f * M + m] != 0.f) { first = std::min(first, ks); last = std::max(last, ks); }
                }
            if (last < first) { first_of[tl] = 0; units[tl] = 0; continue; }      // an all-zero tile still needs its outputs written
            bs.n_entries += last - first + 1;
            first = first / 4 * 4;                       // groups of 4 k-steps start at multiples of 16 bins
            first_of[tl] = first; units[tl] = (last - first + 1 + 3) / 4;
        }
        if (waves == 8 || (ntg <= waves && g < 32)) {         // (FwdParams::xch_groups is a 32-bit mask: groups beyond it keep whole tiles -- ADVICE r04)
            // (4-wave plans, n_fft <= 512: only when every tile has a wave of its own -- up to 64 mels, the reference's experiments --
            // since run 1 is then free to carry a piece; with more tiles wave w owns tiles w and 7 - w whole, as before)
            // Wave tl owns tile tl (run 0: it writes the tile's outputs).  The HTK bands widen with frequency -- at 128 mels the last
            // tile has five times the k-steps of the first, at 64 mels four tiles meet eight waves -- so the k-steps of the wide
            // tiles beyond a common limit L are dealt, in contiguous pieces, to the run 1 of waves with narrow or no tiles of their
            // own (one piece per wave; their sums reach the owner through LDS, dmel_fwd_kernel's exchange).  L = the smallest
            // limit for which largest-remainder-first onto largest-spare-first fits.  (Round 3 split every tile in two halves,
            // wave tl and 7 - tl: the slowest wave carried 24 k-steps at BASELINE config 2 where 19.5 is the mean, 56 / 36.5 at
            // config 5, 120 / 68 at the reference's ESC-50 shape at n_fft 4096.)
            const int W = waves;
            int own[8];
            std::vector<Piece> pieces;
            deal_ksteps(units, ntg, W, own, &pieces);
            int mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (const Piece& pc : pieces) mask[pc.tile] |= 1 << pc.wave;
            for (int tl = 0; tl < ntg; ++tl) {
                int4 tr = units[tl] > 0 ? emit(8 * g + tl, first_of[tl], first_of[tl] + 4 * own[tl]) : make_int4(0, 0, 0, 8 * g + tl);
                tr.w |= mask[tl] << 16;
                ranges[(size_t)(g * W + tl) * 2 + 0] = tr;
            }
            for (const Piece& pc : pieces) {
                int4 tr = emit(8 * g + pc.tile, first_of[pc.tile] + 4 * pc.a, first_of[pc.tile] + 4 * (pc.a + pc.n));
                tr.w |= 1 << 30;                                   // a piece: summed into its owner's tile, not written by this wave
                ranges[(size_t)(g * W + pc.wave) * 2 + 1] = tr;
            }
            if (W != 8 && !pieces.empty()) bs.xch_groups |= 1u << g;       // g < 32 here
        } else {
            // 4 waves: wave w owns tiles w and 7-w whole
            for (int tl = 0; tl < ntg; ++tl) {
                const int w = tl < 4 ? tl : 7 - tl, loc = tl < 4 ? 0 : 1;
                ranges[(size_t)(g * 4 + w) * 2 + loc] = units[tl] > 0 ? emit(8 * g + tl, first_of[tl], first_of[tl] + 4 * units[tl]) : make_int4(0, 0, 0, 8 * g + tl);
            }
        }
    }
    return bs;
}

// register-resident prefix of every run of group 0, at a fixed position per (wave, run)
RegPrefix build_reg_prefix(const BStream& bs, int waves, int nbpre)
{
    RegPrefix rp;
    rp.ent_pre.assign((size_t)waves * 2 * nbpre * 64, 0.f);
    for (int w = 0; w < waves; ++w)
        for (int loc = 0; loc < 2; ++loc) {
            const int4 tr = bs.tile_ranges[(size_t)w * 2 + loc];
            const int n = std::min(tr.y, nbpre);
            rp.pre_groups[w * 2 + loc] = (n + 3) / 4;
            if (n > 0)
                std::copy(bs.ent_b.begin() + tr.z, bs.ent_b.begin() + tr.z + (size_t)n * 64, rp.ent_pre.begin() + ((size_t)(w * 2 + loc) * nbpre) * 64);
        }
    return rp;
}

SplitBf16 build_split_bf16(const std::vector<float>& fb, int N, int M)
{
    // the same matrix as B fragments of v_mfma_f32_16x16x32_bf16, split into two bf16 halves (DMEL_FLAG_MFMA_BF16X3):
    // [(tile * (N/64) + kstep) * 2 + (hi | lo)][lane][8]: lane l holds rows 32 kstep + 8 (l >> 4) + e of column 16 tile + (l & 15)
    const int F = N / 2 + 1, NT = (M + 15) / 16, ks32 = N / 64;
    auto bf16_rne = [](float v) -> unsigned short {
        unsigned u; std::memcpy(&u, &v, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);      // NaN stays NaN
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    };
    SplitBf16 sb;
    std::vector<unsigned short>& eh = sb.ent_h;
    eh.resize((size_t)NT * ks32 * 2 * 64 * 8);
    for (int tile = 0; tile < NT; ++tile)
        for (int ks = 0; ks < ks32; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int f = 32 * ks + 8 * (l >> 4) + e, m = 16 * tile + (l & 15);
                    const float v = (m < M) ? fb[(size_t)f * M + m] : 0.f;
                    const unsigned short hi = bf16_rne(v);
                    unsigned hu = (unsigned)hi << 16; float hf; std::memcpy(&hf, &hu, 4);
                    const unsigned short lo = bf16_rne(v - hf);
                    const size_t base = ((size_t)(tile * ks32 + ks) * 2) * 64 * 8;
                    eh[base + (size_t)l * 8 + e] = hi;
                    eh[base + 64 * 8 + (size_t)l * 8 + e] = lo;
                }
    sb.fb_nyq.assign(fb.begin() + (size_t)(F - 1) * M, fb.begin() + (size_t)F * M);
    return sb;
}

// ---- kTrainW: the schedule of the wave-local contraction (FwdParams::wl_*) --------------------------------------------------------------
// A quad = 4 consecutive mel bands; its band =
// the bins where any of them is non-zero.  A block of the 4x4x1 MFMA walks one PIECE of a band, one bin per step; a phase
// holds 16 pieces and is as long as its longest, rounded up to 4 steps.  Whole quads are one piece.  Where a wave holds ONE
// frame (n_fft >= 2048: two of the four rows idle, phases 100-330 steps long) a wide quad is split over 2 or 4 blocks of one
// phase -- pieces of its band, B operands restricted to the piece -- and the partial sums are merged across lanes after the
// phase's loop (wl_merge: one or two rounds of ds_bpermute + add; the final piece's lanes carry the mel band).
QuadBands wl_quad_bands(const std::vector<float>& fb, int F, int M)
{
    const int Q = (M + 3) / 4;
    QuadBands qb;
    qb.first.assign(Q, 0); qb.width.assign(Q, 0);
    for (int q = 0; q < Q; ++q) {
        int lo = F, hi = -1;
        for (int f = 0; f < F; ++f)
            for (int j = 0; j < 4 && 4 * q + j < M; ++j)
                if (fb[(size_t)f * M + 4 * q + j] != 0.f) { lo = std::min(lo, f); hi = std::max(hi, f); }
        qb.first[q] = hi >= lo ? lo : 0; qb.width[q] = hi >= lo ? hi - lo + 1 : 0;
    }
    return qb;
}

// split factors: pieces no longer than w*, s in {1, 2, 4}; w* by exhaustive search over the step count of the resulting phases
int wl_group_quads(const QuadBands& qb, int wstar, bool may_split, WlPhases& phases)
{
    const std::vector<int>& first = qb.first, & width = qb.width;
    const int Q = (int)width.size();
    struct Grp { int quad, s, len; };
    std::vector<Grp> gs;
    for (int q = 0; q < Q; ++q) {
        int sp = 1;
        while (may_split && (width[q] + sp - 1) / sp > wstar && sp < 4) sp *= 2;
        gs.push_back({q, sp, (width[q] + sp - 1) / sp});
    }
    std::stable_sort(gs.begin(), gs.end(), [](const Grp& a, const Grp& b) { return a.len > b.len; });
    phases.clear();
    std::vector<int> used;
    int gid = 0;
    for (const Grp& g : gs) {
        size_t ph = 0;
        while (ph < phases.size() && used[ph] + g.s > 16) ++ph;
        if (ph == phases.size()) { phases.emplace_back(); used.push_back(0); }
        for (int i = 0; i < g.s; ++i) {
            const int lo = first[g.quad] + i * g.len;
            const int w = std::max(0, std::min(g.len, first[g.quad] + width[g.quad] - lo));
            phases[ph].push_back({g.quad, lo, w, gid, i, g.s});
        }
        used[ph] += g.s; ++gid;
    }
    if ((int)phases.size() > kWlMaxPhases) return 1 << 30;
    // cost in steps: the phases' lengths plus 40 per phase -- measured, not derived: config 3's three phases of 100 steps in all
    // run as long as its two phases of 136 (45.9-46.2 against 45.5-46.1 us, 40 more vector instructions per wave: kept whole),
    // config 5's three of 104 beat its two of 160 by 4 % (66.1-67.9 against 68.9-71.0 us); and -- decisively -- the staged epilogue
    // is lost beyond four phases (config 3 in five phases: 53.0 us)
    int total = 0;
    for (auto& ph : phases) { int wm = 0; for (auto& pc : ph) wm = std::max(wm, pc.w); total += std::max(4, (wm + 3) / 4 * 4) + 40 + (ph.size() && ph[0].s > 1 ? 2 : 0); }
    if ((int)phases.size() > 4) total += 1000;
    return total;
}

WlPhases wl_search_phases(const QuadBands& qb, bool may_split)
{
    WlPhases phases;
    int wmaxq = 4;
    for (int w : qb.width) wmaxq = std::max(wmaxq, w);
    int best = 1 << 30, best_w = wmaxq;
    if (may_split)
        for (int wstar = 4; wstar <= wmaxq; ++wstar) {
            WlPhases trial;
            const int t = wl_group_quads(qb, wstar, may_split, trial);
            if (t < best) { best = t; best_w = wstar; }
        }
    wl_group_quads(qb, best_w, may_split, phases);
    // (narrowest phase first, as before: the lane table and the first B groups of phase 0 are the ones requested early)
    std::reverse(phases.begin(), phases.end());
    return phases;
}

// Bank conflicts of the A operand reads (dmel_kernels.h, slot_stride_f2): the 8 blocks of each 32-lane group must sit
// at bins that differ modulo 8.  A block may start anywhere in [lo, hi] -- the piece must fit into the phase's L steps
// and the run must not pass bin F - 1 -- so each piece is matched to one of the 16 (group, residue) places it can
// reach (augmenting paths; 16 x 16); if that fails the phase gets four more steps.
WlPlacement wl_place_phase(const std::vector<WlPiece>& pcs, int F)
{
    const int nq = (int)pcs.size();
    int wmax = 0;
    for (int i = 0; i < nq; ++i) wmax = std::max(wmax, pcs[i].w);
    WlPlacement pm;
    int* slot_of = pm.slot_of, * k0_of = pm.k0_of;
    int L = std::max(4, (wmax + 3) / 4 * 4);
    for (;; L += 4) {
        int lo[16], hi[16], owner[16];
        for (int i = 0; i < nq; ++i) {
            hi[i] = std::max(0, std::min(pcs[i].lo, F - L));
            lo[i] = std::min(hi[i], std::max(0, pcs[i].lo + pcs[i].w - L));
        }
        auto can = [&](int i, int r) { for (int k = hi[i]; k >= lo[i] && k > hi[i] - 8; --k) if ((k & 7) == r) return true; return false; };
        std::fill(owner, owner + 16, -1);
        bool seen[16];
        std::function<bool(int)> place = [&](int i) -> bool {
            for (int sl = 0; sl < 16; ++sl) {
                if (seen[sl] || !can(i, sl & 7)) continue;
                seen[sl] = true;
                if (owner[sl] < 0 || place(owner[sl])) { owner[sl] = i; return true; }
            }
            return false;
        };
        bool ok = true;
        for (int i = 0; i < nq && ok; ++i) {               // longest (least freedom) first
            std::fill(seen, seen + 16, false);
            ok = place(i);
        }
        if (!ok && L < wmax + 64) continue;
        std::fill(slot_of, slot_of + 16, -1);
        if (ok) { for (int sl = 0; sl < 16; ++sl) if (owner[sl] >= 0) slot_of[owner[sl]] = sl; }
        else {                                        // (not reached with 16 places for 16 pieces: any residue has two)
            bool used[16] = {};
            for (int i = 0; i < nq; ++i) for (int sl = 0; sl < 16; ++sl) if (!used[sl]) { used[sl] = true; slot_of[i] = sl; break; }
        }
        for (int i = 0; i < nq; ++i) {
            k0_of[i] = hi[i];
            for (int k = hi[i]; k >= lo[i] && k > hi[i] - 8; --k) if ((k & 7) == (slot_of[i] & 7)) { k0_of[i] = k; break; }
        }
        break;
    }
    pm.L = wmax > 0 ? L : 0;
    return pm;
}

WlSchedule wl_fill(const std::vector<float>& fb, int F, int M, const WlPhases& phases)
{
    WlSchedule ws;
    ws.phases = (int)phases.size();
    std::vector<int2>& lanes = ws.lane;
    std::vector<int>& merge = ws.merge;
    std::vector<float4>& b4 = ws.b4;
    lanes.resize((size_t)ws.phases * 64);
    merge.assign((size_t)ws.phases * 64, 0);
    ws.total4 = 0;
    for (int ph = 0; ph < ws.phases; ++ph) {
        const std::vector<WlPiece>& pcs = phases[ph];
        const int nq = (int)pcs.size();
        const WlPlacement pm = wl_place_phase(pcs, F);
        const int n4 = pm.L / 4;
        ws.len4[ph] = n4;
        const size_t base = b4.size();
        b4.resize(base + (size_t)n4 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
        for (int sl = 0; sl < 16; ++sl)                  // places nobody took: no mel band, a bin of their residue
            for (int j = 0; j < 4; ++j) { lanes[(size_t)ph * 64 + 4 * sl + j] = make_int2(8 * (sl & 7), -1); merge[(size_t)ph * 64 + 4 * sl + j] = (4 * sl + j) | ((4 * sl + j) << 8); }
        int mg = 0;
        for (int i = 0; i < nq; ++i) {
            const WlPiece& pc = pcs[i];
            const int b = pm.slot_of[i], k0 = pm.k0_of[i];
            // the pieces of this piece's group in this phase (they were placed together), in the order of their index
            int blk[4] = {b, b, b, b};
            for (int i2 = 0; i2 < nq; ++i2) if (pcs[i2].group == pc.group) blk[pcs[i2].idx] = pm.slot_of[i2];
            // merge tree: round 1: piece 0 += piece 1, piece 2 += piece 3; round 2: piece 0 += piece 2; the result sits with piece 0
            int p1 = b, p2 = b, f1 = 0, f2 = 0;
            if (pc.s >= 2 && pc.idx == 0) { p1 = blk[1]; f1 = 1; }
            if (pc.s == 4 && pc.idx == 2) { p1 = blk[3]; f1 = 1; }
            if (pc.s == 4 && pc.idx == 0) { p2 = blk[2]; f2 = 1; }
            if (pc.s >= 2) mg |= 1;
            if (pc.s == 4) mg |= 2;
            const bool fin = pc.idx == 0;
            for (int j = 0; j < 4; ++j) {
                const int m = 4 * pc.quad + j;
                lanes[(size_t)ph * 64 + 4 * b + j] = make_int2(8 * k0, (fin && m < M) ? m : -1);
                merge[(size_t)ph * 64 + 4 * b + j] = (4 * p1 + j) | ((4 * p2 + j) << 8) | (f1 << 16) | (f2 << 17);
                if (m >= M) continue;
                for (int st = 0; st < 4 * n4; ++st) {
                    const int f = k0 + st;
                    const float v = (f < F && f >= pc.lo && f < pc.lo + pc.w) ? fb[(size_t)f * M + m] : 0.f;
                    float4& e = b4[base + (size_t)(st / 4) * 64 + 4 * b + j];
                    (st % 4 == 0 ? e.x : st % 4 == 1 ? e.y : st % 4 == 2 ? e.z : e.w) = v;
                }
            }
        }
        ws.mg[ph] = mg;
        ws.total4 += n4;
    }
    return ws;
}

WlSchedule build_wl_schedule(const std::vector<float>& fb, int F, int M, bool may_split)
{
    return wl_fill(fb, F, M, wl_search_phases(wl_quad_bands(fb, F, M), may_split));
}

// ---- every table of one n_fft ---------------------------------------------------------------------------------------------------------
bool build_host_tables(const std::vector<float>& fb, int N, int M, bool split_bank, bool allow_split, HostTables* out)
{
    HostTables& h = *out;
    const int F = N / 2 + 1;
    h.tw_long = build_long_twiddles(N);
    h.rows = build_row_tables(fb, F, M);
    const bool is_pow2 = (N & (N - 1)) == 0;
    if (N > kMaxFastNfft || !is_pow2) {
        h.tbank = build_transposed_bank(fb, F, M);
    } else if (N >= kMinFastNfft) {
        int r0 = 0, c0 = 0, r1 = 0, c1 = 0;
        if (!forward_plan_rc(N, false, &r0, &c0) || !forward_plan_rc(N, true, &r1, &c1)) return false;
        h.tw = build_plan_twiddles(N, r0, c0);
        h.twp_same = r0 == r1 && c0 == c1;
        if (!h.twp_same) h.twp = build_plan_twiddles(N, r1, c1);
        const int waves = forward_waves(N);
        h.bs = build_b_stream(fb, F, M, waves);
        h.pre = build_reg_prefix(h.bs, waves, forward_nbpre(N));
        if (split_bank && forward_has_hsplit(N)) h.h = build_split_bf16(fb, N, M);
        if (forward_has_wlc(N) && (M + 3) / 4 <= 16 * kWlMaxPhases) h.wl = build_wl_schedule(fb, F, M, allow_split && forward_wlc_one_frame(N));
    }
    return true;
}

// ---- the big path ---------------------------------------------------------------------------------------------------------------------
// in-place radix-2 FFT in double precision (host: the transform of Bluestein's chirp filter, once per DFT length)
void host_fft(std::vector<double>& re, std::vector<double>& im)
{
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        for (size_t s0 = 0; s0 < n; s0 += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double wr = std::cos(ang * (double)k), wi = std::sin(ang * (double)k);
                const size_t a = s0 + k, b = a + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr; im[b] = im[a] - ti;
                re[a] += tr; im[a] += ti;
            }
    }
}

int big_fft_length(int N)
{
    if ((N & (N - 1)) == 0) return N;
    int M = 1;
    while (M < 2 * N - 1) M <<= 1;
    return M;
}

// the phase of Bluestein's chirp at k: pi k^2 / N
static double chirp_phase(int k, int N)
{
    const long long q = ((long long)k * k) % (2LL * N);        // k^2 mod 2N: the phase argument stays small
    return M_PI * (double)q / (double)N;
}

std::vector<float2> build_chirp(int N)
{
    std::vector<float2> chirp(N);
    for (int k = 0; k < N; ++k) {
        const double a = chirp_phase(k, N);
        chirp[k] = make_float2((float)std::cos(a), (float)(-std::sin(a)));
    }
    return chirp;
}

std::vector<float2> build_chirp_filter(int N, int M)
{
    int logM = 0;
    while ((1 << logM) < M) ++logM;
    std::vector<double> hr(M, 0.0), hi(M, 0.0);
    for (int k = 0; k < N; ++k) {
        const double a = chirp_phase(k, N);
        hr[k] = std::cos(a); hi[k] = std::sin(a);
        if (k) { hr[M - k] = std::cos(a); hi[M - k] = std::sin(a); }
    }
    host_fft(hr, hi);
    std::vector<float2> hbr(M);
    for (int j = 0; j < M; ++j) {
        unsigned r = 0;
        for (int bbit = 0; bbit < logM; ++bbit) r |= ((unsigned)(j >> bbit) & 1u) << (logM - 1 - bbit);
        hbr[r] = make_float2((float)(hr[j] / M), (float)(hi[j] / M));     // position r of a DIF output holds bin brev(r) = j
    }
    return hbr;
}

}  // namespace dmel
