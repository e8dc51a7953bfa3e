// dmel_tables.h -- the host arithmetic behind every table the kernels read: pure builders that return std::vectors and plain structs.
//
// No HIP runtime call: only the vector types and the constexpr geometry of dmel_kernels.h, so a program without kernels and without a
// device links this unit alone (tests/host/tables_dump.cpp records every table's bytes on the CPU).  dmel_api.cpp chooses the bank, calls
// the builders and uploads what they return.  Facts of the plan or the environment (may_split) arrive as arguments.  The six geometry
// queries the builders need -- forward_plan_rc, _waves, _nbpre, _has_hsplit, _has_wlc, _wlc_one_frame (dmel_kernels.h) -- are defined here too.
#pragma once
#include "dmel_kernels.h"

#include <vector>

namespace dmel {

// ---- the HTK bank ---------------------------------------------------------------------------------------------------------------------
void linspace_f32(float start, float end, int steps, std::vector<float>& out);      // torch.linspace (fp32, CPU)
void mel_fbanks_htk(int n_freqs, double f_min, double f_max, int n_mels, int sample_rate, float* fb);    // (n_freqs, n_mels): models.py:42-48

// ---- tables of every n_fft: fb is the (F, M) bank, F = n_fft / 2 + 1 --------------------------------------------------------------------
struct RowTables {
    std::vector<int2> rowband;     // (F): non-zero column range of every filterbank row (dL/dx)
    std::vector<float4> rowpk;     // (F): (first two non-zero coefficients, first column, columns) of every row (dL/dx, wave-FFT kernel)
    bool long_rows = false;        // some row has more than two columns
};
RowTables build_row_tables(const std::vector<float>& fb, int F, int M);

struct TransposedBank { std::vector<float> fbT; std::vector<int2> band; };       // long transforms: (M, F) transposed bank, (M) bands
TransposedBank build_transposed_bank(const std::vector<float>& fb, int F, int M);

std::vector<float2> build_long_twiddles(int N);       // (N / 2) twiddles exp(-2 pi i k / N)

struct PlanTwiddles { std::vector<float2> tw1, tw2; };
PlanTwiddles build_plan_twiddles(int N, int R, int C);    // of a plan (R, C): tw1 (R, G) = w_N^(lg q), tw2 (R, C) = w_G^(r p1)

// ---- the MFMA B-fragment stream of the fused kernel ------------------------------------------------------------------------------------
struct Piece { int wave, tile, a, n; };
void deal_ksteps(const int* units, int ntg, int W, int* own, std::vector<Piece>* pieces);

struct BStream {
    int KS = 0, NT = 0, groups = 0, n_entries = 0, n_dense = 0;
    std::vector<float> ent_b;
    std::vector<int4> tile_ranges;
    unsigned xch_groups = 0;       // FwdParams::xch_groups
};
BStream build_b_stream(const std::vector<float>& fb, int F, int M, int waves);

struct RegPrefix {
    std::vector<float> ent_pre;
    int pre_groups[16] = {};       // per (wave, run) of group 0: real groups of 4 k-steps inside ent_pre
};
RegPrefix build_reg_prefix(const BStream& bs, int waves, int nbpre);

struct SplitBf16 {
    std::vector<unsigned short> ent_h;     // B fragments of the split-bf16 contraction (FwdParams::ent_h)
    std::vector<float> fb_nyq;             // the row of bin n_fft / 2 (n_mels)
};
SplitBf16 build_split_bf16(const std::vector<float>& fb, int N, int M);

// ---- kTrainW: the schedule of the wave-local contraction (FwdParams::wl_*) --------------------------------------------------------------
struct QuadBands { std::vector<int> first, width; };       // per quad of 4 consecutive mel bands: the bins where any of them is non-zero
QuadBands wl_quad_bands(const std::vector<float>& fb, int F, int M);

struct WlPiece { int quad, lo, w, group, idx, s; };        // bins [lo, lo + w) of a quad's band: piece idx of the s its group has
typedef std::vector<std::vector<WlPiece>> WlPhases;
int wl_group_quads(const QuadBands& qb, int wstar, bool may_split, WlPhases& phases);     // pieces no longer than wstar; returns the cost in steps
WlPhases wl_search_phases(const QuadBands& qb, bool may_split);                           // the cheapest wstar's phases, narrowest first

struct WlPlacement { int L = 0, slot_of[16] = {}, k0_of[16] = {}; };      // steps of the phase; per piece: its block, its first bin
WlPlacement wl_place_phase(const std::vector<WlPiece>& pcs, int F);

struct WlSchedule {
    std::vector<float4> b4;        // B operands
    std::vector<int2> lane;        // lane table
    std::vector<int> merge;        // [phase * 64 + lane]: partner lane of merge round 1 | round 2 << 8 | receives in round 1 << 16 | in round 2 << 17
    int phases = 0, total4 = 0;
    int len4[kWlMaxPhases] = {};
    int mg[kWlMaxPhases] = {};     // per phase: bit 0 / 1 = merge round 1 / 2 is needed
};
WlSchedule wl_fill(const std::vector<float>& fb, int F, int M, const WlPhases& phases);
WlSchedule build_wl_schedule(const std::vector<float>& fb, int F, int M, bool may_split);

// ---- every table of one n_fft, chosen as build_tables uploads them: a vector left empty is a table this n_fft does not have -----------------
struct HostTables {
    std::vector<float2> tw_long;
    RowTables rows;
    TransposedBank tbank;          // n_fft beyond the fused kernel or not a power of two
    PlanTwiddles tw, twp;          // the fused kernel's sizes: twiddles of the plan of the training modes and of the modes that pack two frames
    bool twp_same = false;         // ... per FFT, where that plan differs (else twp stays empty)
    BStream bs;
    RegPrefix pre;
    SplitBf16 h;                   // split_bank, n_fft 64 .. 4096
    WlSchedule wl;                 // the sizes kTrainW is built for, up to 16 kWlMaxPhases quads
};
// split_bank: the bank is the caller's (custom or dense-device) and gets the split-bf16 fragments; allow_split: the wave-local schedule may
// split wide quads where a wave holds one frame.  false: a power of two inside the fused kernel's range has no FFT plan
bool build_host_tables(const std::vector<float>& fb, int N, int M, bool split_bank, bool allow_split, HostTables* out);

// ---- the big path (dmel_big.hip) --------------------------------------------------------------------------------------------------------
void host_fft(std::vector<double>& re, std::vector<double>& im);
int big_fft_length(int N);                               // the power-of-two FFT behind DFT length N: N itself, or >= 2 N - 1 (Bluestein)
std::vector<float2> build_chirp(int N);                  // c[n] = exp(-i pi n^2 / N)
std::vector<float2> build_chirp_filter(int N, int M);    // the transform of the chirp's filter over M points, / M, in the order a DIF output has

}  // namespace dmel
