// tables_dump.cpp -- stand-alone: every host table of csrc/dmel_tables.cpp for a list of configurations, written as bytes.  No device, no
// HIP runtime call, no other unit of the library: tests/test_tables_cpu.py builds and runs it and hashes what it wrote.
//
//   tables_dump CONFIGS OUTDIR
//
// CONFIGS: one configuration per line, "name n_fft n_mels sample_rate f_min f_max kind", kind = htk | custom | dense (the three banks
// build_tables chooses between: HTK, a caller's bank -- here a seeded one with all-zero rows and columns --, the dense-device structure).
// OUTDIR/name.bin: records of [16 bytes name, zero padded][8 bytes length][bytes]: the bytes the host wrote of every table the
// configuration has (not the allocation's padding), the bank itself ("fb") and "scalars", int32 in the order of kScalars below.
#include "../../differentiable-mel-spectrogram_amd/csrc/dmel_tables.cpp"

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

namespace {

// F KS NT groups n_entries n_dense pre_groups[16] xch_groups ent_b_floats long_rows wl_phases wl_total4 wl_len4[8] wl_mg[8] M logM waves
constexpr int kScalars = 6 + 16 + 5 + 2 * dmel::kWlMaxPhases + 3;

struct Out {
    FILE* f;
    template <class T> void rec(const char* name, const std::vector<T>& v)
    {
        if (v.empty()) return;
        char nm[16] = {};
        std::snprintf(nm, sizeof nm, "%s", name);
        const uint64_t n = v.size() * sizeof(T);
        std::fwrite(nm, 1, 16, f); std::fwrite(&n, 8, 1, f); std::fwrite(v.data(), 1, n, f);
    }
};

// the caller's bank of a "custom" configuration: uniform in [0, 1) from a 64-bit LCG, a quarter of the entries, every seventh row and every fifth column zero
std::vector<float> seeded_bank(int F, int M, uint64_t seed)
{
    std::vector<float> fb((size_t)F * M);
    uint64_t s = seed;
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < M; ++m) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const float v = (float)(s >> 40) / 16777216.0f;
            fb[(size_t)f * M + m] = (f % 7 == 3 || m % 5 == 2 || v < 0.25f) ? 0.f : v;
        }
    return fb;
}

bool dump(const std::string& dir, const std::string& name, int N, int M, int sr, double f_min, double f_max, const std::string& kind)
{
    const int F = N / 2 + 1;
    std::vector<float> fb((size_t)F * M);
    if (kind == "dense") std::fill(fb.begin(), fb.end(), 1.0f);
    else if (kind == "custom") fb = seeded_bank(F, M, (uint64_t)N * 1000 + M);
    else dmel::mel_fbanks_htk(F, f_min, f_max, M, sr, fb.data());
    dmel::HostTables h;
    if (!dmel::build_host_tables(fb, N, M, kind != "htk", kind != "dense", &h)) return false;
    FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    if (!f) return false;
    Out o{f};
    o.rec("fb", fb);
    o.rec("tw_long", h.tw_long); o.rec("rowband", h.rows.rowband); o.rec("rowpk", h.rows.rowpk);
    o.rec("fbT", h.tbank.fbT); o.rec("band", h.tbank.band);
    o.rec("tw1", h.tw.tw1); o.rec("tw2", h.tw.tw2); o.rec("tw1p", h.twp.tw1); o.rec("tw2p", h.twp.tw2);
    o.rec("ent_b", h.bs.ent_b); o.rec("tile_ranges", h.bs.tile_ranges); o.rec("ent_pre", h.pre.ent_pre);
    o.rec("ent_h", h.h.ent_h); o.rec("fb_nyq", h.h.fb_nyq);
    o.rec("wl_lane", h.wl.lane); o.rec("wl_merge", h.wl.merge); o.rec("wl_b4", h.wl.b4);
    int bigM = 0, logM = 0;
    if (N > dmel::kMaxFastNfft || (N & (N - 1)) != 0) {        // the big path's tables
        bigM = dmel::big_fft_length(N);
        while ((1 << logM) < bigM) ++logM;
        o.rec("big_tw", dmel::build_long_twiddles(bigM));
        if (bigM != N) { o.rec("chirp", dmel::build_chirp(N)); o.rec("hbr", dmel::build_chirp_filter(N, bigM)); }
    }
    std::vector<int32_t> sc = {F, h.bs.KS, h.bs.NT, h.bs.groups, h.bs.n_entries, h.bs.n_dense};
    sc.insert(sc.end(), h.pre.pre_groups, h.pre.pre_groups + 16);
    sc.insert(sc.end(), {(int32_t)h.bs.xch_groups, (int32_t)h.bs.ent_b.size(), (int32_t)h.rows.long_rows, h.wl.phases, h.wl.total4});
    sc.insert(sc.end(), h.wl.len4, h.wl.len4 + dmel::kWlMaxPhases);
    sc.insert(sc.end(), h.wl.mg, h.wl.mg + dmel::kWlMaxPhases);
    sc.insert(sc.end(), {bigM, logM, h.bs.tile_ranges.empty() ? 0 : dmel::forward_waves(N)});
    if ((int)sc.size() != kScalars) return false;
    o.rec("scalars", sc);
    return std::fclose(f) == 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: tables_dump CONFIGS OUTDIR\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string name, kind;
        int N, M, sr;
        double f_min, f_max;
        if (!(ls >> name >> N >> M >> sr >> f_min >> f_max >> kind)) continue;
        if (!dump(argv[2], name, N, M, sr, f_min, f_max, kind)) { std::fprintf(stderr, "tables_dump: %s failed\n", name.c_str()); return 1; }
        ++n;
    }
    std::printf("%d configurations\n", n);
    return 0;
}
