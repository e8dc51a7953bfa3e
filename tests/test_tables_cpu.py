"""The host tables (csrc/dmel_tables.cpp) without a GPU: tests/host/tables_dump.cpp, a stand-alone program with its own main that includes only
that unit, writes every table's bytes for a list of configurations.  Checked here:

  a. SHA-256 of every table and of the scalar fields, folded by name into one SHA-256 per configuration, equal profiles/r30_table_digests.json,
     which was recorded from the PARENT commit's build_tables / big_tables_for (NOTEBOOK R30 says how) -- the move changed no byte;
  b. the B-fragment stream, replayed through tile_ranges (own runs and pieces summed), is the bank: every non-zero entry exactly once;
  c. the wave-local schedule, replayed through wl_lane / wl_len4 / wl_b4 with a group's pieces summed as wl_merge routes them, is the bank,
     every non-zero entry exactly once, and block b of every phase starts at a bin with (k0 & 7) == (b & 7).

Nothing is loaded into Python."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "profiles", "r30_table_digests.json")

N_FFTS = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 1000, 20000, 32768]
N_MELS = [1, 8, 40, 64, 80, 128, 129, 257]
RATES = [(16000, 0.0, None), (44100, 50.0, 14000.0), (8000, 0.0, None)]      # (sample rate, f_min, f_max; None: the plan's default, sample_rate // 2)
SCALARS = (["F", "KS", "NT", "groups", "n_entries", "n_dense"] + [f"pre_groups{i}" for i in range(16)] +
           ["xch_groups", "ent_b_floats", "long_rows", "wl_phases", "wl_total4"] + [f"wl_len4_{i}" for i in range(8)] + [f"wl_mg{i}" for i in range(8)] +
           ["M", "logM", "waves"])


def configurations(full=False):
    """(name, n_fft, n_mels, sample_rate, f_min, f_max, kind).  full: the list the digests file was recorded over; the test runs it without the
    second and third sample rate of the sizes from 8192 on, whose tables -- two copies of the bank, no schedule -- are two thirds of the
    full list's 700 MB and made the file take 7 s instead of 4"""
    out = []
    for n in N_FFTS:
        for m in N_MELS:
            for r, (sr, f_min, f_max) in enumerate(RATES if full or n < 8192 else RATES[:1]):
                out.append((f"n{n}_m{m}_r{r}_htk", n, m, sr, f_min, float(sr // 2) if f_max is None else f_max, "htk"))
    # beyond 32 groups of mel tiles (FwdParams::xch_groups is a 32-bit mask): group 32 with seven tiles, and with one tile, which below group 32 would have a wave of its own
    out += [(f"n256_m{m}_r0_htk", 256, m, 16000, 0.0, 8000.0, "htk") for m in (4200, 4100)]
    for n in (64, 1024, 2048, 4096):
        for m in (64, 128):
            out += [(f"n{n}_m{m}_r0_{kind}", n, m, 16000, 0.0, 8000.0, kind) for kind in ("custom", "dense")]     # (HTK: above)
    return out


def config_text(cfgs):
    return "".join(f"{name} {n} {m} {sr} {f_min!r} {f_max!r} {kind}\n" for name, n, m, sr, f_min, f_max, kind in cfgs)


def read_records(path):
    """{table: bytes} of one file the dump program wrote"""
    buf = memoryview(open(path, "rb").read())
    out, at = {}, 0
    while at < len(buf):
        name = bytes(buf[at:at + 16]).rstrip(b"\0").decode()
        size = int.from_bytes(buf[at + 16:at + 24], "little")
        out[name] = buf[at + 24:at + 24 + size]
        at += 24 + size
    return out


def table_digests(records):
    return {k: hashlib.sha256(v).hexdigest() for k, v in records.items()}


def digest_of(records):
    """one SHA-256 per configuration over the SHA-256 of every table it has and of its scalar fields, by name: the digests file stays one short line per configuration"""
    return hashlib.sha256("".join(f"{k} {d}\n" for k, d in sorted(table_digests(records).items())).encode()).hexdigest()


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the dump program includes dmel_kernels.h, which needs HIP's vector types")
    tmp = tmp_path_factory.mktemp("tables")
    exe, cfg, out = str(tmp / "tables_dump"), str(tmp / "configs.txt"), tmp / "out"
    out.mkdir()
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "host", "tables_dump.cpp"), "-o", exe], check=True)
    cfgs = configurations()
    open(cfg, "w").write(config_text(cfgs))
    res = subprocess.run([exe, cfg, str(out)], capture_output=True, text=True)
    assert res.returncode == 0 and f"{len(cfgs)} configurations" in res.stdout, res.stdout + res.stderr
    return {c[0]: read_records(str(out / (c[0] + ".bin"))) for c in cfgs}


def test_every_table_has_the_parents_bytes(dumped):
    want = json.load(open(DIGESTS))
    assert sorted(want) == sorted(c[0] for c in configurations(full=True)) and set(dumped) <= set(want)
    bad = [(name, scalars(rec), table_digests(rec)) for name, rec in dumped.items() if digest_of(rec) != want[name]]
    assert not bad, (len(bad), bad[0])


def scalars(rec):
    return dict(zip(SCALARS, np.frombuffer(rec["scalars"], np.int32).tolist()))


def bank(rec):
    sc = scalars(rec)
    fb = np.frombuffer(rec["fb"], np.float32)
    return fb.reshape(sc["F"], fb.size // sc["F"])


def replay_b_stream(rec):
    """(sum, number of non-zero contributions) per (bin, mel) of the B-fragment stream, padded to whole 4 x 16 blocks (a run is whole groups of
    4 k-steps: it may pass the last k-step by up to three)"""
    sc = scalars(rec)
    ent_b = np.frombuffer(rec["ent_b"], np.float32) if "ent_b" in rec else np.zeros(0, np.float32)
    acc = np.zeros((4 * (sc["KS"] + 3), 16 * sc["NT"]), np.float32)
    cnt = np.zeros(acc.shape, np.int32)
    for ks_a, nks, off, w in np.frombuffer(rec["tile_ranges"], np.int32).reshape(-1, 4):
        if w == -1 or nks == 0:
            continue
        tile = int(w) & 0xffff
        blk = ent_b[off:off + nks * 64].reshape(nks * 4, 16)          # lane l of k-step ks: row 4 ks + (l >> 4), column 16 tile + (l & 15)
        acc[4 * ks_a:4 * (ks_a + nks), 16 * tile:16 * tile + 16] += blk
        cnt[4 * ks_a:4 * (ks_a + nks), 16 * tile:16 * tile + 16] += blk != 0
    return acc, cnt


def test_b_fragment_stream_reconstructs_the_bank(dumped):
    own_wave = pair_tiles = beyond_mask = 0
    n = 0
    for name, rec in dumped.items():
        if "tile_ranges" not in rec:
            continue
        n += 1
        sc, fb = scalars(rec), bank(rec)
        acc, cnt = replay_b_stream(rec)
        want = np.zeros(acc.shape, np.float32)
        want[:fb.shape[0], :fb.shape[1]] = fb
        assert np.array_equal(acc, want), name
        assert np.array_equal(cnt, (want != 0).astype(np.int32)), name
        assert sc["ent_b_floats"] * 4 == len(rec.get("ent_b", b"")), name
        if sc["waves"] == 4:                                             # which branch of the 4-wave plans each group of 8 tiles took
            for g in range(sc["groups"]):
                ntg = min(8, sc["NT"] - 8 * g)
                if ntg <= 4 and g < 32:
                    own_wave += 1
                else:
                    pair_tiles += 1
                    beyond_mask += ntg <= 4
            assert sc["xch_groups"] >> min(sc["groups"], 32) == 0, name
    assert n == (8 * len(RATES) + 2) * len(N_MELS) + 2 + 16, n           # every n_fft of the fused kernel
    assert own_wave and pair_tiles and beyond_mask, (own_wave, pair_tiles, beyond_mask)


def replay_wave_local(rec, n_bins):
    """per mel band: (sum, number of non-zero contributions) over the bins, as the lanes that carry the band end up with after the merge
    rounds; and the (phase, block, first bin, lane word) of every block"""
    sc = scalars(rec)
    lane = np.frombuffer(rec["wl_lane"], np.int32).reshape(-1, 64, 2)
    merge = np.frombuffer(rec["wl_merge"], np.int32).reshape(-1, 64)
    b4 = np.frombuffer(rec["wl_b4"], np.float32).reshape(-1, 64, 4) if "wl_b4" in rec else np.zeros((0, 64, 4), np.float32)
    assert lane.shape[0] == sc["wl_phases"] and b4.shape[0] == sc["wl_total4"]
    bands, blocks, base = {}, [], 0
    for ph in range(sc["wl_phases"]):
        n4 = sc[f"wl_len4_{ph}"]
        coef = b4[base:base + n4].transpose(1, 0, 2).reshape(64, 4 * n4)            # [lane][step]
        base += n4
        val = np.zeros((64, n_bins + 4 * n4 + 8), np.float32)
        for i in range(64):
            k0 = lane[ph, i, 0] // 8
            val[i, k0:k0 + 4 * n4] = coef[i]
            if i % 4 == 0:
                blocks.append((ph, i // 4, int(k0), int(lane[ph, i, 0])))
        cnt = (val != 0).astype(np.int32)
        p1, p2, f1, f2 = merge[ph] & 0xff, (merge[ph] >> 8) & 0xff, (merge[ph] >> 16) & 1, (merge[ph] >> 17) & 1
        assert bool(f1.any()) == bool(sc[f"wl_mg{ph}"] & 1) and bool(f2.any()) == bool(sc[f"wl_mg{ph}"] & 2)
        for partner, recv in ((p1, f1), (p2, f2)):                                    # a round: every receiving lane adds its partner's sum
            val = val + np.where(recv[:, None] == 1, val[partner], 0)
            cnt = cnt + np.where(recv[:, None] == 1, cnt[partner], 0)
        for i in range(64):
            m = int(lane[ph, i, 1])
            if m >= 0:
                assert m not in bands, m
                bands[m] = (val[i], cnt[i])
    return bands, blocks


def test_wave_local_schedule_reconstructs_the_bank_on_conflict_free_bins(dumped):
    n = n_blocks = 0
    for name, rec in dumped.items():
        if "wl_lane" not in rec:
            continue
        n += 1
        fb = bank(rec)
        F, M = fb.shape
        bands, blocks = replay_wave_local(rec, F)
        assert sorted(bands) == list(range(M)), name
        for m, (val, cnt) in bands.items():
            assert np.array_equal(val[:F], fb[:, m]) and not val[F:].any(), (name, m)
            assert np.array_equal(cnt[:F], (fb[:, m] != 0).astype(np.int32)), (name, m)
        for ph, b, k0, word in blocks:
            assert word % 8 == 0, (name, ph, b, word)
            # Finding on the parent's tables (NOTEBOOK R30): the rule holds in every phase of every HTK bank.  A caller's or the dense bank's
            # quads span all the bins, so a block can only start at bin 0: the placement fails, pays its 64 extra steps per phase and leaves all
            # blocks on bin 0.  No table is changed for it here; what those banks do satisfy is asserted
            assert (k0 & 7) == (b & 7) or (not name.endswith("_htk") and k0 == 0), (name, ph, b, k0)
        n_blocks += len(blocks)
    assert n >= 2 * len(N_MELS) * len(RATES) + 2 * 4, n                  # n_fft 1024 and 2048 at the least, and their custom and dense banks
    assert n_blocks >= 16 * n
