"""CPU-side checks of the C-ABI library: it loads without a GPU, exports every symbol of include/dmel.h,
its host-side functions agree with the oracle, and device entry points fail loudly without a device."""
import os
import re

import numpy as np
import pytest

import cases as C
from oracle import dmel_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from dmel_amd import capi
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)          # strip comments
    declared = sorted(set(re.findall(r"\b(dmel_[a-z_0-9]+)\s*\(", code)))
    assert declared, "no declarations found"
    assert sorted(capi.SYMBOLS) == declared
    for name in declared:
        assert hasattr(L, name), f"libdmel_hip.so does not export {name}"
    assert L.dmel_abi_version() == 5


def test_signature_table_has_the_headers_parameter_counts():
    """capi's one table name -> (restype, argtypes) against include/dmel.h: an entry for every declared function with as many argtypes
    as the declaration has parameters ((void) is none), and after load() every symbol carries them -- an entry point without argtypes
    would receive its pointers as C int."""
    from dmel_amd import capi
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "dmel.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    decls = re.findall(r"\b(dmel_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", code)
    assert sorted(n for n, _ in decls) == sorted(capi.SYMBOLS)
    for name, params in decls:
        count = 0 if params.strip() == "void" else params.count(",") + 1
        restype, argtypes = capi._SIGNATURES[name]
        assert len(argtypes) == count, (name, count, argtypes)
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name


def test_n_fft_rule_matches_oracle_and_fixtures():
    from dmel_amd import capi
    for case in C.CASES:
        if case["optimized"]:
            assert capi.n_fft(case["lambd"]) == int(C.load(case)["n_fft"]) == O.n_fft(case["lambd"])
    rng = np.random.default_rng(0)
    for lam in np.concatenate([rng.uniform(0, 700, 500), [0.0, 1 / 6, 1 / 3, 0.5, 85.33333, 85.5, 682.6, 682.7]]):
        assert capi.n_fft(float(lam)) == O.n_fft(float(lam))
        assert capi.n_fft(-float(lam)) == O.n_fft(float(lam))


@pytest.mark.parametrize("F,M,sr,fmin,fmax", [(257, 64, 16000, 0, 8000), (513, 128, 16000, 0, 8000), (1025, 128, 16000, 0, 8000),
                                             (1025, 128, 44100, 0, 22050), (65, 64, 8000, 0, 4000), (2049, 64, 8000, 0, 4000),
                                             (129, 40, 16000, 125.0, 7000.0)])
def test_filterbank_tables(F, M, sr, fmin, fmax):
    """SURVEY.md 8(c) G8 table shapes.  torchaudio is absent, so these are formula-vs-formula (parity unpinned):
    the product's C++ table against the oracle's C table, plus the structural properties of an HTK bank."""
    from dmel_amd import capi
    fb = capi.mel_fbanks_host(F, fmin, fmax, M, sr)
    assert np.array_equal(fb, O.mel_fbanks(F, fmin, fmax, M, sr))
    assert fb.min() >= 0.0 and fb.max() <= 1.0
    assert ((fb > 0).sum(axis=1) <= 2).all()            # triangles overlap pairwise only
    nz = [np.flatnonzero(fb[:, m]) for m in range(M)]
    assert all(len(i) == 0 or (np.diff(i) == 1).all() for i in nz)   # each band is one contiguous run


def test_window_host_matches_oracle():
    from dmel_amd import capi
    for lam, n, norm in ((64.0, 512, False), (128.0, 1024, True), (13.3333, 128, False), (400.0, 4096, True)):
        w, dw = capi.window_host(lam, n, norm)
        wo, dwo = O.window(lam, n, norm)
        assert np.array_equal(w, wo)
        assert np.abs(dw - dwo).max() <= 1e-6 * np.abs(dwo).max()


def test_no_device_fails_loudly():
    import torch
    from dmel_amd import MelSpectrogramLayer, capi
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert capi.device_count() == 0
    with pytest.raises(capi.DmelError):
        capi.Plan(16000, 256, 64, 16000)
    layer = MelSpectrogramLayer(torch.tensor(64.0), 64, 16000, 16000, hop_length=256, optimized=True)
    assert list(layer.state_dict().keys()) == ["lambd"]
    with pytest.raises(RuntimeError):
        layer(torch.zeros(1, 16000))          # CPU tensor: there is no CPU fallback


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "differentiable-mel-spectrogram_amd")
    for dirpath, _, files in os.walk(pkg):
        if "build" in dirpath.split(os.sep):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "dmel_oracle" not in text and "import oracle" not in text and "from oracle" not in text, f


@pytest.mark.parametrize("F,M,sr,fmin,fmax", [(257, 64, 16000, 0, 8000), (513, 128, 16000, 0, 8000), (1025, 128, 16000, 0, 8000),
                                             (1025, 128, 44100, 0, 22050), (2049, 64, 8000, 0, 4000), (129, 40, 16000, 125.0, 7000.0)])
def test_filterbank_against_independent_implementation(F, M, sr, fmin, fmax):
    """torchaudio is absent, but Hugging Face transformers ships an independent HTK triangular filterbank
    (audio_utils.mel_filter_bank, documented as equivalent to torchaudio's melscale_fbanks for norm=None,
    mel_scale='htk'); it works in fp64 where torchaudio works in fp32, hence the 5e-5 band (measured: <= 1.4e-5)."""
    import warnings
    au = pytest.importorskip("transformers.audio_utils")
    from dmel_amd import capi
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = au.mel_filter_bank(F, M, fmin, fmax, sr, norm=None, mel_scale="htk")
    fb = capi.mel_fbanks_host(F, fmin, fmax, M, sr)
    assert ref.shape == fb.shape
    assert float(np.abs(ref - fb).max()) <= 5e-5
    # same support, up to entries that are zero in one and <= 5e-5 in the other
    assert ((ref > 5e-5) <= (fb > 0)).all() and ((fb > 5e-5) <= (ref > 0)).all()


def test_filterbank_tables_g8():
    """the filterbank tables for the survey's six (n_freqs, n_mels, sample_rate).  tests/golden/g8_fbanks.npz was written
    by the stand-in for torchaudio's melscale_fbanks (its `source` entry says which: torchaudio is absent from this image -- row a6 stays
    unpinned until tests/golden/make_g8_fbanks.py has been run where torchaudio exists); the host builder of the product and the oracle
    must reproduce the tables: same support, values within 6e-6.  Round 6 brought both to torch's own fp32 evaluation -- the correctly
    rounded 10 ** x (libm's powf is an ulp off at a tenth of the mel points) and the fused multiply-add inside torch.linspace -- and four of
    the six tables are now BIT-IDENTICAL to the torch evaluation (they were 5e-6 ... 1.5e-5 off); the other two differ by <= 4.9e-6 in a few
    entries: torch.linspace's vectorised kernel rounds its chunk bases by the CPU's vector width (AVX2 / AVX-512 builds differ among themselves)."""
    from dmel_amd import capi
    from oracle import dmel_oracle as O
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_fbanks.npz"))
    assert "source" in gold.files
    keys = [k for k in gold.files if k.startswith("fb_")]
    assert len(keys) == 6
    for k in keys:
        F, M, sr = (int(v) for v in k.split("_")[1:])
        ref = gold[k]
        assert ref.shape == (F, M)
        for name, fb in (("capi", capi.mel_fbanks_host(F, 0.0, float(sr // 2), M, sr)), ("oracle", O.mel_fbanks(F, 0.0, float(sr // 2), M, sr))):
            assert float(np.abs(fb - ref).max()) <= 6e-6, (k, name, float(np.abs(fb - ref).max()))
            assert ((ref > 6e-6) <= (fb > 0)).all() and ((fb > 6e-6) <= (ref > 0)).all(), (k, name)
    exact = sum(bool(np.array_equal(capi.mel_fbanks_host(*[int(v) for v in k.split("_")[1:2]], 0.0, float(int(k.split("_")[3]) // 2), int(k.split("_")[2]), int(k.split("_")[3])), gold[k])) for k in keys)
    assert exact >= 4, exact


def test_every_exported_symbol_is_named_in_integration_md():
    """INTEGRATION.md shows a maintainer what each entry point replaces in the reference: none may be missing from it"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dmel.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    names = sorted(set(re.findall(r"^(?:dmel_status|int32_t|size_t|const char\*)\s+(dmel_[a-z0-9_]+)\s*\(", header, flags=re.M)))
    assert len(names) > 50
    # `dmel_comm_unique_id / create / ...` style lists name a family by prefix + suffixes
    def named(n):
        if n in doc:
            return True
        for fam in ("dmel_comm_", "dmel_mailbox_", "dmel_plan_"):
            if n.startswith(fam) and fam in doc and re.search(r"[/ ]" + re.escape(n[len(fam):]) + r"\b", doc):
                return True
        return False
    missing = [n for n in names if not named(n)]
    assert not missing, missing


def test_argument_checks_of_the_round_four_entry_points_need_no_device():
    """every new entry point refuses NULL handles / pointers with DMEL_ERR_INVALID_ARGUMENT before it touches a device, and the
    registry look-up never dereferences what it is given"""
    import ctypes as ct
    from dmel_amd import capi
    L = capi.load()
    null = ct.c_void_p(None)
    INVALID = capi.DMEL_ERR_INVALID_ARGUMENT if hasattr(capi, "DMEL_ERR_INVALID_ARGUMENT") else 1
    assert L.dmel_plan_is_live(null) == 0
    assert L.dmel_plan_is_live(ct.c_void_p(0x1234)) == 0                     # not a plan: a look-up, no dereference
    assert L.dmel_lambd_ring_size() >= 64
    assert L.dmel_plan_retain(ct.c_void_p(0x1234)) == INVALID               # retain checks the registry too
    assert L.dmel_spectrogram_ex_dev(null, null, 1, null, 256, 1, null, null, null) == INVALID
    assert L.dmel_backward_x_dev(null, null, 1, null, 1024, 0, null, null, null, null) == INVALID
    assert L.dmel_backward_x_spec_dev(null, null, 1, null, 256, 1, null, null, null) == INVALID
    assert L.dmel_forward_dev_fixed_spec(null, null, 1, null, 1024, 0, ct.c_double(1e-10), null, null, null, null, null) == INVALID
    assert L.dmel_backward_fb_saved(null, null, 1, 1024, 0, null, null, null, null) == INVALID
    assert L.dmel_backward_fb_saved_dl(null, null, 1, 1024, 0, null, null, null, null, null, null, null) == INVALID
    assert L.dmel_mailbox_set_timeout_ms(null, ct.c_uint64(1000)) == INVALID
    assert L.dmel_mailbox_set_spin_limit(null, 10) == INVALID
    assert b"NULL" in L.dmel_last_error() or b"null" in L.dmel_last_error().lower()
    # Adam's argument ranges are torch.optim.Adam's (a negative lr was accepted)
    one = ct.c_void_p(16)       # never dereferenced: the range check comes first
    assert L.dmel_adam_step(one, one, one, one, one, None, 1, ct.c_double(-1e-3), ct.c_double(0.9), ct.c_double(0.999), ct.c_double(1e-8),
                            ct.c_double(0.0), 0, None) == INVALID
    assert L.dmel_adam_step(one, one, one, one, one, None, 1, ct.c_double(1e-3), ct.c_double(0.9), ct.c_double(0.999), ct.c_double(1e-8),
                            ct.c_double(-0.1), 0, None) == INVALID


def test_contraction_partition_covers_every_tile_once_and_balances():
    """dmel_contraction_partition_host (what build_tables uses for the 8-wave plans and for 4-wave plans with up to four tiles): every
    unit of every tile is taken exactly once, pieces are contiguous behind the owner's share, a wave carries at most one piece and
    never one of its own tile, and the slowest wave is no slower than with round 3's split in halves (wave t and 7 - t)"""
    import random
    from dmel_amd import capi
    rng = random.Random(5)
    cases = [([2, 2, 3, 4, 4, 6, 8, 10], 8), ([15, 24, 38, 59], 8), ([2, 2, 4, 5, 8, 11, 16, 25], 8), ([2, 4, 5, 8], 4), ([33] * 8, 8), ([33] * 4, 8),
             ([0, 0, 7], 8), ([1], 8), ([], 8), ([5], 4), ([40, 1, 1, 1], 4)]
    for _ in range(300):
        w = rng.choice([4, 8])
        n = rng.randint(0, w)
        cases.append(([rng.choice([0, 1, 2, 3, 5, 8, 13, 40, 100]) if rng.random() < 0.5 else rng.randint(0, 60) for _ in range(n)], w))
    for units, waves in cases:
        own, pieces = capi.contraction_partition(units, waves)
        load = [own[w] for w in range(waves)]
        taken = [own[t] if t < len(units) else 0 for t in range(waves)]
        helpers = set()
        nxt = {t: own[t] for t in range(len(units))}
        for (w, t, a, n) in pieces:
            assert 0 <= w < waves and 0 <= t < len(units) and w != t and n > 0, (units, waves, pieces)
            assert w not in helpers, (units, pieces)                       # one piece per wave
            helpers.add(w)
            assert a == nxt[t], (units, pieces)                           # contiguous, in order
            nxt[t] += n
            taken[t] += n
            load[w] += n
        for t, u in enumerate(units):
            assert taken[t] == u and 0 <= own[t] <= u and (own[t] > 0 or u == 0), (units, waves, own, pieces)
        assert all(own[w] == 0 for w in range(len(units), waves))
        total = sum(units)
        if total:
            assert max(load) <= max(units), (units, load)
            if waves == 8:
                old = [0] * 8
                for t, u in enumerate(units):
                    h = (u + 1) // 2
                    old[t] += h
                    old[7 - t] += u - h
                assert max(load) <= max(old), (units, load, old)
