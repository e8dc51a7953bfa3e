"""Seeded random geometries for the two K-window layers (MultiWindowMelSpectrogram, BandSplitMelSpectrogram): what
tests/test_hip_kwindow_random.py runs on the GPU and tests/test_kwindow_cases_cpu.py holds to its claims without one.  Plain numpy.

A case is a tests/golden/cases.py-style dict (C.make_input, C.make_cotangent and C.out_shape work on it; ``lambd`` is ``lams[0]``) plus
  lams          K window widths, K in 1 ... 8, each log-uniform over the n_fft 32 ... 16384 the layers serve, one in five negative;
                with probability 0.4 two channels are forced onto the same n_fft (one launch for both), with probability 0.2 two hold
                ``x`` and ``1.002 x`` on either side of an n_fft boundary (6 x just below n_fft + 1: time_frequency.py:39 truncates)
  L, hop, B     rows from max(8, n_min // 4) samples to a few times n_max (rows shorter than a channel's n_fft occur), hop as
                test_hip_random_shapes._random_cases draws it with T capped at 300, B in 1 ... 4; exactly two cases of every call have
                rows of 32769 ... 40000 samples (the prep kernel's partial sums), with hop >= 400 and B = 2
  sr, n_mels, f_min, f_max, normalize_window   the scalar sweep's values
  edges, edges_default    the band layer's K_band + 1 edges, K_band = min(K, n_mels) (it takes ``lams[:K_band]``): the default even split
                (``edges_default``: the layer is built with band_edges=None) or random strictly increasing edges with a one-row group
                (K_band = 1 has one group of all rows: the default)
  lens          B clip lengths in 1 ... L.  Classes: "edge" {1, hop - 1, hop, hop + 1}; "full" L itself; "last_tile" a length short of
                L that ends within the last two frames (inside the last tile for every frames-per-tile the kernels use, or the whole
                of a last tile of one frame); for L > 32768 "above" and "below" 32768.  A case holds one value of each class its B clips
                have room for (a value may serve two classes: the long rows hold L or a last-tile length above, an edge value below);
                with fewer clips than classes the classes are taken in a shuffled order
Cost cap: B K T max n_fft <= ``cost_cap`` (redrawn otherwise), which keeps the fp64 oracle of a case in seconds."""
import numpy as np

import cases as C

NFFTS = [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
SRS = [8000, 16000, 22050, 44100]
N_MELS = [1, 7, 16, 40, 64, 80, 128, 130]
F_MINS = [0.0, 50.0, 300.0]
LENGTH_CLASSES = ["edge", "full", "last_tile", "above", "below"]


def n_fft(lam):
    """next_pow2(int(6 |lambd|)) with the product in fp32 (time_frequency.py:39,61; tests/test_kwindow_cases_cpu.py holds it to the oracle's)"""
    v = int(np.float32(abs(np.float32(lam))) * np.float32(6.0))
    return 1 << max(v - 1, 0).bit_length()


def straddles(lams):
    """the channel pairs (i, j) that hold x and 1.002 x with different n_fft"""
    out = []
    for i, a in enumerate(lams):
        for j, b in enumerate(lams):
            if i != j and a * b > 0 and abs(abs(b) / abs(a) - 1.002) <= 1e-9 and n_fft(a) != n_fft(b):
                out.append((i, j))
    return out


def shared_n_fft(lams):
    ns = [n_fft(v) for v in lams]
    return len(set(ns)) < len(ns)


def launches(lams):
    """{n_fft: channel mask}: the launches a forward of these channels needs"""
    out = {}
    for k, v in enumerate(lams):
        out[n_fft(v)] = out.get(n_fft(v), 0) | (1 << k)
    return out


def length_classes(case, lb):
    """the classes (see the module's docstring) a clip length belongs to"""
    L, hop = case["L"], case["hop"]
    T = L // hop + 1
    out = set()
    if lb in (1, hop - 1, hop, hop + 1):
        out.add("edge")
    if lb == L:
        out.add("full")
    if max(1, (T - 2) * hop) <= lb < L:
        out.add("last_tile")
    if L > 32768:
        out.add("above" if lb > 32768 else "below")
    return out


def _draw_lam(rng, nft=None):
    nft = int(2 ** rng.integers(5, 15)) if nft is None else nft            # 32 ... 16384
    return float(rng.uniform(0.55, 0.99) * nft / 6.0) * (1.0 if rng.random() < 0.8 else -1.0)


def _draw_lams(rng):
    K = int(rng.integers(1, 9))
    lams = [_draw_lam(rng) for _ in range(K)]
    if K >= 2 and rng.random() < 0.4:                                      # two channels, one n_fft
        i, j = (int(v) for v in rng.choice(K, 2, replace=False))
        lams[j] = _draw_lam(rng, n_fft(lams[i]))
    if K >= 2 and rng.random() < 0.2:                                      # x and 1.002 x around a boundary: n_fft below, 2 n_fft above
        i, j = (int(v) for v in rng.choice(K, 2, replace=False))
        nft = int(2 ** rng.integers(5, 14))                                # 32 ... 8192
        sign = 1.0 if rng.random() < 0.8 else -1.0
        while True:
            x = float((nft + 1) / 6.0 * rng.uniform(1.0 / 1.002, 1.0))
            if n_fft(x) == nft and n_fft(1.002 * x) == 2 * nft:
                break
        lams[i], lams[j] = sign * x, sign * 1.002 * x
    return lams


def _draw_edges(rng, K, M):
    """(edges, default?) for K groups over M rows"""
    even = [(k * M) // K for k in range(K + 1)]
    if K == 1 or rng.random() < 0.5:
        return even, True
    if M == K:
        return list(range(K + 1)), False                                    # every group is one row
    # a one-row group [p, p + 1): both its ends are cuts (K = 2 has one cut: the row is the first or the last)
    p = int(rng.choice([0, M - 1])) if K == 2 else int(rng.integers(0, M))
    cuts = {c for c in (p, p + 1) if 1 <= c <= M - 1}
    rest = [c for c in range(1, M) if c not in cuts]
    cuts |= {int(c) for c in rng.choice(rest, K - 1 - len(cuts), replace=False)}
    return [0] + sorted(cuts) + [M], False


def _draw_lens(rng, case):
    L, hop, B = case["L"], case["hop"], case["B"]
    T = L // hop + 1
    edge = [v for v in (1, hop - 1, hop, hop + 1) if 1 <= v <= L]
    tile = (max(1, (T - 2) * hop), L) if L >= 2 else None                   # [lo, hi)
    if L > 32768:                                                           # B = 2: one above (L or a last-tile length), one below (an edge)
        above = L if rng.random() < 0.5 or tile[0] <= 32768 else int(rng.integers(max(tile[0], 32769), L))
        lens = [above, int(rng.choice(edge))]
    else:
        draws = {"edge": lambda: int(rng.choice(edge)), "full": lambda: L}
        if tile is not None:
            draws["last_tile"] = lambda: int(rng.integers(tile[0], tile[1]))
        names = list(draws)
        rng.shuffle(names)
        lens = [draws[c]() for c in names[:B]]
        lens += [int(rng.integers(1, L + 1)) for _ in range(B - len(lens))]
    order = rng.permutation(B)
    return [lens[i] for i in order]


def kwindow_cases(n, seed, cost_cap=6e6, prefix="kw"):
    rng = np.random.default_rng(seed)
    long_rows = {int(v) for v in rng.choice(n, 2, replace=False)}
    out = []
    while len(out) < n:
        i = len(out)
        lams = _draw_lams(rng)
        K = len(lams)
        ns = [n_fft(v) for v in lams]
        nf = int(rng.choice(ns))                                            # the channel whose n_fft sets the hop's scale
        if i in long_rows:
            L, hop, B = int(rng.integers(32769, 40001)), int(rng.integers(400, 2001)), 2
        else:
            L = int(rng.integers(max(8, min(ns) // 4), max(64, min(4 * max(ns), 30000))))
            hop = int(rng.integers(1, max(2, L // 3))) if rng.random() < 0.3 else int(rng.integers(max(1, nf // 8), max(2, nf)))
            B = int(rng.integers(1, 5))
        if L // hop + 1 > 300:
            hop = L // 299 + 1
        T = L // hop + 1
        sr = int(rng.choice(SRS))
        n_mels = int(rng.choice(N_MELS))
        f_min = float(rng.choice([0.0, 0.0, 50.0, 300.0]))
        f_max = None if rng.random() < 0.6 else float(rng.uniform(0.3, 0.5) * sr)
        if f_max is not None and f_max <= f_min + 100.0:
            f_max = None
        norm = bool(rng.random() < 0.4)
        Kb = min(K, n_mels)
        edges, default = _draw_edges(rng, Kb, n_mels)
        if B * K * T * max(ns) > cost_cap:
            continue
        case = dict(C.BY_NAME["g1_c1"], index=i, name=f"{prefix}{i}_K{K}_n{min(ns)}-{max(ns)}_L{L}_h{hop}_m{n_mels}_B{B}", B=B, L=L, lambd=lams[0], lams=lams,
                    hop=hop, n_mels=n_mels, sr=sr, f_min=f_min, f_max=f_max, normalize_window=norm, seed=7000 + i, edges=edges,
                    edges_default=default)
        case["lens"] = _draw_lens(rng, case)
        out.append(case)
    return out


def band_lams(case):
    return case["lams"][:len(case["edges"]) - 1]


def multi_cotangent(case):
    """(B, K, n_mels, T): the multi-window layer's upstream gradient (the band layer's is C.make_cotangent(case))"""
    from dmel_amd import synth
    B, _, M, T = C.out_shape(case)
    return synth.cotangent((B, len(case["lams"]), M, T), seed=2000 + case["seed"])


def channel_rows(which, case):
    """[(k, lambd[k], output channel, first row, one past the last row)]: what channel k of the layer (``which``: "multi" or "band") owns"""
    if which == "multi":
        return [(k, lam, k, 0, case["n_mels"]) for k, lam in enumerate(case["lams"])]
    e = case["edges"]
    return [(k, lam, 0, e[k], e[k + 1]) for k, lam in enumerate(band_lams(case))]


def cotangent(which, case):
    return multi_cotangent(case) if which == "multi" else C.make_cotangent(case)


def channel_cotangent(which, case, g, k):
    """what channel k's scalar layer is fed: g[:, k:k+1], or the band layer's one cotangent with +0.0 outside rows e_k ... e_{k+1} - 1"""
    if which == "multi":
        return np.ascontiguousarray(g[:, k:k + 1])
    lo, hi = case["edges"][k], case["edges"][k + 1]
    gk = np.zeros_like(g)
    gk[:, :, lo:hi] = g[:, :, lo:hi]
    return gk


def oracle_forward(case, x_np, lam, log, **drop):
    """O.forward of the case's settings at one window width (``drop``: settings overridden, e.g. f_max=None)"""
    from oracle import dmel_oracle as O
    kw = dict(f_min=case["f_min"], f_max=case["f_max"], normalize_window=case["normalize_window"])
    kw.update(drop)
    return O.forward(x_np, lam, case["hop"], case["n_mels"], case["sr"], apply_log=log, **kw)


def composed_xgrad(which, case, x_np, g_np, y_np, lens=None):
    """The reference of the K-window layers' x.grad: (sum over k, [term of channel k]) with term k O.backward_x at lambd[k] for the channel's
    cotangent (channel_cotangent) -- fp64, (B, L).  ``y_np``: the layer's LOG output (None: linear), from which a channel reads its own
    channel (multi) or the one image (band: the rows outside the group meet a zero cotangent).  ``lens``: clip by clip on x[b, :Lc] and the
    first Lc // hop + 1 frames; zero past the clip."""
    from oracle import dmel_oracle as O
    B, L = x_np.shape
    hop = case["hop"]
    terms = []
    for k, lam, c, lo, hi in channel_rows(which, case):
        gk = channel_cotangent(which, case, g_np, k)
        yk = None if y_np is None else y_np[:, c:c + 1]
        args = (case["f_min"], case["f_max"], case["normalize_window"])
        if lens is None:
            terms.append(O.backward_x(x_np, lam, hop, case["sr"], gk, yk, *args))
            continue
        t = np.zeros((B, L), np.float64)
        for b, lb in enumerate(lens):
            tb = lb // hop + 1
            t[b:b + 1, :lb] = O.backward_x(x_np[b:b + 1, :lb], lam, hop, case["sr"], gk[b:b + 1, :, :, :tb],
                                           None if yk is None else yk[b:b + 1, :, :, :tb], *args)
        terms.append(t)
    return sum(terms), terms


# The seeds tried first, 20261021 and 5821, drew cases the CPU test rejects: kw1, kw4 and kw39 of the first and kg5 of the second hold a band
# group whose rows the oracle cannot tell from the same rows at the neighbouring group's lambd (mel bands narrower than a bin of either n_fft:
# all-zero rows on both sides), so a swap of those rows would pass unseen.  The next seed of each replaces them.
FORWARD_SEED, GRAD_SEED = 20261022, 5822
FORWARD_CASES = kwindow_cases(40, FORWARD_SEED)
GRAD_CASES = kwindow_cases(16, GRAD_SEED, cost_cap=1.5e6, prefix="kg")
BF16_CASES = FORWARD_CASES[::5]

# Neighbouring band groups that hold the same lambd value (nothing tells their rows apart): (case name, k).  None in these draws.
SAME_LAMBD = []

# The (case / layer / fixed or lengths / lin or log / channel) whose ORACLE gradient is cancellation-dominated, |d_ref| <= 1e-3 sum |g t|: the only
# ones for which tests/test_hip_kwindow_random.py may skip the plain 1e-4 bar of _assert_dlam.  tests/test_kwindow_cases_cpu.py recomputes the list
# from the oracle alone and holds it to this one.
EXEMPT = [
    "kg13_K8_n32-2048_L1231_h121_m16_B2/band/lengths/log/k5",
    "kg13_K8_n32-2048_L1231_h121_m16_B2/multi/fixed/lin/k1",
    "kg8_K2_n512-2048_L5259_h372_m16_B3/band/fixed/log/k0",
    "kg9_K1_n1024-1024_L3193_h51_m80_B1/band/fixed/log/k0",
    "kg9_K1_n1024-1024_L3193_h51_m80_B1/band/lengths/log/k0",
    "kw0_K1_n2048-2048_L1773_h6_m40_B3/band/fixed/lin/k0",
    "kw14_K3_n64-16384_L16222_h4242_m80_B4/multi/fixed/log/k1",
    "kw14_K3_n64-16384_L16222_h4242_m80_B4/multi/lengths/lin/k1",
    "kw23_K2_n128-128_L424_h89_m40_B3/band/lengths/log/k0",
    "kw32_K5_n256-16384_L2733_h9349_m130_B3/band/lengths/log/k3",
    "kw34_K8_n64-2048_L4525_h695_m128_B1/multi/fixed/lin/k6",
    "kw9_K6_n256-4096_L11815_h1001_m128_B3/band/fixed/lin/k0",
]
