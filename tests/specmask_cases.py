"""SpecMask as numpy restates it, in integers only (include/dmel.h: dmel_specmask_draw / dmel_specmask_apply): Philox4x32-10, the draw of a
stripe, the (images, n_time + n_freq, 2) table of a call and the selection applied to the elements' BITS -- and the cases of the GPU tests.

  counter (calls & 0xffffffff, calls >> 32, image, k // 2), key (seed & 0xffffffff, seed >> 32); stripe k takes the words (w[2 (k % 2)], w[2 (k % 2) + 1])
  cap = min(param, size);  width = (w_a cap) >> 32;  lo = (w_b (size - width)) >> 32;  hi = lo + width
  time stripes: size = Tc, param = min(time_param, Tc * time_permille // 1000);   frequency stripes: size = n_mels, param = freq_param
  y = fill on a valid frame t < Tc under a time stripe or in a band under a frequency stripe, s's bits elsewhere and on every pad frame;
  a clip whose length is outside 1 ... T: every element NaN, its table rows zero

Tensors are (B, C, n_mels, T) arrays of the elements' bits (uint32 for fp32, uint16 for bf16); ``Tc`` a list of B lengths or None."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
NAN_BITS = {4: 0x7FC00000, 2: 0x7FC0}


def philox(c, k):
    """Philox4x32-10 of the counter words c[0 .. 3] under the key words k[0 .. 1]: Python integers, or uint64 arrays holding 32-bit values"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return c


def stripe(wa, wb, param, size):
    cap = min(param, size)
    width = (wa * cap) >> 32
    lo = (wb * (size - width)) >> 32
    return lo, lo + width


def time_param_of(time_param, time_permille, tc):
    """SpecAugment's adaptive cap, in integer division"""
    return min(time_param, tc * time_permille // 1000)


def table(shape, Tc, time_param, time_permille, n_time, freq_param, n_freq, seed, calls):
    """the int32 (B * C, n_time + n_freq, 2) table of one call"""
    B, C, M, T = shape
    n = n_time + n_freq
    tab = np.zeros((B * C, n, 2), dtype=np.int32)
    key = (seed & MASK32, (seed >> 32) & MASK32)
    for i in range(B * C):
        tc = T if Tc is None else int(Tc[i // C])
        if not 1 <= tc <= T:
            continue
        words = {}
        for k in range(n):
            if k // 2 not in words:
                words[k // 2] = philox((calls & MASK32, (calls >> 32) & MASK32, i, k // 2), key)
            w = words[k // 2]
            wa, wb = w[2 * (k % 2)], w[2 * (k % 2) + 1]
            if k < n_time:
                tab[i, k] = stripe(wa, wb, time_param_of(time_param, time_permille, tc), tc)
            else:
                tab[i, k] = stripe(wa, wb, freq_param, M)
    return tab


def filled(shape, Tc, tab, n_time):
    """(B, C, n_mels, T) bool: the elements that take the fill (none in a clip with an invalid length: that clip is NaN)"""
    B, C, M, T = shape
    out = np.zeros(shape, dtype=bool)
    for i in range(B * C):
        b = i // C
        tc = T if Tc is None else int(Tc[b])
        if not 1 <= tc <= T:
            continue
        tm, fm = np.zeros(T, dtype=bool), np.zeros(M, dtype=bool)
        for k, (lo, hi) in enumerate(tab[i]):
            (tm if k < n_time else fm)[lo:hi] = True
        m = tm[None, :] | fm[:, None]
        m[:, tc:] = False
        out[b, i % C] = m
    return out


def invalid(shape, Tc):
    """(B,) bool: the clips whose length is outside 1 ... T"""
    B, T = shape[0], shape[-1]
    return np.array([False] * B if Tc is None else [not 1 <= int(t) <= T for t in Tc])


def fill_bits(fill, elem_bytes):
    """the fill value as the element's bits: fp32 as it is, bf16 rounded to nearest even"""
    u = int(np.array([fill], dtype=np.float32).view(np.uint32)[0])
    if elem_bytes == 4:
        return u
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0x7FC0
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def apply(bits, Tc, tab, n_time, fill):
    """y's bits from s's bits (a (B, C, n_mels, T) uint32 or uint16 array); the backward is apply(g's bits, ..., fill=0.0)"""
    out = bits.copy()
    out[filled(bits.shape, Tc, tab, n_time)] = fill_bits(fill, bits.dtype.itemsize)
    out[invalid(bits.shape, Tc)] = NAN_BITS[bits.dtype.itemsize]
    return out


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------
# (B, C, n_mels, T): one element; two frames; row packing at the 32-frame edge; chunk edges; more images than one workgroup has lanes
# (300 x 4 stripes: two rounds of the draw); real band counts
SHAPES = [(1, 1, 1, 1), (2, 1, 3, 2), (3, 2, 5, 31), (2, 1, 4, 32), (2, 3, 7, 33), (2, 1, 3, 63), (1, 2, 2, 64), (2, 1, 2, 65), (1, 1, 3, 130),
          (300, 1, 2, 5), (2, 1, 128, 32), (2, 1, 64, 81)]
STRIPES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (4, 4), (8, 0)]
TIME_PARAMS = [64, 8, 0, 1000, 20]          # 1000: larger than every axis here; 0: no stripe
FREQ_PARAMS = [8, 300, 2, 0]                # 300: larger than every axis here
PERMILLES = [1000, 200]
CALLS = [0, 1, (1 << 32) + 3]               # the last one reaches the high counter word
SEED = 0x1234567887654321
PAD_PATTERN = [0x7FC00001, 0x80000000, 0x3FC00000, 0xFF800000, 0x7F800001, 0x00000001]      # a NaN, -0.0, 1.5, -inf, a signalling NaN, a denormal


def frame_lengths(shape, idx):
    """B lengths: one clip: T // 2 (at least 1) or, for odd idx, 1; two: (T, 1) or (mid, T); more: T, 1, mid, then random in 1 ... T"""
    B, T = shape[0], shape[-1]
    mid = max(1, T // 2)
    if B == 1:
        return [1 if idx % 2 else mid]
    if B == 2:
        return [T, 1] if idx % 2 == 0 else [mid, T]
    rng = np.random.RandomState(100 + idx)
    return [T, 1, mid] + [int(v) for v in rng.randint(1, T + 1, size=B - 3)]


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for with_lengths in (False, True):
            i = len(out)
            n_time, n_freq = STRIPES[i % len(STRIPES)]
            out.append(dict(shape=shape, Tc=frame_lengths(shape, si) if with_lengths else None, n_time=n_time, n_freq=n_freq,
                            time_param=TIME_PARAMS[i % len(TIME_PARAMS)], freq_param=FREQ_PARAMS[i % len(FREQ_PARAMS)],
                            time_permille=PERMILLES[(i // 2) % 2], calls=CALLS[i % len(CALLS)], seed=SEED + i, fill=0.0 if i % 3 else -1.5))
    # the large counts on the real band counts, full and mixed lengths, both caps: what makes stripes overlap and reach the last positions
    for shape, Tc, permille in (((2, 1, 128, 32), None, 1000), ((2, 1, 64, 81), [81, 40], 200), ((3, 2, 5, 31), [31, 1, 15], 1000),
                                ((2, 1, 64, 81), [20, 81], 1000)):
        i = len(out)
        out.append(dict(shape=shape, Tc=Tc, n_time=4, n_freq=4, time_param=64, freq_param=8, time_permille=permille, calls=CALLS[i % 3],
                        seed=SEED + i, fill=0.0))
    return out


CASES = _cases()


def case_id(c):
    lens = "full" if c["Tc"] is None else "lengths"
    return f'{"x".join(str(v) for v in c["shape"])}-{lens}-{c["n_time"]}t{c["n_freq"]}f-p{c["time_param"]}-{c["freq_param"]}-m{c["time_permille"]}-c{c["calls"]}'


def case_table(c, calls=None):
    return table(c["shape"], c["Tc"], c["time_param"], c["time_permille"], c["n_time"], c["freq_param"], c["n_freq"], c["seed"],
                 c["calls"] if calls is None else calls)


def input_bits(shape, Tc, seed, elem_bytes):
    """(s, g) as bits: finite random values on the valid frames and, on every pad frame, PAD_PATTERN in turn (bf16: its upper halves)"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    B, C, M, T = shape
    out = []
    for _ in range(2):
        u = rng.standard_normal(shape).astype(np.float32).view(np.uint32)
        if Tc is not None:
            pat = np.array(PAD_PATTERN, dtype=np.uint32)[np.arange(B * C * M * T).reshape(shape) % len(PAD_PATTERN)]
            pad = np.arange(T)[None, None, None, :] >= np.asarray(Tc).reshape(B, 1, 1, 1)
            u = np.where(pad, pat, u)
        out.append(u if elem_bytes == 4 else (u >> 16).astype(np.uint16))
    return out
