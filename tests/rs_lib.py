"""The NumPy model of the Reed-Solomon outer code, written from the text of include/svsrs.h ("THE FORMAT") and not from
csrc/svs_rs.hpp: the field, g(x) as a product, the encoder as a polynomial division, the decoder over whole received codewords
(syndromes c(alpha^j) of all k_c + 32 bytes, Berlekamp-Massey on all dirty codewords at once, roots by evaluating the locator at
every position, Forney), and `check_definition`, which holds a decoder's output against the format's definition; the inputs of
tests/test_rs_gpu.py, so that the CPU tier runs the host build of svs_rs.hpp (tests/hostemu/rs_emu.cpp) on the same ones; and
the channel experiment of the README's table (tests/channel_lib.py's frames and model of the channel, tests/fec_lib.py's and
tests/fec_punctured_lib.py's inner code)."""
import ctypes as C

import numpy as np

from testlib import build_emu

N, K, PARITY, T = 255, 223, 32, 16
UNCORRECTABLE = 255
POLY = 0x11D

# ---- the field ------------------------------------------------------------------------------------------------------------------
EXP = np.zeros(510, np.int64)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= POLY
_a, _b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
MUL = np.where((_a == 0) | (_b == 0), 0, EXP[(LOG[_a] + LOG[_b]) % 255]).astype(np.uint8)           # MUL[a, b] = a b
DIV = np.where(_a == 0, 0, EXP[(LOG[_a] - LOG[_b]) % 255]).astype(np.uint8)                          # DIV[a, b] = a / b, b != 0
del _a, _b, _x, _i


def generator():
    """g(x) = prod (x - alpha^i), i = 0 .. 31: 33 coefficients, the highest first"""
    g = [1]
    for i in range(PARITY):
        root = int(EXP[i])
        g = [a ^ int(MUL[root, b]) for a, b in zip(g + [0], [0] + g)]
    return g


G = generator()


# ---- sizes and the layout ---------------------------------------------------------------------------------------------------------
def codewords(k):
    return -(-k // K)


def coded_bytes(k):
    return k + PARITY * codewords(k)


def data_bytes(total):
    """the largest k with coded_bytes(k) <= total, by bisection: coded_bytes is strictly increasing"""
    lo, hi = 0, total + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if coded_bytes(mid) <= total else (lo, mid)
    return lo


def lengths(k):
    """k_c of every codeword"""
    n_cw = codewords(k)
    return np.array([-(-(k - c) // n_cw) for c in range(n_cw)], np.int64)


def gather(k):
    """(index [C, rows + 32], valid [C, rows + 32]): the place in the stream of every codeword byte, data before parity, each
    codeword right-aligned - one that is a byte shorter starts with an invalid entry (a zero coefficient at the top)"""
    n_cw, kc = codewords(k), lengths(k)
    rows = int(kc.max())
    c = np.arange(n_cw)[:, None]
    i = np.arange(rows)[None, :] - (rows - kc)[:, None]                     # the data byte's number, negative: none
    data = i * n_cw + c
    parity = k + np.arange(PARITY)[None, :] * n_cw + c
    index = np.concatenate([np.where(i >= 0, data, 0), parity], axis=1)
    valid = np.concatenate([i >= 0, np.ones((n_cw, PARITY), bool)], axis=1)
    return index, valid


def codeword_matrix(stream, k):
    index, valid = gather(k)
    return np.where(valid, np.asarray(stream, np.uint8)[index], 0).astype(np.uint8)


# ---- the encoder: p(x) = d(x) x^32 mod g(x), by long division --------------------------------------------------------------------
def parity_of(data):
    """the 32 parity bytes of one codeword's data bytes"""
    rem = [int(v) for v in data] + [0] * PARITY
    for i in range(len(data)):
        lead = rem[i]
        if lead:
            for j in range(1, PARITY + 1):
                rem[i + j] ^= int(MUL[lead, G[j]])
    return rem[len(data):]


def encode(data):
    data = np.asarray(data, np.uint8).reshape(-1)
    k, n_cw = data.size, codewords(data.size)
    out = np.empty(coded_bytes(k), np.uint8)
    out[:k] = data
    for c in range(n_cw):
        out[k + np.arange(PARITY) * n_cw + c] = parity_of(data[c::n_cw])
    return out


# ---- the decoder ------------------------------------------------------------------------------------------------------------------
def syndromes(words):
    """uint8 [n, 32]: S_j = c(alpha^j) of every row of `words` (highest coefficient first), by Horner's rule"""
    acc = np.zeros((words.shape[0], PARITY), np.uint8)
    roots = EXP[np.arange(PARITY)].astype(np.uint8)[None, :]
    for i in range(words.shape[1]):
        acc = MUL[acc, roots] ^ words[:, i: i + 1]
    return acc


def _evaluate(poly, zlog):
    """poly uint8 [n, m] (coefficient i of x^i), zlog int [n, p]: poly(alpha^zlog) -> uint8 [n, p]"""
    acc = np.zeros(zlog.shape, np.uint8)
    for i in range(poly.shape[1]):
        coef = poly[:, i: i + 1]
        acc ^= np.where(coef == 0, 0, EXP[(LOG[coef] + i * zlog) % 255]).astype(np.uint8)
    return acc


def decode_words(words, n_c):
    """words uint8 [n, width], right-aligned codewords of n_c[i] bytes -> (corrected words, status uint8 [n])"""
    words = words.copy()
    n, width = words.shape
    status = np.zeros(n, np.uint8)
    syn_all = syndromes(words)
    dirty = np.flatnonzero(syn_all.any(axis=1))
    if dirty.size == 0:
        return words, status
    S = syn_all[dirty]
    m = dirty.size
    W = 2 * PARITY
    lam = np.zeros((m, W), np.uint8)
    lam[:, 0] = 1
    B = np.zeros((m, W), np.uint8)
    B[:, 1] = 1                                              # x^m B with m = 1
    L = np.zeros(m, np.int64)
    b = np.ones(m, np.uint8)
    for step in range(PARITY):
        d = np.bitwise_xor.reduce(MUL[lam[:, : step + 1], S[:, step::-1]], axis=1)
        longer = (d != 0) & (2 * L <= step)
        scale = DIV[d, b]
        new = lam ^ MUL[scale[:, None], B]
        keep = np.where(longer[:, None], lam, B)
        b = np.where(longer, d, b)
        L = np.where(longer, step + 1 - L, L)
        lam = new
        B = np.zeros_like(keep)
        B[:, 1:] = keep[:, :-1]
    ok = L <= T
    p = np.arange(N)[None, :]
    zlog = np.broadcast_to((255 - p) % 255, (m, N))
    own = p < n_c[dirty][:, None]
    is_root = (_evaluate(lam[:, : T + 1], zlog) == 0) & own
    ok &= is_root.sum(axis=1) == L
    omega = np.zeros((m, PARITY), np.uint8)                  # S Lambda mod x^32
    for j in range(PARITY):
        omega[:, j] = np.bitwise_xor.reduce(MUL[lam[:, : j + 1], S[:, j::-1]], axis=1)
    slope_poly = lam[:, 1: T + 1: 2]                         # Lambda'(z) = sum over odd i of Lambda_i z^(i - 1): a polynomial in z^2
    slope = _evaluate(slope_poly, (2 * zlog) % 255)
    top = _evaluate(omega, zlog)
    ok &= ~((is_root & ((slope == 0) | (top == 0))).any(axis=1))
    value = MUL[EXP[p % 255].astype(np.uint8), DIV[top, np.where(slope == 0, 1, slope)]]
    value = np.where(is_root & ok[:, None], value, 0).astype(np.uint8)       # by position p; column width - 1 - p
    for row, at in enumerate(dirty):
        if ok[row]:
            words[at] ^= value[row, width - 1:: -1]
            status[at] = L[row]
        else:
            status[at] = UNCORRECTABLE
    return words, status


def decode(stream, k):
    """the format's decoder on a stream of coded_bytes(k) bytes -> (stream uint8, status uint8 [C], counts (corrected, failed))"""
    stream = np.array(stream, np.uint8).reshape(-1)
    assert stream.size == coded_bytes(k)
    index, valid = gather(k)
    words = np.where(valid, stream[index], 0).astype(np.uint8)
    fixed, status = decode_words(words, lengths(k) + PARITY)
    assert not (fixed[~valid]).any(), "a correction outside the codeword's own bytes"
    stream[index[valid]] = fixed[valid]
    good = status != UNCORRECTABLE
    return stream, status, (int(status[good].sum()), int((~good).sum()))


def check_definition(received, decoded, status, k):
    """the definition of include/svsrs.h on a decoder's output: a codeword with a status 0 .. 16 is a code word (zero syndromes)
    that differs from the received one in exactly `status` bytes; one with 255 is as received"""
    before, after = codeword_matrix(received, k), codeword_matrix(decoded, k)
    changed = (before != after).sum(axis=1)
    bad = status == UNCORRECTABLE
    assert ((status <= T) | bad).all()
    assert (changed[bad] == 0).all() and (changed[~bad] == status[~bad]).all(), (changed, status)
    assert not syndromes(after[~bad]).any()
    assert syndromes(after[bad]).any(axis=1).all()


# ---- what the GPU test runs (tests/test_rs_gpu.py); the CPU tier runs the host build of csrc/svs_rs.hpp on the same inputs ------
# one byte; one codeword one byte short of full and full; two codewords of equal (224) and unequal (225) length; the last k of
# two codewords, the first of three, and three unequal; exactly the 64 codewords of one workgroup and one more; five workgroups
# with a ragged last one and k mod C != 0
KS = (1, 222, 223, 224, 225, 445, 446, 447, 64 * 223, 64 * 223 + 1, 257 * 223 + 5)
KINDS = ("clean", "one", "sixteen", "seventeen", "random", "zero", "ends", "burst")
INPUT_SEED = 41


def _rng(kind, k):
    return np.random.default_rng([INPUT_SEED, k, sum(map(ord, kind))])


def _hit(stream, rng, k, c, places):
    """xor a non-zero random byte into the bytes `places` (codeword byte numbers) of codeword c"""
    n_cw, kc = codewords(k), int(lengths(k)[c])
    for i in places:
        at = i * n_cw + c if i < kc else k + (i - kc) * n_cw + c
        stream[at] ^= rng.integers(1, 256)


def received_input(kind, k):
    """the received stream of one case: uint8 [coded_bytes(k)]"""
    rng = _rng(kind, k)
    n_cw, kc = codewords(k), lengths(k)
    if kind == "zero":
        return np.zeros(coded_bytes(k), np.uint8)           # all zero is a code word
    if kind == "random":
        return rng.integers(0, 256, coded_bytes(k)).astype(np.uint8)
    stream = encode(rng.integers(0, 256, k).astype(np.uint8))
    if kind == "burst":
        length = min(n_cw, 40)
        start = int(rng.integers(0, stream.size - length + 1))
        stream[start: start + length] ^= rng.integers(1, 256, length).astype(np.uint8)
    for c in range(n_cw):
        n_c = int(kc[c]) + PARITY
        if kind == "one":
            _hit(stream, rng, k, c, rng.choice(n_c, 1, replace=False))
        elif kind == "seventeen":
            _hit(stream, rng, k, c, rng.choice(n_c, 17, replace=False))
        elif kind == "ends" and c in (0, n_cw - 1):
            _hit(stream, rng, k, c, rng.choice(n_c, 3, replace=False))
        elif kind == "sixteen":
            if c % 2:                                        # parity only, the last parity byte among them
                places = [n_c - 1] + list(n_c - 2 - rng.choice(PARITY - 1, 15, replace=False))
            else:                                            # the first data byte, the last parity byte and 14 between
                places = [0, n_c - 1] + list(1 + rng.choice(n_c - 2, 14, replace=False))
            _hit(stream, rng, k, c, places)
    return stream


_CASES = {}


def case(kind, k):
    """(received, the model's stream, status, counts) of one input of the GPU test, computed once per process"""
    key = (kind, k)
    if key not in _CASES:
        received = received_input(kind, k)
        stream, status, counts = decode(received, k)
        for a in (received, stream, status):
            a.setflags(write=False)
        _CASES[key] = (received, stream, status, counts)
    return _CASES[key]


# ---- the host build of csrc/svs_rs.hpp (tests/hostemu/rs_emu.cpp) ------------------------------------------------------------------
_U64, _P = C.c_uint64, C.c_void_p
PROTOTYPES = {
    "rs_emu_decode": (C.c_int, [_P, _U64, _P, _P, _P]),
    "rs_emu_encode": (C.c_int, [_P, _U64, _P]),
    "rs_emu_data_bytes": (_U64, [_U64]),
    "rs_emu_coded_bytes": (_U64, [_U64]),
}


def emu(build_dir=None):
    """tests/hostemu/rs_emu.cpp, compiled once per process with g++ as the other host emulations are"""
    return build_emu("rs_emu.cpp", PROTOTYPES, build_dir)


def emu_decode(received, k, counts=(0, 0), build_dir=None, mask=None):
    """the host build's decoder (mask: the erased bytes, tests/rse_lib.py; here none) -> (stream, status, counts)"""
    stream = np.array(received, np.uint8)
    status = np.full(codewords(k), 0xEE, np.uint8)
    cnt = np.array(counts, np.uint32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    assert emu(build_dir).rs_emu_decode(stream.ctypes.data, k, None if m is None else m.ctypes.data, status.ctypes.data, cnt.ctypes.data) == 0
    return stream, status, (int(cnt[0]), int(cnt[1]))


# ---- the README's table: both codes through the requantisation channel -------------------------------------------------------------
NAMES = {2: "1/2", 3: "1/3", 23: "2/3", 34: "3/4", 56: "5/6", 78: "7/8"}


def inner(rate):
    """(encode, decode_soft, info_bits) of the inner code at `rate`, from whichever model holds it"""
    import fec_lib as fl
    import fec_punctured_lib as fpl
    lib = fpl if rate in fpl.CODES else fl
    return lib.encode, lib.decode_soft, lib.info_bits


def outer_clip(rate, seed, n_ac=10):
    """(cover, data): channel_lib.survival's three frames of noise in [64, 192) from default_rng(seed) and, drawn behind them
    from the same generator, k = data_bytes(info_bits(capacity, rate) // 8) random data bytes"""
    import channel_lib as cl
    rng = np.random.default_rng(seed)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    k = data_bytes(inner(rate)[2](f * (h // 8) * (w // 8) * n_ac, rate) // 8)
    return cover, rng.integers(0, 256, k).astype(np.uint8)


def outer_survival(rate, quality, seed, delta=20, n_ac=10):
    """the chain of fec_lib.coded_survival / fec_punctured_lib.coded_survival (reference rule, one step) with the RS stream of
    the data as the info bits -> dict(k, C, viterbi_bits: wrong payload bits after Viterbi, viterbi_bytes: wrong data bytes after
    Viterbi, status: the outer decoder's status bytes, wrong_bits: wrong payload bits after the outer code, data / received /
    decoded: the data bytes sent, as Viterbi left them and as the outer code left them)"""
    import channel_lib as cl
    import soft_lib as sl
    from svsdct import channel
    encode_inner, decode_inner, _ = inner(rate)
    cover, data = outer_clip(rate, seed, n_ac)
    k = data.size
    sent = encode(data)
    info = np.unpackbits(sent)
    f, h, w = cover.shape
    per_frame = (h // 8) * (w // 8) * n_ac
    coded = encode_inner(info, rate)
    stream = np.zeros(f * per_frame, np.uint8)
    stream[: coded.size] = coded
    stego = np.stack([cl.model_stego(cover[i: i + 1], delta, n_ac, stream[i * per_frame: (i + 1) * per_frame])[0] for i in range(f)])
    soft = sl.model_batch_soft(cl.model_requantise(stego, channel.quality_steps(quality)), delta, n_ac)[: coded.size]
    received = np.packbits(decode_inner(soft, info.size, rate))
    decoded, status, _ = decode(received, k)
    bits = lambda a: int(np.unpackbits(a[:k] ^ data).sum())   # noqa: E731
    return dict(k=k, C=codewords(k), viterbi_bits=bits(received), viterbi_bytes=int((received[:k] != data).sum()), status=status,
                wrong_bits=bits(decoded), data=data, received=received, decoded=decoded, soft=soft, info_bits=info.size)
