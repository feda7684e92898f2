"""The NumPy model of errors-and-erasures decoding of the Reed-Solomon outer code, written from the text of include/svsrse.h
("THE FORMAT") and not from csrc/svs_rs.hpp: the field, the layout and the syndromes are tests/rs_lib.py's; here are the erasure
locator, Berlekamp-Massey started from it on all dirty codewords at once, the roots by evaluating the locator at every position,
Forney, and `check_definition`, which holds a decoder's output against the format's definition; the inputs of
tests/test_rse_gpu.py, so that the CPU tier runs the host build of svs_rs.hpp (tests/hostemu/rs_emu.cpp) on the same ones; and
the lost-frame experiment of the README's table (tests/channel_lib.py's model of the embed, tests/soft_lib.py's soft bytes,
tests/fec_lib.py's inner code)."""
import numpy as np

import rs_lib as rl
from rs_lib import DIV, EXP, MUL, N, PARITY, UNCORRECTABLE, codewords, coded_bytes, encode, gather, lengths, syndromes, _evaluate

MAX_ERASED = 32


# ---- the decoder ------------------------------------------------------------------------------------------------------------------
def erasure_locator(positions, f):
    """positions int [m, 32] (the first f[i] of a row count), f int [m] -> Gamma uint8 [m, 33], coefficient i of x^i:
    prod (1 - alpha^p x)"""
    gam = np.zeros((positions.shape[0], MAX_ERASED + 1), np.uint8)
    gam[:, 0] = 1
    for t in range(MAX_ERASED):
        x = EXP[positions[:, t] % 255].astype(np.uint8)
        shifted = np.zeros_like(gam)
        shifted[:, 1:] = gam[:, :-1]
        gam = np.where((t < f)[:, None], gam ^ MUL[x[:, None], shifted], gam)
    return gam


def decode_words(words, n_c, erased):
    """words uint8 [n, width], right-aligned codewords of n_c[i] bytes; erased bool [n, width] (False outside a codeword)
    -> (corrected words, status uint8 [n])"""
    words = words.copy()
    n, width = words.shape
    status = np.zeros(n, np.uint8)
    f_all = erased.sum(axis=1)
    status[f_all > MAX_ERASED] = UNCORRECTABLE                  # whatever the received bytes are
    syn_all = syndromes(words)
    dirty = np.flatnonzero(syn_all.any(axis=1) & (f_all <= MAX_ERASED))
    if dirty.size == 0:
        return words, status
    S, f, m = syn_all[dirty], f_all[dirty], dirty.size
    # by position p (the byte that multiplies x^p is column width - 1 - p)
    p = np.arange(N)[None, :]
    erased_at = np.zeros((m, N), bool)
    erased_at[:, :width] = erased[dirty][:, ::-1]
    positions = np.argsort(~erased_at, axis=1, kind="stable")[:, :MAX_ERASED]
    W = 2 * PARITY + 2
    lam = np.zeros((m, W), np.uint8)
    lam[:, : MAX_ERASED + 1] = erasure_locator(positions, f)
    B = np.zeros((m, W), np.uint8)
    B[:, 1:] = lam[:, :-1]                                   # x B = x Gamma
    L = f.copy()
    b = np.ones(m, np.uint8)
    for step in range(PARITY):
        runs = step >= f                                     # the steps run n = f .. 31
        d = np.bitwise_xor.reduce(MUL[lam[:, : step + 1], S[:, step::-1]], axis=1)
        d = np.where(runs, d, 0)
        longer = (d != 0) & (2 * L <= step + f)
        new = lam ^ MUL[DIV[d, b][:, None], B]
        keep = np.where(longer[:, None], lam, B)
        b = np.where(longer, d, b)
        L = np.where(longer, step + 1 - L + f, L)
        lam = new
        shifted = np.zeros_like(keep)
        shifted[:, 1:] = keep[:, :-1]
        B = np.where(runs[:, None], shifted, B)
    ok = 2 * L - f <= PARITY
    zlog = np.broadcast_to((255 - p) % 255, (m, N))
    own = p < n_c[dirty][:, None]
    is_root = (_evaluate(lam[:, : MAX_ERASED + 1], zlog) == 0) & own
    ok &= is_root.sum(axis=1) == L
    ok &= ~(erased_at & ~is_root).any(axis=1)                # an erased position that is no root
    omega = np.zeros((m, PARITY), np.uint8)                  # S Lambda mod x^32
    for j in range(PARITY):
        omega[:, j] = np.bitwise_xor.reduce(MUL[lam[:, : j + 1], S[:, j::-1]], axis=1)
    slope = _evaluate(lam[:, 1: MAX_ERASED + 1: 2], (2 * zlog) % 255)    # Lambda'(z): the odd coefficients, a polynomial in z^2
    top = _evaluate(omega, zlog)
    ok &= ~(is_root & (slope == 0)).any(axis=1)
    ok &= ~(is_root & (top == 0) & ~erased_at).any(axis=1)   # a zero value at an erased root is a byte that was right
    value = MUL[EXP[p % 255].astype(np.uint8), DIV[top, np.where(slope == 0, 1, slope)]]
    value = np.where(is_root & ok[:, None], value, 0).astype(np.uint8)
    for row, at in enumerate(dirty):
        if ok[row]:
            words[at] ^= value[row, width - 1:: -1]
            status[at] = np.count_nonzero(value[row])
        else:
            status[at] = UNCORRECTABLE
    return words, status


def mask_matrix(mask, k):
    """bool [C, rows + 32]: the mask's bytes at the places of gather(k), False where a codeword has no byte"""
    index, valid = gather(k)
    if mask is None:
        return np.zeros(index.shape, bool)
    mask = np.asarray(mask, np.uint8).reshape(-1)
    assert mask.size == coded_bytes(k)
    return valid & (mask[index] != 0)


def decode(stream, k, mask=None):
    """the format's decoder on a stream of coded_bytes(k) bytes with the mask's bytes erased
    -> (stream uint8, status uint8 [C], counts (bytes changed, codewords with 255))"""
    stream = np.array(stream, np.uint8).reshape(-1)
    assert stream.size == coded_bytes(k)
    index, valid = gather(k)
    words = np.where(valid, stream[index], 0).astype(np.uint8)
    fixed, status = decode_words(words, lengths(k) + PARITY, mask_matrix(mask, k))
    assert not (fixed[~valid]).any(), "a correction outside the codeword's own bytes"
    stream[index[valid]] = fixed[valid]
    good = status != UNCORRECTABLE
    return stream, status, (int(status[good].sum()), int((~good).sum()))


def check_definition(received, decoded, status, k, mask=None):
    """the definition of include/svsrse.h on a decoder's output: a codeword with a status 0 .. 32 is a code word (zero
    syndromes) that differs from the received one in exactly `status` bytes, e of them outside E_c with 2 e + f_c <= 32; one
    with 255 is as received"""
    before, after = rl.codeword_matrix(received, k), rl.codeword_matrix(decoded, k)
    erased = mask_matrix(mask, k)
    f = erased.sum(axis=1)
    changed = (before != after).sum(axis=1)
    outside = ((before != after) & ~erased).sum(axis=1)
    bad = status == UNCORRECTABLE
    assert ((status <= MAX_ERASED) | bad).all()
    assert (changed[bad] == 0).all() and (changed[~bad] == status[~bad]).all(), (changed, status)
    assert (2 * outside[~bad] + f[~bad] <= PARITY).all()
    assert not syndromes(after[~bad]).any()


# ---- what the GPU test runs (tests/test_rse_gpu.py); the CPU tier runs the host build of csrc/svs_rs.hpp on the same inputs -----
KS = rl.KS
NOMASK_KINDS = ("sixteen", "seventeen", "random", "burst")   # rs_lib's inputs, run with a NULL mask and with a mask of zeros
KINDS = ("erasures32", "mixed", "over", "f33", "right", "right0", "ends", "burst32", "random", "values")
INPUT_SEED = 43
MASK_VALUES = (1, 0x80, 0xFF)


def _rng(kind, k):
    return np.random.default_rng([INPUT_SEED, k, sum(map(ord, kind))])


def _at(k, c, i):
    """where byte i of codeword c lies in the stream"""
    n_cw, kc = codewords(k), -(-(k - c) // codewords(k))
    return i * n_cw + c if i < kc else k + (i - kc) * n_cw + c


def _plan(kind, c, n_c, rng):
    """(erased places, of them left right, error places) of codeword c, as codeword byte numbers"""
    if kind == "ends":
        return [0, n_c - 1], [], list(1 + rng.choice(n_c - 2, 15, replace=False))
    f, e = {"erasures32": (32, 0), "mixed": (2 * (c % 17), (32 - 2 * (c % 17)) // 2), "values": (2 * (c % 17), (32 - 2 * (c % 17)) // 2),
            "over": (2 * (c % 16) + 1, (33 - (2 * (c % 16) + 1)) // 2), "f33": (33, 0), "right": (10, 11), "right0": (10, 0)}[kind]
    places = [int(v) for v in rng.choice(n_c, f + e, replace=False)]
    erased = places[:f]
    return erased, erased if kind in ("f33", "right", "right0") else [], places[f:]


def received_input(kind, k):
    """(received uint8 [coded_bytes(k)], mask uint8 [coded_bytes(k)], sent or None) of one case"""
    rng = _rng(kind, k)
    n_cw, kc, total = codewords(k), lengths(k), coded_bytes(k)
    if kind == "random":
        return rng.integers(0, 256, total).astype(np.uint8), (rng.random(total) < 0.05).astype(np.uint8), None
    sent = encode(rng.integers(0, 256, k).astype(np.uint8))
    received, mask = sent.copy(), np.zeros(total, np.uint8)
    if kind == "burst32":
        # one run of 32 C consecutive bytes; inside the data bytes, where they hold one, it puts exactly 32 into every codeword
        length = 32 * n_cw
        start = int(rng.integers(0, (k if k >= length else total) - length + 1))
        received[start: start + length] ^= rng.integers(1, 256, length).astype(np.uint8)
        mask[start: start + length] = 1
        return received, mask, sent
    for c in range(n_cw):
        erased, right, errors = _plan(kind, c, int(kc[c]) + PARITY, rng)
        for i in erased:
            mask[_at(k, c, i)] = rng.choice(MASK_VALUES) if kind == "values" else 1
        for i in [i for i in erased if i not in right] + errors:
            received[_at(k, c, i)] ^= rng.integers(1, 256)
    return received, mask, sent


_CASES = {}


def case(kind, k):
    """(received, mask, sent or None, the model's stream, status, counts) of one input of the GPU test, computed once per process"""
    key = (kind, k)
    if key not in _CASES:
        received, mask, sent = received_input(kind, k)
        stream, status, counts = decode(received, k, mask)
        for a in (received, mask, stream, status):
            a.setflags(write=False)
        _CASES[key] = (received, mask, sent, stream, status, counts)
    return _CASES[key]


# ---- the host build of csrc/svs_rs.hpp: rs_lib's (tests/hostemu/rs_emu.cpp), called with a mask ------------------------------------
emu = rl.emu


def emu_decode(received, k, mask=None, counts=(0, 0), build_dir=None):
    """the host build's decoder -> (stream, status, counts)"""
    return rl.emu_decode(received, k, counts, build_dir, mask)


# ---- the README's table: a lost frame -------------------------------------------------------------------------------------------------
LOST_SHAPE = (12, 96, 160)
LOST_SEEDS = (1, 2, 3)
LOST_FRAMES = (0, 5, 11)


def steps_of_sent_bits(lo, hi, rate):
    """brute force over S(t) of include/svsfec.h: the steps t whose sent bits [S(t), S(t + 1)) touch [lo, hi) -> (t0, t1)"""
    from svsdct import fec
    out0, out1 = fec.PATTERNS.get(rate, ((1,), (rate - 1,)))        # rates 2 and 3: every step sends `rate` bits
    hit, before = [], 0
    for t in range(hi + 1):                                  # a step sends at least one bit: S(t) >= t
        after = before + out0[t % len(out0)] + out1[t % len(out0)]
        if before < hi and after > lo:
            hit.append(t)
        before = after
    return hit[0], hit[-1] + 1


def erased_span(frame, n_frames, cap, rate, k, margin=1):
    """the byte span [lo, hi) of the Reed-Solomon stream that the capacity bits of `frame` map to, widened by `margin`"""
    t0, t1 = steps_of_sent_bits(frame * cap // n_frames, (frame + 1) * cap // n_frames, rate)
    total = coded_bytes(k)
    return max(min(t0 // 8, total) - margin, 0), min(min(-(-t1 // 8), total) + margin, total)


_LOST = {}


def lost_frame(seed, frame, delta=20, n_ac=10, rate=2, margin=1):
    """twelve 96 x 160 frames of noise in [64, 192) at full capacity (k = 1 561, C = 7), frame `frame` replaced by fresh noise
    before extraction -> dict(cover, data, received: the frames the receiver gets; plain: (stream, status) of today's chain on
    them; erased: (stream, status) with the frame's soft bytes set to 0x00 and its byte span erased; span; outside: wrong bytes
    after Viterbi outside the span)"""
    key = (seed, frame, margin)
    if key in _LOST:
        return _LOST[key]
    import channel_lib as cl
    import fec_lib as fl
    import soft_lib as sl
    rng = np.random.default_rng(seed)
    f, h, w = LOST_SHAPE
    cover = rng.integers(64, 192, LOST_SHAPE).astype(np.uint8)
    per_frame = (h // 8) * (w // 8) * n_ac
    cap = f * per_frame
    k = rl.data_bytes(fl.info_bits(cap, rate) // 8)
    data = rng.integers(0, 256, k).astype(np.uint8)
    sent = encode(data)
    info = np.unpackbits(sent)
    coded = fl.encode(info, rate)
    stream = np.zeros(cap, np.uint8)
    stream[: coded.size] = coded
    stego = np.stack([cl.model_stego(cover[i: i + 1], delta, n_ac, stream[i * per_frame: (i + 1) * per_frame])[0] for i in range(f)])
    received = stego.copy()
    received[frame] = rng.integers(64, 192, (h, w)).astype(np.uint8)
    soft = sl.model_batch_soft(received, delta, n_ac)
    plain_in = np.packbits(fl.decode_soft(soft[: coded.size], info.size, rate))
    plain = decode(plain_in, k)[:2]
    soft = soft.copy()
    soft[frame * per_frame: (frame + 1) * per_frame] = 0
    viterbi = np.packbits(fl.decode_soft(soft[: coded.size], info.size, rate))
    lo, hi = erased_span(frame, f, cap, rate, k, margin)
    mask = np.zeros(sent.size, np.uint8)
    mask[lo:hi] = 1
    wrong = np.flatnonzero(viterbi != sent)
    _LOST[key] = dict(cover=cover, data=data, k=k, sent=sent, received=received, plain=plain, plain_wrong=int((plain_in != sent).sum()),
                      erased=decode(viterbi, k, mask)[:2], span=(lo, hi), wrong=int(wrong.size),
                      outside=int(((wrong < lo) | (wrong >= hi)).sum()))
    return _LOST[key]
