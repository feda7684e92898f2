"""The NumPy model of the convolutional code and its windowed Viterbi decoder, written from the text of include/svsfec.h ("THE
FORMAT") and not from csrc/svs_fec.hpp: the encoder, the weights, the windowed decoder, an untruncated Viterbi for comparison;
the inputs of tests/test_fec_gpu.py, so that the CPU tier runs the host build of svs_fec.hpp on the same ones; and the channel
experiment of the README's table (tests/channel_lib.py's frames, seed and model of the channel)."""
import ctypes as C

import numpy as np

from testlib import build_emu

SEGMENT, OVERLAP, TAIL = 512, 64, 6
GENERATORS = {2: (0o133, 0o171), 3: (0o133, 0o171, 0o165)}
WEIGHT_MAX = 32767
START_OFF = -(1 << 30)


def coded_bits(n_info, rate):
    return rate * (n_info + TAIL)


def info_bits(capacity, rate):
    return max(capacity // rate - TAIL, 0)


def _parity(v):
    return bin(int(v)).count("1") & 1


# ---- the encoder --------------------------------------------------------------------------------------------------------------
def encode(info, rate):
    """0/1 per payload bit -> 0/1 per coded bit: start state 0, six zero tail bits, out_j = parity(reg & g_j)"""
    info = np.asarray(info, np.uint8).reshape(-1)
    out = np.empty(coded_bits(info.size, rate), np.uint8)
    s = 0
    for t, x in enumerate(list(info) + [0] * TAIL):
        reg = (int(x) << 6) | s
        for j, g in enumerate(GENERATORS[rate]):
            out[rate * t + j] = _parity(reg & g)
        s = reg >> 1
    assert s == 0
    return out


# ---- the weights ----------------------------------------------------------------------------------------------------------------
def weights_of_soft(soft):
    a = np.asarray(soft, np.uint8).astype(np.int64)
    return (2 * (a >> 7) - 1) * (2 * (a & 127) + 1)


def weights_of_int32(values):
    return np.clip(np.asarray(values, np.int32).astype(np.int64), -WEIGHT_MAX, WEIGHT_MAX)


def soft_of_bits(bits, margin=127):
    """a soft byte per bit: the hard bit in bit 7, `margin` (a number or one per bit) in bits 0..6"""
    return (np.asarray(bits, np.uint8) << 7 | np.asarray(margin, np.uint8)).astype(np.uint8)


# ---- the decoders -----------------------------------------------------------------------------------------------------------------
def _branch_signs(rate):
    """int64 [64, r]: for the new state ns, 2 out_j - 1 on the branch from p0 = 2 (ns & 31) with input ns >> 5"""
    sg = np.empty((64, rate), np.int64)
    for ns in range(64):
        reg = ((ns >> 5) << 6) | (2 * (ns & 31))
        for j, g in enumerate(GENERATORS[rate]):
            sg[ns, j] = 2 * _parity(reg & g) - 1
    return sg


_P0 = 2 * (np.arange(64) & 31)


def _window(w, rate, ws, we, n, a, counts):
    """add-compare-select over the steps [ws, we), traceback down to a -> the decoded bits of the steps [a, we)"""
    m = np.zeros(64, np.int64)
    if ws == 0:
        m[1:] = START_OFF
    dec = np.empty((we - ws, 64), np.uint8)
    branch = w[rate * ws: rate * we].reshape(we - ws, rate) @ _branch_signs(rate).T      # [steps, 64]: bm of every new state
    low = high = 0
    for t in range(ws, we):
        bm = branch[t - ws]
        c0, c1 = m[_P0] + bm, m[_P0 + 1] - bm
        d = c1 > c0                                          # p1 wins only when strictly larger
        if counts is not None:
            counts["ties"] = counts.get("ties", 0) + int((c1 == c0).sum())
            counts["steps"] = counts.get("steps", 0) + 1
        m = np.where(d, c1, c0)
        low, high = min(low, c0.min(), c1.min()), max(high, c0.max(), c1.max())
        dec[t - ws] = d
    assert -(1 << 31) < low and high < (1 << 30), "the header's bound: no candidate leaves int32"
    if we == n:
        s = 0
    else:
        s = int(np.argmax(m))                                # numpy's argmax: the first of the largest
        if counts is not None:
            counts["start_ties"] = counts.get("start_ties", 0) + int((m == m.max()).sum() > 1)
    bits = np.empty(we - a, np.uint8)
    for t in range(we - 1, a - 1, -1):
        bits[t - a] = s >> 5
        s = 2 * (s & 31) + int(dec[t - ws, s])
    return bits


def decode_windowed(weights, n_info, rate, counts=None):
    """THE FORMAT's decoder on integer weights (one per coded bit) -> 0/1 per payload bit.  counts (optional dict) receives
    `ties`, the compares with c1 = c0, `steps`, and `start_ties`, the windows whose traceback start was not unique."""
    w = np.asarray(weights, np.int64).reshape(-1)
    n = n_info + TAIL
    assert w.size == rate * n and np.abs(w).max(initial=0) <= WEIGHT_MAX
    out = np.zeros(n_info, np.uint8)
    for a in range(0, n, SEGMENT):
        b = min(a + SEGMENT, n)
        ws, we = max(a - OVERLAP, 0), min(b + OVERLAP, n)
        if a >= n_info:
            break                                            # tail steps only
        bits = _window(w, rate, ws, we, n, a, counts)[: b - a]
        keep = min(b, n_info) - a
        out[a: a + keep] = bits[:keep]
    return out


def decode_full(weights, n_info, rate):
    """the untruncated Viterbi, for comparison: one window over all n steps"""
    w = np.asarray(weights, np.int64).reshape(-1)
    n = n_info + TAIL
    return _window(w, rate, 0, n, n, 0, None)[:n_info]


def decode_soft(soft, n_info, rate, counts=None):
    return decode_windowed(weights_of_soft(soft), n_info, rate, counts)


def decode_int32(values, n_info, rate, counts=None):
    return decode_windowed(weights_of_int32(values), n_info, rate, counts)


# ---- what the GPU test runs (tests/test_fec_gpu.py); the CPU tier runs the host build of csrc/svs_fec.hpp on the same inputs ------
# one step past the tail; a window clamped at both ends (58: 64 steps, 59: 65); exactly one segment (506) and a second of one
# step (507); a last segment as long as the overlap and one step longer (570, 571); exactly two segments (1 018) and a third of
# one step (1 019); four segments and a bit (2 045); several workgroups with a ragged last one (37 segments: ten workgroups,
# the last with one wave)
N_INFOS = (1, 2, 58, 59, 506, 507, 570, 571, 1018, 1019, 2042 + 3, 4 * 512 * 9 + 77)
RATES = (2, 3)
SOFT_KINDS = ("clean", "flipped", "random", "all00", "all80")
INT32_KINDS = ("tally", "extremes")
INPUT_SEED = 23
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _rng(kind, n_info, rate):
    return np.random.default_rng([INPUT_SEED, n_info, rate, sum(map(ord, kind))])


def soft_input(kind, n_info, rate):
    """(soft bytes uint8 [n_coded], the info bits that were encoded or None)"""
    rng = _rng(kind, n_info, rate)
    nc = coded_bits(n_info, rate)
    if kind == "random":
        return rng.integers(0, 256, nc).astype(np.uint8), None
    if kind in ("all00", "all80"):                           # w = -1 / +1 everywhere: every compare away from step 0 a tie
        return np.full(nc, 0x00 if kind == "all00" else 0x80, np.uint8), None
    info = rng.integers(0, 2, n_info).astype(np.uint8)
    coded = encode(info, rate)
    margin = rng.integers(20, 128, nc)
    if kind == "flipped":                                    # 8 % of the coded bits flipped at |w| = 1
        flip = rng.random(nc) < 0.08
        coded = coded ^ flip.astype(np.uint8)
        margin = np.where(flip, 0, margin)
    return soft_of_bits(coded, margin), info


def int32_input(kind, n_info, rate):
    """(int32 weights [n_coded], info or None): `tally` - the sum of two noisy copies as the vote's tally holds them, with
    zeros; `extremes` - encoded info at large values with INT32_MIN, INT32_MAX and 0 sprinkled in"""
    rng = _rng(kind, n_info, rate)
    nc = coded_bits(n_info, rate)
    info = rng.integers(0, 2, n_info).astype(np.uint8)
    sign = 2 * encode(info, rate).astype(np.int64) - 1
    if kind == "tally":
        v = sum(2 * sign * np.where(rng.random(nc) < 0.1, -1, 1) * (2 * rng.integers(0, 128, nc) + 1) for _ in range(2))
        return v.astype(np.int32), info
    v = sign * rng.integers(1, 100_000, nc)
    pick = rng.integers(0, 12, nc)
    v = np.where(pick == 0, I32_MIN, np.where(pick == 1, I32_MAX, np.where(pick == 2, 0, v)))
    return v.astype(np.int32), info


_CASES = {}


def case(kind, n_info, rate):
    """(input array, info or None, the model's decoded bits) of one input of the GPU test, computed once per process"""
    key = (kind, n_info, rate)
    if key not in _CASES:
        values, info = soft_input(kind, n_info, rate) if kind in SOFT_KINDS else int32_input(kind, n_info, rate)
        want = decode_soft(values, n_info, rate) if kind in SOFT_KINDS else decode_int32(values, n_info, rate)
        for a in (values, want):
            a.setflags(write=False)
        _CASES[key] = (values, info, want)
    return _CASES[key]


# ---- the host build of csrc/svs_fec.hpp (tests/hostemu/fec_emu.cpp) --------------------------------------------------------------
_DECODE = (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p])
PROTOTYPES = {"fec_emu_decode_soft": _DECODE, "fec_emu_decode_weights": _DECODE}


def emu(build_dir=None):
    """tests/hostemu/fec_emu.cpp, compiled once per process with g++ as the other host emulations are"""
    return build_emu("fec_emu.cpp", PROTOTYPES, build_dir)


def emu_decode(values, n_info, rate, build_dir=None):
    """the host build's decoder on soft bytes (uint8) or int32 weights -> 0/1 per payload bit"""
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.uint8, np.int32) and values.size == coded_bits(n_info, rate)
    out = np.full((n_info + 7) // 8, 0xEE, np.uint8)
    fn = emu(build_dir).fec_emu_decode_soft if values.dtype == np.uint8 else emu(build_dir).fec_emu_decode_weights
    assert fn(values.ctypes.data, n_info, rate, out.ctypes.data) == 0
    return np.unpackbits(out, count=n_info)


# ---- the README's table: a coded stream through the requantisation channel ------------------------------------------------------
def coded_clip(rate, n_ac=10, seed=None, n_info=None):
    """(cover, info): channel_lib.survival's three frames of noise in [64, 192) and, drawn behind them from the same generator,
    n_info random payload bits (None: as many as the frames' capacity holds at `rate`)"""
    import channel_lib as cl
    rng = np.random.default_rng(cl.SURVIVAL_SEED if seed is None else seed)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    n_info = info_bits(f * (h // 8) * (w // 8) * n_ac, rate) if n_info is None else n_info
    return cover, rng.integers(0, 2, n_info).astype(np.uint8)


def coded_survival(rate, quality, delta=20, n_ac=10, steps=None, seed=None):
    """channel_lib.survival's cover, seed and frames with a coded stream in the place of the three copies: random info of
    info_bits(capacity of the three frames, rate) bits, encoded, embedded over the three frames by the oracle (reference rule;
    steps: a step table, the stepped model), requantised by the model of the channel at `quality`, read as soft bytes by the
    model -> dict(n_info, coded_wrong: wrong coded bits before decoding, soft: wrong payload bits decoding the soft bytes,
    hard: decoding the hard bits alone (margin 0: w = +-1), full: the untruncated Viterbi on the soft bytes)"""
    import channel_lib as cl
    import soft_lib as sl
    from svsdct import channel
    cover, info = coded_clip(rate, n_ac, seed)
    f, h, w = cover.shape
    per_frame = (h // 8) * (w // 8) * n_ac
    n_info = info.size
    coded = encode(info, rate)
    stream = np.zeros(f * per_frame, np.uint8)
    stream[: coded.size] = coded
    table = channel.quality_steps(quality)
    if steps is None:
        stego = np.stack([cl.model_stego(cover[i: i + 1], delta, n_ac, stream[i * per_frame: (i + 1) * per_frame])[0] for i in range(f)])
        soft = sl.model_batch_soft(cl.model_requantise(stego, table), delta, n_ac)
    else:
        import stepped_lib as st
        import stepped_soft_lib as ssl
        stego = np.stack([st.model_embed(cover[i], steps, stream[i * per_frame: (i + 1) * per_frame], n_ac)[0] for i in range(f)])
        soft = np.concatenate([ssl.model_soft(g, steps, n_ac) for g in cl.model_requantise(stego, table)])
    soft = soft[: coded.size]
    hard = soft >> 7
    wrong = lambda bits: int((bits != info).sum())   # noqa: E731
    return dict(n_info=n_info, coded_wrong=int((hard != coded).sum()), soft=wrong(decode_soft(soft, n_info, rate)),
                hard=wrong(decode_soft(soft_of_bits(hard, 0), n_info, rate)), full=wrong(decode_full(weights_of_soft(soft), n_info, rate)))
