"""The NumPy model of the punctured codes, written from the text of include/svsfec.h ("Punctured codes") and not from
csrc/svs_fec.hpp: the pattern table, S(t), the lengths, the encoder as tests/fec_lib.py's rate-2 encoder under a mask, the
depuncturer (one weight per sent bit -> one per mother bit, zeros at the unsent ones) in front of fec_lib.decode_windowed at
rate 2; the inputs of tests/test_fec_punctured_gpu.py, built as fec_lib's are, so that the CPU tier runs the host build
(tests/hostemu/fec_punctured_emu.cpp) on the same ones; and the channel experiment of the README's punctured table."""
import ctypes as C

import numpy as np

import fec_lib as fl
from testlib import build_emu

CODES = (23, 34, 56, 78)
# code -> (out_0 sent, out_1 sent) over the P steps of a period
PATTERNS = {
    23: ("11", "10"),
    34: ("110", "101"),
    56: ("11010", "10101"),
    78: ("1111010", "1000101"),
}
NAMES = {23: "2/3", 34: "3/4", 56: "5/6", 78: "7/8"}


def period(code):
    """(P, K, pre): pre[i] = the sent bits of the steps 0 .. i - 1 of a period"""
    out0, out1 = PATTERNS[code]
    per_step = [int(a) + int(b) for a, b in zip(out0, out1)]
    return len(out0), sum(per_step), [sum(per_step[:i]) for i in range(len(out0))]


def S(t, code):
    """the sent bits before step t"""
    p, k, pre = period(code)
    return (t // p) * k + pre[t % p]


def coded_bits(n_info, code):
    return S(n_info + fl.TAIL, code)


def steps_that_fit(capacity, code):
    """the largest n with S(n) <= capacity, found by bisection: S is strictly increasing"""
    lo, hi = 0, capacity + 1                                 # S(lo) <= capacity < S(hi): S(t) >= t
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if S(mid, code) <= capacity else (lo, mid)
    return lo


def info_bits(capacity, code):
    """steps_that_fit minus 6; 0 when that is not positive"""
    return max(steps_that_fit(capacity, code) - fl.TAIL, 0)


def mask(n, code):
    """bool [2 n]: mother bit 2 t + j is sent"""
    out0, out1 = PATTERNS[code]
    p = len(out0)
    m = np.empty(2 * n, bool)
    m[0::2] = [out0[t % p] == "1" for t in range(n)]
    m[1::2] = [out1[t % p] == "1" for t in range(n)]
    return m


def encode(info, code):
    info = np.asarray(info, np.uint8).reshape(-1)
    return fl.encode(info, 2)[mask(info.size + fl.TAIL, code)]


def depuncture(weights, n_info, code):
    """one weight per sent bit -> int64 [2 n]: the weight of its sent bit where mother bit 2 t + j was sent, 0 where not"""
    n = n_info + fl.TAIL
    w = np.asarray(weights, np.int64).reshape(-1)
    assert w.size == coded_bits(n_info, code)
    full = np.zeros(2 * n, np.int64)
    full[mask(n, code)] = w
    return full


def decode(weights, n_info, code, counts=None):
    return fl.decode_windowed(depuncture(weights, n_info, code), n_info, 2, counts)


def decode_soft(soft, n_info, code):
    return decode(fl.weights_of_soft(soft), n_info, code)


def decode_int32(values, n_info, code):
    return decode(fl.weights_of_int32(values), n_info, code)


# ---- what the GPU test runs ---------------------------------------------------------------------------------------------------
# fec_lib's lengths: at least three segments, windows that start at 448 and 960 (every ws mod P, not 0 at P = 7), a ragged last
# workgroup; and 1 019 .. 1 025, where (n_info + 6) mod 7 takes every residue (and mod 2, 3 and 5 too)
N_INFOS = tuple(sorted(set(fl.N_INFOS) | set(range(1019, 1026))))
LARGEST = max(N_INFOS)
KINDS = ("flipped", "random", "all80", "tally")
LARGEST_KINDS = ("random", "tally")


def lengths(kind):
    return tuple(n for n in N_INFOS if n != LARGEST or kind in LARGEST_KINDS)


def _rng(kind, n_info, code):
    return np.random.default_rng([fl.INPUT_SEED, n_info, code, sum(map(ord, kind))])


def soft_input(kind, n_info, code):
    """fec_lib.soft_input for a punctured stream: (soft bytes uint8 [n_sent], the info bits that were encoded or None)"""
    rng = _rng(kind, n_info, code)
    nc = coded_bits(n_info, code)
    if kind == "random":
        return rng.integers(0, 256, nc).astype(np.uint8), None
    if kind == "all80":
        return np.full(nc, 0x80, np.uint8), None
    assert kind == "flipped"
    info = rng.integers(0, 2, n_info).astype(np.uint8)
    coded = encode(info, code)
    flip = rng.random(nc) < 0.08                             # 8 % of the sent bits flipped at |w| = 1, as fec_lib does
    margin = np.where(flip, 0, rng.integers(20, 128, nc))
    return fl.soft_of_bits(coded ^ flip.astype(np.uint8), margin), info


def int32_input(kind, n_info, code):
    """fec_lib.int32_input's `tally`: the sum of two noisy copies as the vote's tally holds them, with zeros"""
    assert kind == "tally"
    rng = _rng(kind, n_info, code)
    nc = coded_bits(n_info, code)
    info = rng.integers(0, 2, n_info).astype(np.uint8)
    sign = 2 * encode(info, code).astype(np.int64) - 1
    v = sum(2 * sign * np.where(rng.random(nc) < 0.1, -1, 1) * (2 * rng.integers(0, 128, nc) + 1) for _ in range(2))
    return v.astype(np.int32), info


_CASES = {}


def case(kind, n_info, code):
    """(input array, info or None, the model's decoded bits, the model's depunctured weights as int32 [2 n]), once per process"""
    key = (kind, n_info, code)
    if key not in _CASES:
        values, info = int32_input(kind, n_info, code) if kind == "tally" else soft_input(kind, n_info, code)
        weights = fl.weights_of_int32(values) if kind == "tally" else fl.weights_of_soft(values)
        mother = depuncture(weights, n_info, code)
        want = fl.decode_windowed(mother, n_info, 2)
        mother = mother.astype(np.int32)
        for a in (values, want, mother):
            a.setflags(write=False)
        _CASES[key] = (values, info, want, mother)
    return _CASES[key]


# ---- the host build (tests/hostemu/fec_punctured_emu.cpp) -----------------------------------------------------------------------
_U64 = C.c_uint64
PROTOTYPES = {
    "fec_punctured_emu_decode_soft": (C.c_int, [C.c_void_p, _U64, C.c_int, C.c_void_p]),
    "fec_punctured_emu_decode_weights": (C.c_int, [C.c_void_p, _U64, C.c_int, C.c_void_p]),
    "fec_punctured_emu_sent_before": (_U64, [_U64, C.c_int]),
    "fec_punctured_emu_steps_that_fit": (_U64, [_U64, C.c_int]),
}


def emu(build_dir=None):
    """tests/hostemu/fec_punctured_emu.cpp, compiled once per process with g++ as the other host emulations are"""
    return build_emu("fec_punctured_emu.cpp", PROTOTYPES, build_dir)


def emu_decode(values, n_info, code, build_dir=None):
    """the host build's decoder on n_sent soft bytes (uint8) or int32 weights -> 0/1 per payload bit"""
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.uint8, np.int32) and values.size == coded_bits(n_info, code)
    out = np.full((n_info + 7) // 8, 0xEE, np.uint8)
    lib = emu(build_dir)
    fn = lib.fec_punctured_emu_decode_soft if values.dtype == np.uint8 else lib.fec_punctured_emu_decode_weights
    assert fn(values.ctypes.data, n_info, code, out.ctypes.data) == 0
    return np.unpackbits(out, count=n_info)


# ---- the README's table: a punctured stream through the requantisation channel --------------------------------------------------
def coded_clip(code, n_ac=10, n_info=None):
    """fec_lib.coded_clip with the payload length of a punctured code: (cover, info)"""
    import channel_lib as cl
    f, h, w = cl.SURVIVAL_SHAPE
    return fl.coded_clip(2, n_ac, n_info=info_bits(f * (h // 8) * (w // 8) * n_ac, code) if n_info is None else n_info)


def coded_survival(code, quality, delta=20, n_ac=10):
    """fec_lib.coded_survival for a punctured code (reference rule, one step): dict(n_info, coded_wrong: wrong sent bits before
    decoding, soft: wrong payload bits decoding the soft bytes, hard: decoding the hard bits alone)"""
    import channel_lib as cl
    import soft_lib as sl
    from svsdct import channel
    cover, info = coded_clip(code, n_ac)
    f, h, w = cover.shape
    per_frame = (h // 8) * (w // 8) * n_ac
    coded = encode(info, code)
    stream = np.zeros(f * per_frame, np.uint8)
    stream[: coded.size] = coded
    stego = np.stack([cl.model_stego(cover[i: i + 1], delta, n_ac, stream[i * per_frame: (i + 1) * per_frame])[0] for i in range(f)])
    soft = sl.model_batch_soft(cl.model_requantise(stego, channel.quality_steps(quality)), delta, n_ac)[: coded.size]
    hard = soft >> 7
    wrong = lambda bits: int((bits != info).sum())   # noqa: E731
    return dict(n_info=info.size, coded_wrong=int((hard != coded).sum()), soft=wrong(decode_soft(soft, info.size, code)),
                hard=wrong(decode_soft(fl.soft_of_bits(hard, 0), info.size, code)))
