"""The convolutional code and its soft-decision Viterbi decoder (libsvsfec.so, include/svsfec.h): a constraint-length-7 code
at rate 1/2 (generators 133, 171) or 1/3 (133, 171, 165), six zero tail bits, decoded on the device by a windowed Viterbi from
one soft byte (svs_soft_extract) or one int32 (an entry of svs_soft_vote's tally) per coded bit.  `rate` is a code: 2, 3, or
one of PUNCTURED = (23, 34, 56, 78) - the rate-1/2 code at rate 2/3, 3/4, 5/6 or 7/8, some coded bits not sent (PATTERNS); the
decoder then takes one value per SENT bit and gives the unsent ones the weight 0.

    coded = encode(info_bits, rate)                          host: 0/1 per coded bit
    ... embed `coded`, let the channel do its worst, soft-extract ...
    info = decode_soft(soft_bytes, n_info, rate)             device: 0/1 per payload bit

batch.embed_coded_frames / batch.extract_coded_frames wrap both ends around the frame calls and keep the soft bytes on the device.
The library is loaded on first use; SVSFEC_LIB overrides its path.  There is no CPU fallback for the decoder.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import native
from .staging import Staged

LIB_PATH = os.environ.get("SVSFEC_LIB", os.path.join(native._PKG_DIR, "lib", "libsvsfec.so"))
ABI_VERSION = 1
RATES = (2, 3)
RATE_2_3, RATE_3_4, RATE_5_6, RATE_7_8 = PUNCTURED = (23, 34, 56, 78)
# code -> (out_0 sent, out_1 sent) for the steps of a period (include/svsfec.h, "Punctured codes")
PATTERNS = {
    RATE_2_3: ((1, 1), (1, 0)),
    RATE_3_4: ((1, 1, 0), (1, 0, 1)),
    RATE_5_6: ((1, 1, 0, 1, 0), (1, 0, 1, 0, 1)),
    RATE_7_8: ((1, 1, 1, 1, 0, 1, 0), (1, 0, 0, 0, 1, 0, 1)),
}
SEGMENT, OVERLAP, TAIL = 512, 64, 6
MAX_INFO_BITS = 1 << 40

_u8p = C.c_void_p
# name -> (restype, argtypes); every symbol include/svsfec.h declares
SIGNATURES = {
    "svs_fec_abi_version": (C.c_int, []),
    "svs_fec_last_error": (C.c_char_p, []),
    "svs_fec_coded_bits": (C.c_uint64, [C.c_uint64, C.c_int]),
    "svs_fec_info_bits": (C.c_uint64, [C.c_uint64, C.c_int]),
    "svs_fec_encode": (C.c_int, [_u8p, C.c_uint64, C.c_int, _u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "svs_fec_decode_soft_dev": (C.c_int, [_u8p, C.c_uint64, C.c_int, _u8p, C.c_uint64, C.c_void_p]),
    "svs_fec_decode_weights_dev": (C.c_int, [_u8p, C.c_uint64, C.c_int, _u8p, C.c_uint64, C.c_void_p]),
}

load, check = native.bind(globals(), "svs_fec")


def _rate(rate) -> int:
    if isinstance(rate, bool) or rate not in RATES + PUNCTURED:
        raise ValueError(f"rate {rate!r}: 2 (rate 1/2), 3 (rate 1/3) or a punctured code 23, 34, 56, 78 (rate 2/3 .. 7/8)")
    return int(rate)


def _period(rate: int):
    """(P, K, pre): the period of a punctured code, its sent bits, and pre[i], those of its steps 0 .. i - 1"""
    out0, out1 = PATTERNS[rate]
    pre = [0]
    for a, b in zip(out0, out1):
        pre.append(pre[-1] + a + b)
    return len(out0), pre[-1], pre[:-1]


def sent_before(t: int, rate: int) -> int:
    """S(t): the bits a punctured code sends before step t"""
    p, k, pre = _period(_rate(rate))
    return t // p * k + pre[t % p]


def _n_info(n_info) -> int:
    n_info = int(n_info)
    if not 0 <= n_info <= MAX_INFO_BITS:
        raise ValueError(f"n_info {n_info} outside 0 .. 2**40")
    return n_info


def coded_bits(n_info: int, rate: int = 2) -> int:
    """rate * (n_info + 6), under a punctured code S(n_info + 6): the coded bits sent for n_info payload bits"""
    rate, n = _rate(rate), _n_info(n_info) + TAIL
    return sent_before(n, rate) if rate in PUNCTURED else rate * n


def info_bits(capacity_bits: int, rate: int = 2) -> int:
    """capacity // rate - 6, under a punctured code (the largest n with S(n) <= capacity) - 6; at least 0: the largest payload
    whose coded stream fits capacity_bits"""
    rate, cap = _rate(rate), int(capacity_bits)
    if rate not in PUNCTURED:
        return max(cap // rate - TAIL, 0)
    p, k, pre = _period(rate)
    return max(cap // k * p + max(i for i in range(p) if pre[i] <= cap % k) - TAIL, 0)


def _step_holding(x: int, rate: int) -> int:
    """the largest t with S(t) <= x: the step that sends bit x"""
    if rate not in PUNCTURED:
        return x // rate
    p, k, pre = _period(rate)
    return x // k * p + max(i for i in range(p) if pre[i] <= x % k)


def steps_of_sent_bits(lo: int, hi: int, rate: int = 2):
    """(t0, t1): the trellis steps t0 .. t1 - 1 whose sent bits touch the range [lo, hi) of the coded stream, lo < hi.  Rates 2 and
    3: t0 = lo // rate, t1 = ceil(hi / rate); a punctured code: S(t) of include/svsfec.h inverted.  Payload bit t is the input
    of step t, so these are also the payload bits that a damaged stretch of the coded stream bears on most directly (the six
    tail steps lie behind the payload)."""
    rate, lo, hi = _rate(rate), int(lo), int(hi)
    if not 0 <= lo < hi:
        raise ValueError(f"[{lo}, {hi}) is no range of sent bits")
    return _step_holding(lo, rate), _step_holding(hi - 1, rate) + 1


def encode(bits, rate: int = 2) -> np.ndarray:
    """Payload bits (0/1 per entry) -> the coded stream, uint8 0/1 per coded bit (svs_fec_encode; host code, no GPU)."""
    rate = _rate(rate)
    b = np.asarray(bits, np.uint8).reshape(-1)
    if b.size == 0:
        return np.zeros(0, np.uint8)
    packed = np.packbits(b)
    n_coded = coded_bits(b.size, rate)
    out = np.empty((n_coded + 7) // 8, np.uint8)
    got = C.c_uint64(0)
    check(load().svs_fec_encode(packed.ctypes.data, b.size, rate, out.ctypes.data, out.size, C.byref(got)), "svs_fec_encode")
    assert got.value == n_coded
    return np.unpackbits(out, count=n_coded)


def decode_soft_device(d_soft: int, n_info: int, rate: int, d_info_packed_out: int, out_capacity_bytes: int, stream: int = 0) -> None:
    """Enqueue the decoder on `stream` (svs_fec_decode_soft_dev): coded_bits(n_info, rate) soft bytes at d_soft, coded bit i
    (under a punctured code: sent bit i) in byte i, -> ceil(n_info / 8) packed bytes at d_info_packed_out."""
    check(load().svs_fec_decode_soft_dev(d_soft, _n_info(n_info), _rate(rate), d_info_packed_out, int(out_capacity_bytes),
                                         stream or None), "svs_fec_decode_soft_dev")


def decode_weights_device(d_weights: int, n_info: int, rate: int, d_info_packed_out: int, out_capacity_bytes: int,
                          stream: int = 0) -> None:
    """Enqueue the decoder on `stream` (svs_fec_decode_weights_dev): coded_bits(n_info, rate) int32 weights (4-byte aligned, each
    clamped to +-32767; the tally of svs_soft_vote_dev at period = n_coded) -> ceil(n_info / 8) packed bytes."""
    check(load().svs_fec_decode_weights_dev(d_weights, _n_info(n_info), _rate(rate), d_info_packed_out, int(out_capacity_bytes),
                                            stream or None), "svs_fec_decode_weights_dev")


def _decode_staged(values: np.ndarray, n_info: int, rate: int, device: int, call) -> np.ndarray:
    n_info, rate = _n_info(n_info), _rate(rate)
    if values.ndim != 1 or values.size != coded_bits(n_info, rate):
        raise ValueError(f"{values.size} values are not the {coded_bits(n_info, rate)} coded bits of n_info = {n_info} at rate {rate}")
    if n_info == 0:
        return np.zeros(0, np.uint8)
    load()
    out_bytes = (n_info + 7) // 8
    with Staged(device) as dev:
        d_in, d_out = dev.upload(np.ascontiguousarray(values)), dev.alloc(out_bytes)
        call(d_in, n_info, rate, d_out, out_bytes)
        packed = dev.download(d_out, out_bytes)
        dev.synchronise()
    return np.unpackbits(packed, count=n_info)


def decode_soft(soft_bytes, n_info: int, rate: int = 2, device: int = 0) -> np.ndarray:
    """Decode soft bytes held on the host: staged through svs_malloc / svs_memcpy_*, decoded by svs_fec_decode_soft_dev.
    soft_bytes: uint8 [coded_bits(n_info, rate)].  Returns uint8 0/1 [n_info]."""
    a = np.asarray(soft_bytes)
    if a.dtype != np.uint8:
        raise TypeError("soft_bytes must be uint8: one byte per coded bit (svs_soft_extract)")
    return _decode_staged(a, n_info, rate, device, decode_soft_device)


def decode_weights(weights, n_info: int, rate: int = 2, device: int = 0) -> np.ndarray:
    """decode_soft for int32 weights held on the host (svs_fec_decode_weights_dev): a tally of svs_soft_vote, or any integers
    whose sign is the bit and whose size is the confidence."""
    a = np.asarray(weights)
    if a.dtype != np.int32:
        raise TypeError("weights must be int32: one value per coded bit (soft.tally)")
    return _decode_staged(a, n_info, rate, device, decode_weights_device)
