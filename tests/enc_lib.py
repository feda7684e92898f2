"""The inputs and the expectations of the device encoders' tests (include/svsenc.h, libsvsenc.so, svsdct/enc.py).  The encoders
define no format, so every expectation is something that exists and is pinned already: the NumPy models of the two codes
(fec_lib.encode, fec_punctured_lib.encode, rs_lib.encode), soft.tile, and the host encoders svs_fec_encode / svs_rs_encode.  The
CPU tier runs the host build of csrc/svs_enc.hpp (tests/hostemu/enc_emu.cpp) on the lengths the GPU tier runs the kernels on;
and, for positions no buffer reaches, the parity formula of include/svsfec.h evaluated bit by bit on a synthetic stream."""
import ctypes as C

import numpy as np

import fec_lib as fl
import fec_punctured_lib as fpl
import rs_lib as rl
from testlib import build_emu
from svsdct import fec, rs, soft

RATES = (2, 3, 23, 34, 56, 78)
# the steps a lane takes at each rate code (svsenc::FecUnit) and the sent bits they make
UNIT_STEPS = {2: 16, 34: 24, 78: 28, 3: 32, 23: 64, 56: 80}
UNIT_BITS = {2: 32, 34: 32, 78: 32, 3: 96, 23: 96, 56: 96}
# the decoder tests' lengths (the largest 4 * 512 * 9 + 77); lengths round a byte and a dword of info; and n = n_info + 6 one step
# either side of every rate's unit and of the 64 units of a wave
N_INFOS = tuple(sorted(set(fpl.N_INFOS) | {7, 8, 9, 25, 26, 31, 32, 33}
                       | {s * m - fl.TAIL + e for s in UNIT_STEPS.values() for m in (1, 64) for e in (-1, 0, 1)}))
LARGEST = 4 * 512 * 9 + 77
KS = rl.KS
PERIODS = (1, 7, 14, 31, 32, 33, 4794)
INPUT_SEED = 61
TAPS = ((0, 2, 3, 5, 6), (0, 1, 2, 3, 6), (0, 1, 2, 4, 6))          # out_j[t] = xor of x[t - d] over these d (133, 171, 165)


def tile_lengths(period):
    return tuple(n for n in (period - 1, period, period + 1, 3 * period + 5) if n > 0)


_INFO, _CODED, _DATA, _STREAM, _BITS = {}, {}, {}, {}, {}


def info(n_info):
    """the payload bits of one length, 0/1 per bit"""
    if n_info not in _INFO:
        _INFO[n_info] = np.random.default_rng([INPUT_SEED, n_info]).integers(0, 2, n_info).astype(np.uint8)
        _INFO[n_info].setflags(write=False)
    return _INFO[n_info]


def packed_info(n_info):
    """numpy.packbits of info(n_info) with ONES in the pad bits of the last byte: no encoder may read them"""
    p = np.packbits(info(n_info))
    if n_info % 8:
        p[-1] |= 0xFF >> (n_info % 8)
    return p


def coded(n_info, rate):
    """the model's coded stream, packed: what every encoder must write, the pad bits 0; computed once per process"""
    key = (n_info, rate)
    if key not in _CODED:
        bits = (fpl if rate in fpl.CODES else fl).encode(info(n_info), rate)
        assert bits.size == fec.coded_bits(n_info, rate)
        _CODED[key] = np.packbits(bits)
        _CODED[key].setflags(write=False)
    return _CODED[key]


def data(k):
    if k not in _DATA:
        _DATA[k] = np.random.default_rng([INPUT_SEED, k, 1]).integers(0, 256, k).astype(np.uint8)
        _DATA[k].setflags(write=False)
    return _DATA[k]


def stream(k):
    """the host encoder's stream of data(k) (tests/test_rs_cpu.py pins it to the model), once per process"""
    if k not in _STREAM:
        _STREAM[k] = rs.encode_array(data(k))
        _STREAM[k].setflags(write=False)
    return _STREAM[k]


def tile_bits(period):
    if period not in _BITS:
        _BITS[period] = np.random.default_rng([INPUT_SEED, period, 2]).integers(0, 2, period).astype(np.uint8)
        _BITS[period].setflags(write=False)
    return _BITS[period]


def packed_tile_bits(period):
    p = np.packbits(tile_bits(period))
    if period % 8:
        p[-1] |= 0xFF >> (period % 8)
    return p


def tiled(period, n_out):
    return np.packbits(soft.tile(tile_bits(period), n_out))


# ---- the synthetic stream of enc_emu.cpp and the formats evaluated on it bit by bit ---------------------------------------------------
def hashed_byte(i):
    return (((i + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 56


def hashed_bit(t, n_bits):
    """bit t of the synthetic stream's first n_bits bits, 0 outside them"""
    return (hashed_byte(t >> 3) >> (7 - (t & 7))) & 1 if 0 <= t < n_bits else 0


def sent_bit(g, n_info, rate):
    """sent bit g of the coded stream of the synthetic stream's first n_info bits, from include/svsfec.h: the step and the output
    that bit g is, then the parity of the output's taps.  A bit at or behind the stream's end is 0"""
    if g >= fec.coded_bits(n_info, rate):
        return 0
    if rate in (2, 3):
        t, j = divmod(g, rate)
    else:
        t = fec._step_holding(g, rate)
        out0, out1 = fec.PATTERNS[rate]
        i = t % len(out0)
        j = [j for j, row in enumerate((out0, out1)) if row[i]][g - fec.sent_before(t, rate)]
    return sum(hashed_bit(t - d, n_info) for d in TAPS[j]) & 1


def unit_words(u, n_info, rate):
    """the dwords of unit u of that stream, the first sent bit in bit 31 of the first"""
    first = u * UNIT_BITS[rate]
    return [sum(sent_bit(first + 32 * w + b, n_info, rate) << (31 - b) for b in range(32)) for w in range(UNIT_BITS[rate] // 32)]


def tile_word(d, period, n_out):
    return sum((hashed_bit((32 * d + b) % period, period) if 32 * d + b < n_out else 0) << (31 - b) for b in range(32))


# ---- the host build of csrc/svs_enc.hpp (tests/hostemu/enc_emu.cpp) -------------------------------------------------------------------
_U64, _P = C.c_uint64, C.c_void_p
PROTOTYPES = {
    "enc_emu_fec_encode": (C.c_int, [_P, _U64, C.c_int, _P]),
    "enc_emu_fec_unit_hashed": (C.c_int, [_U64, C.c_int, _U64, _P]),
    "enc_emu_unit_steps": (C.c_int, [C.c_int]),
    "enc_emu_hashed_byte": (C.c_uint32, [_U64]),
    "enc_emu_rs_encode": (C.c_int, [_P, _U64, _P]),
    "enc_emu_tile": (C.c_int, [_P, _U64, _P, _U64]),
    "enc_emu_tile_dword_hashed": (C.c_uint32, [_U64, _U64, _U64]),
}


def emu(build_dir=None):
    """tests/hostemu/enc_emu.cpp, compiled once per process with g++ as the other host emulations are"""
    return build_emu("enc_emu.cpp", PROTOTYPES, build_dir)


GUARD = 16
SENTINEL = 0xA5


def emu_fec_encode(n_info, rate, build_dir=None):
    src = packed_info(n_info)
    nbytes = (fec.coded_bits(n_info, rate) + 7) // 8
    out = np.full(nbytes + GUARD, SENTINEL, np.uint8)
    assert emu(build_dir).enc_emu_fec_encode(src.ctypes.data, n_info, rate, out.ctypes.data) == 0
    assert (out[nbytes:] == SENTINEL).all(), "the emulation wrote behind the coded stream"
    return out[:nbytes]


def emu_rs_encode(k, in_place, build_dir=None):
    total = rl.coded_bytes(k)
    out = np.full(total + GUARD, SENTINEL, np.uint8)
    src = data(k).copy()
    if in_place:
        out[:k] = src
    assert emu(build_dir).enc_emu_rs_encode(out.ctypes.data if in_place else src.ctypes.data, k, out.ctypes.data) == 0
    assert (out[total:] == SENTINEL).all() and np.array_equal(src, data(k))
    return out[:total]


def emu_tile(period, n_out, build_dir=None):
    src = packed_tile_bits(period)
    nbytes = (n_out + 7) // 8
    out = np.full(nbytes + GUARD, SENTINEL, np.uint8)
    assert emu(build_dir).enc_emu_tile(src.ctypes.data, period, out.ctypes.data, n_out) == 0
    assert (out[nbytes:] == SENTINEL).all(), "the emulation wrote behind the tiled stream"
    return out[:nbytes]
