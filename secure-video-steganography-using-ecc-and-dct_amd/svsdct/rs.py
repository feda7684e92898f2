"""The Reed-Solomon outer code (libsvsrs.so, include/svsrs.h): RS(255, 223) over GF(2^8), shortened, byte-interleaved over all
its codewords, decoded on the device in place - up to 16 wrong bytes a codeword corrected, and a status byte a codeword that
says how many were, or 255: not decodable, left as received.  It sits behind the Viterbi decoder of svsdct/fec.py, whose packed
output bytes are its input.

    stream = encode(data)                                    host: data + 32 parity bytes per 223 data bytes
    ... fec.encode, embed, the channel, soft extract, Viterbi ...
    data, status = decode(stream, len(data))                 device

batch.embed_coded_frames / batch.extract_coded_frames take outer=True and keep everything between the soft extract and the
status bytes on the device.  The library is loaded on first use; SVSRS_LIB overrides its path.  There is no CPU decoder.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import fec as _fec
from . import native
from .staging import Staged

LIB_PATH = os.environ.get("SVSRS_LIB", os.path.join(native._PKG_DIR, "lib", "libsvsrs.so"))
ABI_VERSION = 1
CODEWORD, DATA, PARITY, T = 255, 223, 32, 16
UNCORRECTABLE = 255
MAX_DATA_BYTES = 1 << 37

_p = C.c_void_p
# name -> (restype, argtypes); every symbol include/svsrs.h declares
SIGNATURES = {
    "svs_rs_abi_version": (C.c_int, []),
    "svs_rs_last_error": (C.c_char_p, []),
    "svs_rs_codewords": (C.c_uint64, [C.c_uint64]),
    "svs_rs_coded_bytes": (C.c_uint64, [C.c_uint64]),
    "svs_rs_data_bytes": (C.c_uint64, [C.c_uint64]),
    "svs_rs_encode": (C.c_int, [_p, C.c_uint64, _p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "svs_rs_decode_dev": (C.c_int, [_p, C.c_uint64, _p, C.c_uint64, _p, C.c_void_p]),
}

load, check = native.bind(globals(), "svs_rs")


def _k(k) -> int:
    k = int(k)
    if not 0 <= k <= MAX_DATA_BYTES:
        raise ValueError(f"k {k} outside 0 .. 2**37")
    return k


def codewords(k: int) -> int:
    """C = ceil(k / 223): the codewords that k data bytes are interleaved over"""
    return -(-_k(k) // DATA)


def coded_bytes(k: int) -> int:
    """k + 32 C: the bytes of the stream of k data bytes"""
    return _k(k) + PARITY * codewords(k)


def data_bytes(total_bytes: int) -> int:
    """the largest k whose stream fits total_bytes; 0 when there is none"""
    total = int(total_bytes)
    if total < 0:
        raise ValueError("total_bytes is negative")
    return min(total // CODEWORD * DATA + max(total % CODEWORD - PARITY, 0), MAX_DATA_BYTES)


def payload_bits(capacity_bits: int, rate: int = 2) -> int:
    """the payload bits that `capacity_bits` carry under both codes: 8 data_bytes(fec.info_bits(capacity_bits, rate) // 8)"""
    return 8 * data_bytes(_fec.info_bits(capacity_bits, rate) // 8)


def _bytes(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), np.uint8)
    a = np.asarray(data)
    if a.dtype != np.uint8:
        raise TypeError("the outer code takes bytes: a bytes object or a uint8 array")
    return np.ascontiguousarray(a.reshape(-1))


def encode_array(data) -> np.ndarray:
    """encode on a uint8 array -> uint8 [coded_bytes(k)] (svs_rs_encode; host code, no GPU)"""
    d = _bytes(data)
    k = _k(d.size)
    out = np.empty(coded_bytes(k), np.uint8)
    if k == 0:
        return out
    got = C.c_uint64(0)
    check(load().svs_rs_encode(d.ctypes.data, k, out.ctypes.data, out.size, C.byref(got)), "svs_rs_encode")
    assert got.value == out.size
    return out


def encode(data) -> bytes:
    """k data bytes -> the stream: the data itself, then 32 C interleaved parity bytes"""
    return encode_array(data).tobytes()


def decode_device(d_stream: int, k: int, d_status: int, status_capacity: int, d_counts: int = 0, stream: int = 0) -> None:
    """Enqueue the decoder on `stream` (svs_rs_decode_dev): coded_bytes(k) bytes at d_stream, any alignment, decoded in place;
    codewords(k) status bytes to d_status; d_counts: 0 or a 4-byte aligned uint32[2] that the call adds to."""
    check(load().svs_rs_decode_dev(d_stream, _k(k), d_status, int(status_capacity), d_counts or None, stream or None), "svs_rs_decode_dev")


def _decode_staged(stream, k: int, erased, device: int, load_lib, launch):
    """The staged call that decode and rse.decode share: the stream (and the mask, if there is one) up through svs_malloc /
    svs_memcpy_*, launch(d_stream, k, d_erased or 0, d_status, codewords(k)), the data bytes and the status bytes down."""
    s = _bytes(stream)
    k = _k(k)
    if s.size != coded_bytes(k):
        raise ValueError(f"{s.size} bytes are not the {coded_bytes(k)} of a stream of k = {k}")
    m = None if erased is None else _bytes(erased)
    if m is not None and m.size != s.size:
        raise ValueError(f"{m.size} mask bytes are not the {s.size} of the stream")
    if k == 0:
        return b"", np.zeros(0, np.uint8)
    load_lib()
    n_cw = codewords(k)
    with Staged(device) as dev:
        d_stream, d_status = dev.upload(s), dev.alloc(n_cw)
        launch(d_stream, k, 0 if m is None else dev.upload(m), d_status, n_cw)
        data, status = dev.download(d_stream, k), dev.download(d_status, n_cw)
        dev.synchronise()
    return data.tobytes(), status


def decode(stream, k: int, device: int = 0):
    """Decode a stream held on the host: staged through svs_malloc / svs_memcpy_*, decoded by svs_rs_decode_dev.
    stream: coded_bytes(k) bytes.  Returns (data: bytes [k], status: uint8 [codewords(k)] - bytes corrected, or 255)."""
    return _decode_staged(stream, k, None, device, load,
                          lambda d_stream, k, d_erased, d_status, n_cw: decode_device(d_stream, k, d_status, n_cw))
