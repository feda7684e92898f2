"""Errors-and-erasures decoding of the Reed-Solomon outer code (libsvsrse.so, include/svsrse.h): the code, the stream and the
sizes are those of svsdct/rs.py; the decoder also takes a mask, one byte per stream byte, of the bytes the receiver knows to be
bad - the bytes a lost frame maps to - and then stands e wrong bytes and f erased ones in a codeword whenever 2 e + f <= 32:
up to 32 known-bad bytes, twice what svs_rs_decode_dev corrects blind.  A status byte a codeword says how many bytes were changed,
or 255: not decodable, left as received.

    stream = rs.encode(data)
    ... fec.encode, embed, the channel, soft extract, Viterbi ...
    data, status = decode(stream, len(data), mask(len(data), [(lo, hi)]))       device

batch.extract_coded_frames(..., outer=True, lost_frames=[...]) builds the mask from the frames the receiver gave up on and
keeps everything on the device.  The library is loaded on first use; SVSRSE_LIB overrides its path.  There is no CPU decoder.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import native
from .rs import MAX_DATA_BYTES, PARITY, UNCORRECTABLE, _bytes, _decode_staged, _k, codewords, coded_bytes  # noqa: F401

LIB_PATH = os.environ.get("SVSRSE_LIB", os.path.join(native._PKG_DIR, "lib", "libsvsrse.so"))
ABI_VERSION = 1
MAX_ERASED = 32

_p = C.c_void_p
# name -> (restype, argtypes); every symbol include/svsrse.h declares
SIGNATURES = {
    "svs_rse_abi_version": (C.c_int, []),
    "svs_rse_last_error": (C.c_char_p, []),
    "svs_rse_decode_dev": (C.c_int, [_p, C.c_uint64, _p, _p, C.c_uint64, _p, C.c_void_p]),
}

load, check = native.bind(globals(), "svs_rse")


def mask(k: int, spans) -> np.ndarray:
    """uint8 [coded_bytes(k)]: 1 in every byte of the stream that one of the [lo, hi) byte ranges `spans` holds, 0 elsewhere.
    A range is clipped to the stream; lo > hi or a negative bound is a ValueError."""
    out = np.zeros(coded_bytes(k), np.uint8)
    for lo, hi in spans:
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi < lo:
            raise ValueError(f"[{lo}, {hi}) is no byte range")
        out[lo:hi] = 1
    return out


def decode_device(d_stream: int, k: int, d_erased: int, d_status: int, status_capacity: int, d_counts: int = 0, stream: int = 0) -> None:
    """Enqueue the decoder on `stream` (svs_rse_decode_dev): coded_bytes(k) bytes at d_stream, any alignment, decoded in place;
    d_erased: 0 or coded_bytes(k) mask bytes, any alignment, not written; codewords(k) status bytes to d_status; d_counts: 0 or
    a 4-byte aligned uint32[2] that the call adds to."""
    check(load().svs_rse_decode_dev(d_stream, _k(k), d_erased or None, d_status, int(status_capacity), d_counts or None, stream or None),
          "svs_rse_decode_dev")


def decode(stream, k: int, erased=None, device: int = 0):
    """Decode a stream held on the host: staged through svs_malloc / svs_memcpy_*, decoded by svs_rse_decode_dev.
    stream: coded_bytes(k) bytes; erased: None or as many mask bytes (non-zero: that byte is erased).
    Returns (data: bytes [k], status: uint8 [codewords(k)] - bytes changed, or 255)."""
    return _decode_staged(stream, k, erased, device, load, decode_device)
