"""The device encoders (libsvsenc.so, include/svsenc.h): the sending half of the coded path on the GPU - the Reed-Solomon encoder of
svsdct/rs.py, the convolutional encoder of svsdct/fec.py at its six rate codes, and soft.tile on packed bits.  They define no
format: every call writes the bytes of the host encoder of the same name.

    rs_encode_device(d_data, k, d_stream, capacity)                       data -> data + parity (d_stream == d_data: in place)
    fec_encode_device(d_info, n_info, rate, d_coded, capacity)            packed info bits -> packed coded bits
    tile_device(d_bits, period, d_out, n_out_bits, capacity)              packed bits -> copy after copy

batch.embed_coded_device chains them in front of embed_device on one stream; batch.embed_coded_frames(encoder="device") is the
same chain behind one upload.  rs_encode, fec_encode and tile are the staged forms for arrays held on the host: they return what
rs.encode_array, fec.encode and soft.tile return.  The library is loaded on first use; SVSENC_LIB overrides its path.  There is no
fall-back: the host encoders are calls of their own.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import fec as _fec
from . import native
from . import rs as _rs
from .staging import Staged

LIB_PATH = os.environ.get("SVSENC_LIB", os.path.join(native._PKG_DIR, "lib", "libsvsenc.so"))
ABI_VERSION = 1
MAX_TILE_BITS = 1 << 43

_p = C.c_void_p
# name -> (restype, argtypes); every symbol include/svsenc.h declares
SIGNATURES = {
    "svs_enc_abi_version": (C.c_int, []),
    "svs_enc_last_error": (C.c_char_p, []),
    "svs_rs_encode_dev": (C.c_int, [_p, C.c_uint64, _p, C.c_uint64, C.c_void_p]),
    "svs_fec_encode_dev": (C.c_int, [_p, C.c_uint64, C.c_int, _p, C.c_uint64, C.c_void_p]),
    "svs_bits_tile_dev": (C.c_int, [_p, C.c_uint64, _p, C.c_uint64, C.c_uint64, C.c_void_p]),
}

load, check = native.bind(globals(), "svs_enc")


def _tile_bits(n, what: str, least: int) -> int:
    n = int(n)
    if not least <= n <= MAX_TILE_BITS:
        raise ValueError(f"{what} {n} outside {least} .. 2**43")
    return n


def rs_encode_device(d_data: int, k: int, d_stream_out: int, capacity_bytes: int, stream: int = 0) -> None:
    """Enqueue the Reed-Solomon encoder on `stream` (svs_rs_encode_dev): k data bytes at d_data -> rs.coded_bytes(k) bytes at
    d_stream_out, any alignment.  d_stream_out == d_data encodes in place (only the parity is written); otherwise the buffers
    must not overlap."""
    check(load().svs_rs_encode_dev(d_data, _rs._k(k), d_stream_out, int(capacity_bytes), stream or None), "svs_rs_encode_dev")


def fec_encode_device(d_info_packed: int, n_info: int, rate: int, d_coded_packed_out: int, capacity_bytes: int, stream: int = 0) -> None:
    """Enqueue the convolutional encoder on `stream` (svs_fec_encode_dev): the first n_info bits at d_info_packed (any byte
    alignment) -> ceil(fec.coded_bits(n_info, rate) / 8) bytes at d_coded_packed_out, 4-byte aligned."""
    check(load().svs_fec_encode_dev(d_info_packed, _fec._n_info(n_info), _fec._rate(rate), d_coded_packed_out, int(capacity_bytes),
                                    stream or None), "svs_fec_encode_dev")


def tile_device(d_bits_packed: int, period_bits: int, d_out_packed: int, n_out_bits: int, capacity_bytes: int, stream: int = 0) -> None:
    """Enqueue the tile on `stream` (svs_bits_tile_dev): output bit i = input bit i mod period_bits, i < n_out_bits;
    ceil(n_out_bits / 8) bytes at d_out_packed, 4-byte aligned, out of place."""
    check(load().svs_bits_tile_dev(d_bits_packed, _tile_bits(period_bits, "period_bits", 1), d_out_packed,
                                   _tile_bits(n_out_bits, "n_out_bits", 0), int(capacity_bytes), stream or None), "svs_bits_tile_dev")


def _staged(host_in: np.ndarray, out_bytes: int, device: int, call) -> np.ndarray:
    """host_in up, call(d_in, d_out), out_bytes down (null stream, synchronised)"""
    load()
    with Staged(device) as dev:
        d_in, d_out = dev.upload(host_in), dev.alloc(out_bytes)
        call(d_in, d_out)
        out = dev.download(d_out, out_bytes)
        dev.synchronise()
    return out


def rs_encode(data, device: int = 0) -> np.ndarray:
    """rs.encode_array on the device: a bytes object or uint8 array -> uint8 [rs.coded_bytes(k)]"""
    d = _rs._bytes(data)
    k = _rs._k(d.size)
    total = _rs.coded_bytes(k)
    if k == 0:
        return np.empty(0, np.uint8)
    return _staged(d, total, device, lambda d_in, d_out: rs_encode_device(d_in, k, d_out, total))


def fec_encode(bits, rate: int = 2, device: int = 0) -> np.ndarray:
    """fec.encode on the device: payload bits (0/1 per entry) -> uint8 0/1 per coded bit"""
    rate = _fec._rate(rate)
    b = np.asarray(bits, np.uint8).reshape(-1)
    if b.size == 0:
        return np.zeros(0, np.uint8)
    n_coded = _fec.coded_bits(b.size, rate)
    nbytes = (n_coded + 7) // 8
    out = _staged(np.packbits(b), nbytes, device, lambda d_in, d_out: fec_encode_device(d_in, b.size, rate, d_out, nbytes))
    return np.unpackbits(out, count=n_coded)


def tile(bits, n_bits: int, device: int = 0) -> np.ndarray:
    """soft.tile on the device: the payload repeated to n_bits stream bits, the last copy cut: uint8 0 / 1"""
    b = np.asarray(bits, np.uint8).reshape(-1)
    n_bits = int(n_bits)
    if b.size == 0:
        raise ValueError("an empty payload cannot be tiled")
    if n_bits < 0:
        raise ValueError("n_bits is negative")
    if n_bits == 0:
        return np.zeros(0, np.uint8)
    nbytes = (n_bits + 7) // 8
    out = _staged(np.packbits(b), nbytes, device, lambda d_in, d_out: tile_device(d_in, b.size, d_out, n_bits, nbytes))
    return np.unpackbits(out, count=n_bits)
