"""Keyed dither modulation, restated in NumPy (csrc/svs_block.hpp is the definition the kernels use; include/svsdct.h the rule).

With a dither key both sides shift the quantiser lattice of every payload coefficient by a key-derived offset d in
[-delta, delta): the embedder applies its rule to c - d and writes the result moved back by d, the receiver reads the parity
of the index of c - d.  The offset depends on the clip frame t, the block's raster index i inside the frame and the flat
coefficient index k - not on a keyed block order or a coefficient selection.  It costs no distortion (QIM distortion is shift
invariant); it removes the comb in the histogram of c mod delta that announces an undithered stego frame, and a receiver
without the key reads coin flips.  NOT a cryptographic generator (lowbias32): confidentiality remains the AES-GCM layer's.
"""
from __future__ import annotations

import os

import numpy as np

from .synth import _lowbias32

KEY_MAX = (1 << 64) - 1
_M32 = 0xFFFFFFFF


def check_key(key) -> int:
    """-> the key as an int; raises ValueError unless 0 <= key < 2**64"""
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)):
        raise TypeError(f"dither key must be an integer, not {type(key).__name__}")
    key = int(key)
    if not 0 <= key <= KEY_MAX:
        raise ValueError(f"dither key {key} outside 0 .. 2**64 - 1")
    return key


def key_from_env(environ=None):
    """SVS_DITHER_KEY of the drop-in embed / extract loops: unset (or empty) -> None, no dither; otherwise int(value, 0)
    (decimal, 0x..., 0o..., 0b...), which must lie in 0 .. 2**64 - 1 (ValueError otherwise)."""
    value = (os.environ if environ is None else environ).get("SVS_DITHER_KEY")
    if value is None or value.strip() == "":
        return None
    return check_key(int(value.strip(), 0))


def _lb(x) -> np.ndarray:
    return _lowbias32(np.asarray(x, np.uint64) & np.uint64(_M32)) & np.uint64(_M32)


def seed(key) -> int:
    """lb(lb(hi32(key) ^ 0x85EBCA6B) ^ lo32(key)): not the block order's seed, so one key may serve both"""
    key = check_key(key)
    return int(_lb(int(_lb((key >> 32) ^ 0x85EBCA6B)) ^ (key & _M32)))


def hashes(key, t: int, n_blocks_per_frame: int) -> np.ndarray:
    """uint32 [N][64]: h of block i, coefficient k of clip frame t (column 0, the DC position, is never used)"""
    s_t = _lb(seed(key) ^ (int(t) & _M32))
    i = np.arange(int(n_blocks_per_frame), dtype=np.uint64)
    s_b = _lb(s_t + i * np.uint64(0x9E3779B1))
    k = np.arange(64, dtype=np.uint64)
    return _lb(s_b[:, None] ^ ((k * np.uint64(0x632BE5AB)) & np.uint64(_M32))[None, :]).astype(np.uint32)


def dither(key, t: int, n_blocks_per_frame: int, delta) -> np.ndarray:
    """float32 [N][64]: d of raster block i and flat coefficient k of clip frame t, d = r * (float)delta with
    r = (float)(h >> 8) * 2^-23 - 1 in [-1, 1) (every step one float32 operation, all but the last exact)"""
    h = hashes(key, t, n_blocks_per_frame)
    r = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return r * np.float32(delta)
