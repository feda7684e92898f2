"""Keyed block order, restated in NumPy (csrc/svs_order.hpp is the definition the kernels use).

With a block key, the bits of frame t of a clip no longer fill its blocks in raster order: stream slot j of the frame (its bits
j*n .. j*n+n-1) goes to block sigma_t(j), a key-seeded permutation of the frame's N blocks (a four-round Feistel network with
cycle walking).  Frames keep their stream ranges; only the blocks inside a frame are reordered.  The permutation is NOT
cryptographic: it hides where the payload sits from a look at the frame; confidentiality comes from the AES-GCM layer.

Because the reference operator treats every 8x8 block on its own, the keyed operator is the reference operator on
block-permuted frames:
    keyed_embed(F)   = unpermute_blocks(reference_embed(permute_blocks(F)))
    keyed_extract(S) = reference_extract(permute_blocks(S))
which is how the tests check the kernels.  A user can call these to see where the bits of a frame went.
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
        raise TypeError(f"block key must be an integer, not {type(key).__name__}")
    key = int(key)
    if not 0 <= key <= KEY_MAX:
        raise ValueError(f"block key {key} outside 0 .. 2**64 - 1")
    return key


def key_from_env(environ=None):
    """SVS_BLOCK_KEY of the drop-in embed / extract loops: unset (or empty) -> None, the reference's raster order; otherwise
    int(value, 0) (decimal, 0x..., 0o..., 0b...), which must lie in 0 .. 2**64 - 1 (ValueError otherwise)."""
    value = (os.environ if environ is None else environ).get("SVS_BLOCK_KEY")
    if value is None or value.strip() == "":
        return None
    return check_key(int(value.strip(), 0))


def _lb(x: int) -> int:
    return int(_lowbias32(np.uint64(x & _M32)))


def _params(key: int, t: int, n_blocks: int):
    key = check_key(key)
    s = _lb(_lb((key >> 32) ^ 0x9E3779B9) ^ (key & _M32))
    s = _lb(s ^ (int(t) & _M32))
    rk = [_lb(s + (r + 1) * 0x632BE5AB) for r in range(4)]
    k = max(2, (int(n_blocks) - 1).bit_length())
    b = k >> 1
    return rk, b, (1 << b) - 1, (1 << (k - b)) - 1, 1 << k


def _feistel(x: np.ndarray, rk, b, mask_l, mask_h, rounds) -> np.ndarray:
    h, l = x >> np.uint64(b), x & np.uint64(mask_l)
    for r in rounds:
        if r % 2 == 0:
            l = l ^ (_lowbias32(h ^ np.uint64(rk[r])) & np.uint64(mask_l))
        else:
            h = h ^ (_lowbias32(l ^ np.uint64(rk[r])) & np.uint64(mask_h))
    return (h << np.uint64(b)) | l


def _walk(key, t, n_blocks, rounds) -> np.ndarray:
    n_blocks = int(n_blocks)
    if n_blocks < 1:
        raise ValueError("n_blocks must be >= 1")
    if n_blocks == 1:
        return np.zeros(1, np.int64)
    rk, b, mask_l, mask_h, size = _params(key, t, n_blocks)
    # the permutation of the whole domain [0, 2^k), then cycle walking into [0, N) for all starting points at once
    perm = _feistel(np.arange(size, dtype=np.uint64), rk, b, mask_l, mask_h, rounds).astype(np.int64)
    y = perm[:n_blocks].copy()
    out = y >= n_blocks
    while out.any():
        y[out] = perm[y[out]]
        out = y >= n_blocks
    return y


def slot_to_block(key, t: int, n_blocks: int) -> np.ndarray:
    """int64 [N]: entry j = sigma_t(j), the block (raster index inside the frame) that takes stream slot j of clip frame t"""
    return _walk(key, t, n_blocks, (0, 1, 2, 3))


def block_to_slot(key, t: int, n_blocks: int) -> np.ndarray:
    """int64 [N]: entry i = sigma_t^-1(i), the stream slot of block i of clip frame t"""
    return _walk(key, t, n_blocks, (3, 2, 1, 0))


def _blocks(frames: np.ndarray):
    a = np.asarray(frames)
    if a.ndim == 2:
        a = a[None]
    f, h, w = a.shape[:3]
    if h % 8 or w % 8:
        raise ValueError("frame height and width must be multiples of 8")
    # [F, N, 8, 8, ...] in raster block order
    return a.reshape(f, h // 8, 8, w // 8, 8, *a.shape[3:]).swapaxes(2, 3).reshape(f, (h // 8) * (w // 8), 8, 8, *a.shape[3:])


def _unblocks(blocks: np.ndarray, shape) -> np.ndarray:
    f, h, w = shape[:3]
    return blocks.reshape(f, h // 8, w // 8, 8, 8, *shape[3:]).swapaxes(2, 3).reshape(shape)


def permute_blocks(frames: np.ndarray, key, first_frame: int = 0) -> np.ndarray:
    """P(F): block sigma_t(j) of frame f (t = first_frame + f) moves to raster position j.  frames [F, H, W] (or [H, W], or
    with trailing channel axes); returns a new array of the same shape."""
    a = np.asarray(frames)
    shape = a.shape if a.ndim != 2 else (1, *a.shape)
    blk = _blocks(a)
    out = np.empty_like(blk)
    for f in range(blk.shape[0]):
        out[f] = blk[f][slot_to_block(key, first_frame + f, blk.shape[1])]
    return _unblocks(out, shape).reshape(a.shape)


def unpermute_blocks(frames: np.ndarray, key, first_frame: int = 0) -> np.ndarray:
    """P^-1: the inverse of permute_blocks (raster position j goes back to block sigma_t(j))"""
    a = np.asarray(frames)
    shape = a.shape if a.ndim != 2 else (1, *a.shape)
    blk = _blocks(a)
    out = np.empty_like(blk)
    for f in range(blk.shape[0]):
        out[f][slot_to_block(key, first_frame + f, blk.shape[1])] = blk[f]
    return _unblocks(out, shape).reshape(a.shape)
