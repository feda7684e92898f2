"""Helpers of the keyed-dither tests (tests/test_dither_cpu.py, tests/test_dither_gpu.py): the NumPy model - the model embed and
extract of coeff_select_lib / minmove_lib with the three changes of the rule (include/svsdct.h) written out: the quantiser sees
c - d, the written value is moved back by d unless the rule left c - d alone, and the receiver reads the parity of the index of
c - d -, the hash restated here (svsdct/dither.py is code under test and is imported for nothing), and the host build of the
dithered block bodies of csrc/svs_block.hpp (tests/hostemu)."""
import numpy as np

from minmove_lib import band
from oracle.qim_dct_oracle import (BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _inv, _quant_index, _requantised,
                                   bits_from_any)
from testlib import host_embed_call, host_extract_call, hostemu

RULES = ("reference", "nearest", "minmove")
M32 = 0xFFFFFFFF


# ---- the hash, restated with Python integers -------------------------------------------------------------------------
def lb(h):
    """lowbias32 (csrc/svs_order.hpp)"""
    h &= M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def seed_of(key):
    return lb(lb(((key >> 32) & M32) ^ 0x85EBCA6B) ^ (key & M32))


def hash_of(key, t, i, k):
    """h of clip frame t, raster block i, flat coefficient k"""
    s_t = lb(seed_of(key) ^ (t & M32))
    s_b = lb((s_t + i * 0x9E3779B1) & M32)
    return lb(s_b ^ ((k * 0x632BE5AB) & M32))


def _lb_np(h):
    h = h & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def hash_table(key, t, n_blocks):
    """uint32 [N][64] of hash_of, vectorised (tests/test_dither_cpu.py holds it to the integer form)"""
    s_t = lb(seed_of(key) ^ (t & M32))
    i = np.arange(n_blocks, dtype=np.uint64)
    s_b = _lb_np(np.uint64(s_t) + i * np.uint64(0x9E3779B1))
    k = np.arange(64, dtype=np.uint64)
    return _lb_np(s_b[:, None] ^ ((k * np.uint64(0x632BE5AB)) & np.uint64(M32))[None, :]).astype(np.uint32)


def dither_table(key, t, n_blocks, delta):
    """float32 [N][64]: d = ((float)(h >> 8) * 2^-23 - 1) * (float)delta, every step in float32"""
    r = (hash_table(key, t, n_blocks) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    d = r * np.float32(delta)
    assert d.dtype == np.float32
    return d


# ---- the model ---------------------------------------------------------------------------------------------------------
def _index(n_ac, index):
    if index is None:
        index = np.arange(1, max(0, min(int(n_ac), MAX_AC)) + 1)
    return np.asarray(index, np.int64).reshape(-1)


def model_embed(gray, delta, payload, n_ac=MAX_AC, rule="reference", index=None, key=None, t=0, perm=None, stats=None):
    """One frame.  key None: the model of the call without a dither (oracle.frame_embed for the reference rule,
    nearest_lib / minmove_lib's for the others, coeff_select_lib's lookup).  With a key, the three marked lines.  perm: None
    (raster order) or slot -> block of a keyed block order; the dither is that of the block's PHYSICAL position.
    Returns (stego uint8, bits consumed).  stats (optional dict) receives the float32 coefficients before and after."""
    assert rule in RULES
    _check_plane(gray)
    gray = np.ascontiguousarray(gray, np.uint8)
    bits = bits_from_any(payload)
    index = _index(n_ac, index)
    n_use = int(index.size)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    budget = int(bits.size)
    out_f = np.float32(gray)
    if budget == 0:
        return gray.copy(), 0
    if delta <= 0 or n_use == 0:
        touched, consumed = n_blocks, 0
    else:
        touched = min(n_blocks, -(-budget // n_use))
        consumed = min(budget, n_blocks * n_use)
    full = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)
    where = perm[:touched]                                            # the blocks of stream slots 0 .. touched - 1
    coef = _fwd(full[where].reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK * BLOCK)
    if consumed:
        use = bits[:consumed].astype(np.int64)
        bi = np.arange(consumed) // n_use
        ki = index[np.arange(consumed) % n_use]
        c = coef[bi, ki]
        if key is not None:
            d = dither_table(key, t, n_blocks, delta)[where[bi], ki]
            cq = c - d                                                 # change 1: the quantiser sees c - d (float32)
        else:
            cq = c
        assert cq.dtype == np.float32
        q = _quant_index(cq, delta)
        wrong = (q & 1) != use
        step = np.where(use == 1, 1, -1)
        if rule != "reference":
            c0 = _requantised(q, delta)
            step = np.where(cq > c0, 1, np.where(cq < c0, -1, step))
        ct = np.float32(_requantised(np.where(wrong, q + step, q), delta))
        if rule == "minmove":
            r = band(delta)[ki]
            new = np.minimum(np.maximum(cq, ct - r), ct + r)
        else:
            new = ct
        assert new.dtype == np.float32
        if key is not None:                                            # change 2: moved back by d, unless the rule left c - d alone
            new = np.where(new.view(np.uint32) == cq.view(np.uint32), c, new + d)
            assert new.dtype == np.float32
        coef[bi, ki] = new
        if stats is not None:
            stats.update(c=c.copy(), new=new.copy(), k=ki)
    rec = _inv(coef.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK, BLOCK)
    full[where] = rec
    out_f = full.reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
    return np.uint8(np.clip(out_f, 0, 255)), int(consumed)


def model_extract(gray, delta, n_ac=MAX_AC, index=None, key=None, t=0, perm=None):
    """One frame -> 0/1 bits in stream order.  key None: oracle.frame_extract_bits with coeff_select_lib's lookup."""
    _check_plane(gray)
    index = _index(n_ac, index)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    if index.size == 0:
        return np.zeros(0, np.uint8)
    if delta <= 0:
        return np.zeros(n_blocks * index.size, np.uint8)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    blk = _blocks_view(np.float32(gray)).reshape(1, n_blocks, BLOCK, BLOCK)
    coef = _fwd(blk).reshape(n_blocks, BLOCK * BLOCK)[:, index]
    if key is not None:
        coef = coef - dither_table(key, t, n_blocks, delta)[:, index]    # change 3: the parity of the index of c - d
        assert coef.dtype == np.float32
    return (_quant_index(coef, delta) & 1).astype(np.uint8)[perm].reshape(-1)


def _perm(order_key, t, n_blocks):
    if order_key is None:
        return None
    from svsdct.order import slot_to_block    # the keyed order has tests of its own (tests/test_block_order_*.py)
    return slot_to_block(order_key, t, n_blocks)


def model_batch_embed(frames, delta, bits, n_ac=MAX_AC, rule="reference", index=None, key=None, first_frame=0, order_key=None):
    """the frame loop of oracle.batch_embed over model_embed: frame f is clip frame first_frame + f -> (stego, consumed)"""
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    pos = 0
    for f in range(frames.shape[0]):
        if pos < bits.size:
            out[f], used = model_embed(frames[f], delta, bits[pos:], n_ac, rule, index, key, first_frame + f,
                                       _perm(order_key, first_frame + f, n_blocks))
            pos += used
        else:
            out[f] = frames[f]
    return out, pos


def model_batch_extract(frames, delta, n_ac=MAX_AC, index=None, key=None, first_frame=0, order_key=None):
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    return np.concatenate([model_extract(frames[f], delta, n_ac, index, key, first_frame + f,
                                         _perm(order_key, first_frame + f, n_blocks)) for f in range(frames.shape[0])])


def payload(n_bits, seed=3):
    return np.random.default_rng(seed).integers(0, 2, n_bits).astype(np.uint8)


def noise(shape, lo=16, hi=240, seed=1):
    return np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.uint8)


def psnr(a, b):
    e = float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    return float("inf") if e == 0 else 10 * np.log10(255.0 ** 2 * a.size / e)


# ---- the dithered block bodies on the host (tests/hostemu) -------------------------------------------------------------
def host_hash(key, t, i, k, delta=1.0):
    """-> (seed, s_b, h, d) of the product header"""
    out = np.zeros(3, np.uint32)
    d = hostemu().dt_hash(int(key), int(t), int(i), int(k), float(delta), out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2]), np.float32(d)


def _plan(res):
    return dict(path=int(res.path), rows=int(res.rows), selected=int(res.selected), qm=int(res.qm), dithered=int(res.dithered))


def host_embed(frames, delta, n_ac, bits, key, first_frame=0, rule="reference", index=None, bit_offset=0, n_bits=None, flags=0):
    """a dithered gray embed call through the product headers on the host -> (stego, bits embedded, plan dict)"""
    out, res, _ = host_embed_call(frames, delta, n_ac, bits, bit_offset=bit_offset, n_bits=n_bits, index=index,
                                  pocketfft=flags & 1, guarded=flags & 2, nearest=int(rule == "nearest"),
                                  minmove=int(rule == "minmove"), dither_key=int(key), first_frame=int(first_frame))
    return out, int(res.used), _plan(res)


def host_extract(frames, delta, n_ac, key, first_frame=0, index=None, flags=0):
    """a dithered gray extract call on the host -> (0/1 bits, plan dict)"""
    out, res, _ = host_extract_call(frames, delta, n_ac, index=index, pocketfft=flags & 1, guarded=flags & 2, dither_key=int(key),
                                    first_frame=int(first_frame))
    return out, _plan(res)
