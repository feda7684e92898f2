"""Helpers of the coefficient-selection tests (tests/test_coeff_select_cpu.py, tests/test_coeff_select_gpu.py): the restatement -
oracle.frame_embed / frame_extract_bits with ONE lookup changed (stream bit i of a block goes to coefficient index[i] instead
of 1 + i) and an optional nearest rule, built from the oracle's own pieces -, a literal per-block loop form, the zig-zag table
written out (not derived by the code under test), and the host build of the block bodies (tests/hostemu)."""
import numpy as np
from scipy.fftpack import dct, idct

from oracle.qim_dct_oracle import (BLOCK, _blocks_view, _check_plane, _fwd, _inv, _quant_index, _requantised, bits_from_any)
from testlib import host_embed_call, host_extract_call, hostemu

# JPEG zig-zag scan of an 8 x 8 block, flat row-major indices, position 0 = DC (ITU-T T.81 figure A.6)
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10,
          17, 24, 32, 25, 18, 11, 4, 5,
          12, 19, 26, 33, 40, 48, 41, 34,
          27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36,
          29, 22, 15, 23, 30, 37, 44, 51,
          58, 59, 52, 45, 38, 31, 39, 46,
          53, 60, 61, 54, 47, 55, 62, 63]

DELTAS = (8, 20, 7.3)            # the three quantiser classes: QM_POW2, QM_F32, QM_DOUBLE
COUNTS = (1, 3, 10, 32, 33, 63)


def zigzag(count, first=1):
    return ZIGZAG[first:first + count]


def prefix(count):
    return list(range(1, count + 1))


def reversed_list(count):
    """the row-major prefix backwards: the same coefficients, the opposite bit order"""
    return list(range(count, 0, -1))


def scattered(count, seed=5):
    """`count` distinct indices of 1..63 in a seeded random order"""
    return [int(k) for k in np.random.default_rng(seed + count).permutation(np.arange(1, 64))[:count]]


KINDS = {"zigzag": zigzag, "reversed": reversed_list, "scattered": scattered}


def select_embed(gray, delta, payload, index, nearest=False):
    """oracle.frame_embed with the coefficient lookup changed: ki = index[i % n] (frame_embed: 1 + i % n), n = len(index).
    nearest: the SVS_NEAREST rule of tests/nearest_lib.model_embed.  Returns (gray copy, stego uint8, bits consumed)."""
    _check_plane(gray)
    gray = np.ascontiguousarray(gray, np.uint8)
    bits = bits_from_any(payload)
    index = np.asarray(index, np.int64).reshape(-1)
    n_use = int(index.size)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    budget = int(bits.size)
    out_f = np.float32(gray)
    if budget == 0:
        return gray.copy(), gray.copy(), 0
    if delta <= 0 or n_use == 0:
        touched, consumed = n_blocks, 0
    else:
        touched = min(n_blocks, -(-budget // n_use))
        consumed = min(budget, n_blocks * n_use)
    blk = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)[:touched]
    coef = _fwd(blk.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK * BLOCK)
    if consumed:
        use = bits[:consumed].astype(np.int64)
        bi = np.arange(consumed) // n_use
        ki = index[np.arange(consumed) % n_use]                  # the one changed line
        c = coef[bi, ki]
        q = _quant_index(c, delta)
        wrong = (q & 1) != use
        step = np.where(use == 1, 1, -1)
        if nearest:
            c0 = _requantised(q, delta)
            step = np.where(c > c0, 1, np.where(c < c0, -1, step))
        q = np.where(wrong, q + step, q)
        coef[bi, ki] = _requantised(q, delta)
    rec = _inv(coef.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK, BLOCK)
    full = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)
    full[:touched] = rec
    out_f = full.reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
    return gray.copy(), np.uint8(np.clip(out_f, 0, 255)), int(consumed)


def select_extract_bits(gray, delta, index):
    """oracle.frame_extract_bits with the lookup changed: the coefficients index[0], index[1], .. of each block"""
    _check_plane(gray)
    index = np.asarray(index, np.int64).reshape(-1)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    if index.size == 0:
        return np.zeros(0, np.uint8)
    if delta <= 0:
        return np.zeros(n_blocks * index.size, np.uint8)
    blk = _blocks_view(np.float32(gray)).reshape(1, n_blocks, BLOCK, BLOCK)
    coef = _fwd(blk).reshape(n_blocks, BLOCK * BLOCK)[:, index]  # the one changed line
    return (_quant_index(coef, delta) & 1).astype(np.uint8).reshape(-1)


def select_batch_embed(frames, delta, bits, index, nearest=False):
    """the frame loop of oracle.batch_embed over select_embed -> (stego, consumed)"""
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    pos = 0
    for k in range(frames.shape[0]):
        if pos < bits.size:
            _, out[k], used = select_embed(frames[k], delta, bits[pos:], index, nearest)
            pos += used
        else:
            out[k] = frames[k]
    return out, pos


def select_batch_extract(frames, delta, index):
    return np.concatenate([select_extract_bits(f, delta, index) for f in frames])


def select_loops(gray, mode, delta, payload, index):
    """oracle.frame_operator_loops with `for k in index` instead of `for k in range(1, n + 1)` (small inputs)"""
    bits = bits_from_any(payload)
    pix = np.float32(gray)
    out = pix.copy()
    h, w = pix.shape
    taken, limit, emitted, done = 0, (int(bits.size) if mode == "embed" else 0), [], False
    for y0 in range(0, h, BLOCK):
        if done:
            break
        for x0 in range(0, w, BLOCK):
            if mode == "embed" and taken >= limit:
                done = True
                break
            tile = pix[y0:y0 + BLOCK, x0:x0 + BLOCK]
            flat = dct(dct(tile, axis=0, norm="ortho"), axis=1, norm="ortho").flatten()
            new = flat.copy()
            for k in index:
                if mode == "embed" and taken >= limit:
                    break
                if delta <= 0:
                    if mode == "extract":
                        emitted.append(0)
                    continue
                qi = int(round(flat[k] / delta))
                if mode == "embed":
                    want = int(bits[taken])
                    if qi % 2 != want:
                        qi += 1 if want == 1 else -1
                    new[k] = float(qi * delta)
                    taken += 1
                else:
                    emitted.append(qi % 2)
            if mode == "embed":
                out[y0:y0 + BLOCK, x0:x0 + BLOCK] = idct(
                    idct(new.reshape(BLOCK, BLOCK), axis=0, norm="ortho"), axis=1, norm="ortho")
    if mode == "embed":
        return gray.copy(), np.uint8(np.clip(out, 0, 255)), taken
    return np.array(emitted, np.uint8)


def content(kind, f=1, h=64, w=96, seed=1):
    """[F, H, W]: noise in [16, 240); clip: noise in [0, 256); flat: constant blocks of several values, 0 and 255 among them"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(16, 240, (f, h, w), dtype=np.uint8)
    if kind == "clip":
        return rng.integers(0, 256, (f, h, w), dtype=np.uint8)
    if kind == "flat":
        v = rng.integers(0, 256, (f, h // 8, w // 8), dtype=np.uint8)
        v[:, 0, 0], v[:, 0, 1] = 0, 255
        return np.repeat(np.repeat(v, 8, axis=1), 8, axis=2)
    raise ValueError(kind)


def payload(n_bits, seed=3):
    return np.random.default_rng(seed).integers(0, 2, n_bits).astype(np.uint8)


# ---- the block bodies on the host (tests/hostemu) ---------------------------------------------------------------------
def _plan(res):
    return dict(path=int(res.path), rows=int(res.rows), selected=int(res.selected), qm=int(res.qm))


def host_embed(frames, delta, index, bits, bit_offset=0, n_bits=None, flags=0, nearest=False):
    """a select embed call through the product headers on the host (svs_route.hpp's plan, svs_block.hpp's bodies)
    -> (stego, bits embedded, plan dict).  Always with the exact arithmetic: a plan without the table (a prefix selection)
    streams, and the streaming bodies give the same bytes and have tests of their own."""
    out, res, _ = host_embed_call(frames, delta, 0, bits, bit_offset=bit_offset, n_bits=n_bits, index=index, pocketfft=flags & 1,
                                  guarded=flags & 2, nearest=int(nearest), streaming_bodies=0)
    return out, int(res.used), _plan(res)


def host_extract(frames, delta, index, flags=0):
    """a select extract call on the host -> (0/1 bits, plan dict)"""
    out, res, _ = host_extract_call(frames, delta, 0, index=index, pocketfft=flags & 1, guarded=flags & 2, streaming_bodies=0)
    return out, _plan(res)


def host_table(index):
    """svs::make_coeff_table -> (valid, slot[64], count)"""
    idx = np.ascontiguousarray(np.asarray(index, np.int64).reshape(-1).astype(np.uint8)) if len(index) else np.zeros(1, np.uint8)
    out = np.zeros(65, np.int32)
    ok = hostemu().cs_table(idx.ctypes.data, len(index), out.ctypes.data)
    return bool(ok), out[:64].copy(), int(out[64])
