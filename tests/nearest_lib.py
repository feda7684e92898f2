"""Helpers of the SVS_NEAREST tests (tests/test_nearest_cpu.py, tests/test_nearest_gpu.py): the NumPy model of the nearest-parity
embed, built from the oracle's own pieces, the content classes the feature was measured on, and the host build of the embed
bodies of csrc/svs_block.hpp with the flag (tests/hostemu)."""
import numpy as np

from oracle.qim_dct_oracle import (BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _inv, _quant_index, _requantised,
                                   bits_from_any)
from testlib import host_embed_call, hostemu

DELTAS = (8, 20, 7.3, 0.1, 5000.3)            # QM_POW2, QM_F32, QM_DOUBLE, and two QM_DOUBLE steps on the exact route
N_ACS = (1, 3, 7, 8, 10, 15, 16, 20, 63)
# (content, n_ac, delta) of the feature's measurements (include/svsdct.h, SVS_NEAREST)
MEASURED = (("noise", 3, 8), ("noise", 10, 8), ("noise", 10, 20), ("noise", 63, 8), ("noise_full", 63, 8), ("smooth", 10, 20),
            ("noise", 3, 4), ("noise", 7, 2))


def content(kind, h=480, w=640, seed=1):
    """noise: uniform in [16, 240); noise_full: uniform in [0, 256) (clips); smooth: a sine pattern with sigma = 3 noise; flat:
    constant blocks of several values; letterbox: smooth with black bars"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(16, 240, (h, w), dtype=np.uint8)
    if kind == "noise_full":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    smooth = (128 + 60 * np.sin(x / 17.0) + 40 * np.cos(y / 11.0) + rng.normal(0, 3, (h, w))).clip(0, 255).astype(np.uint8)
    if kind == "smooth":
        return smooth
    if kind == "flat":
        values = rng.integers(0, 256, (h // 8, w // 8), dtype=np.uint8)
        return np.repeat(np.repeat(values, 8, axis=0), 8, axis=1)
    if kind == "letterbox":
        bar = max(8, (h // 6) // 8 * 8)
        smooth[:bar] = 0
        smooth[h - bar:] = 0
        return smooth
    raise ValueError(kind)


def payload(n_bits, seed=3):
    return np.random.default_rng(seed).integers(0, 2, n_bits).astype(np.uint8)


def model_embed(gray, delta, payload, n_ac=MAX_AC, nearest=True, stats=None):
    """oracle.frame_embed with ONE line changed: a wrong parity moves to q + 1 if c > c0, q - 1 if c < c0 and the reference's
    way if c == c0, c0 = _requantised(q, delta) (include/svsdct.h, SVS_NEAREST).  nearest=False is frame_embed itself.
    Returns (gray copy, stego uint8, bits consumed).  stats (optional dict) receives, over the forced coefficients, the
    counts `up` (c > c0), `down` (c < c0), `tie` (c == c0), and the arrays `c`, `old` (the reference's new value), `new`
    (this rule's), `forced` (bool per payload coefficient)."""
    _check_plane(gray)
    gray = np.ascontiguousarray(gray, np.uint8)
    bits = bits_from_any(payload)
    n_use = max(0, min(int(n_ac), MAX_AC))
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
        ki = 1 + np.arange(consumed) % n_use
        c = coef[bi, ki]
        q = _quant_index(c, delta)
        wrong = (q & 1) != use
        ref_step = np.where(use == 1, 1, -1)
        step = ref_step
        if nearest:
            c0 = _requantised(q, delta)
            step = np.where(c > c0, 1, np.where(c < c0, -1, ref_step))      # the rule
            if stats is not None:
                stats.update(up=int((wrong & (c > c0)).sum()), down=int((wrong & (c < c0)).sum()),
                             tie=int((wrong & (c == c0)).sum()), c=c.copy(), forced=wrong,
                             old=_requantised(np.where(wrong, q + ref_step, q), delta))
        q = np.where(wrong, q + step, q)
        coef[bi, ki] = _requantised(q, delta)
        if nearest and stats is not None:
            stats["new"] = coef[bi, ki].copy()
    rec = _inv(coef.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK, BLOCK)
    full = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)
    full[:touched] = rec
    out_f = full.reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
    return gray.copy(), np.uint8(np.clip(out_f, 0, 255)), int(consumed)


def model_batch(frames, delta, bits, n_ac, nearest=True):
    """the frame loop of oracle.batch_embed over model_embed: frame k takes bits [k * cap, (k + 1) * cap) -> (stego, consumed)"""
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    pos = 0
    for k in range(frames.shape[0]):
        if pos < bits.size:
            _, out[k], used = model_embed(frames[k], delta, bits[pos:], n_ac, nearest)
            pos += used
        else:
            out[k] = frames[k]
    return out, pos


def sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


# ---- the embed bodies on the host (tests/hostemu) ---------------------------------------------------------------------
def host_embed(frames, delta, n_ac, bits, bit_offset=0, n_bits=None, pocketfft=False, nearest=True):
    """a gray embed call through the product headers on the host -> (stego, bits embedded, blocks replayed exactly, path)"""
    out, res, _ = host_embed_call(frames, delta, n_ac, bits, bit_offset=bit_offset, n_bits=n_bits, pocketfft=pocketfft,
                                  guarded=not pocketfft, nearest=int(nearest))
    return out, int(res.used), int(res.replayed), int(res.path)


def plan(delta, n_ac, total, n_bits, pocketfft=False, bgr=False, nearest=True):
    """-> (path, nearest, use) of csrc/svs_route.hpp plan_embed"""
    out = np.zeros(6, np.int64)
    hostemu().emu_plan_rule(float(delta), int(n_ac), int(total), int(n_bits), int(pocketfft), int(bgr), int(nearest), 0,
                            out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[3])
