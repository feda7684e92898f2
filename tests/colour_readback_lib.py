"""Helpers of the colour read-back tests (tests/test_colour_readback_cpu.py, tests/test_colour_readback_gpu.py): colour covers
whose gray falls in the content classes of readback_lib, and a NumPy model of the contract of svs_embed_bgr_readback*
(include/svsdct.h) built only from pieces that other tests pin: the fixed-point gray (test_keep_colour_cpu.gray_of), the
oracle's stego (readback_lib.oracle_stego), the host build of csrc/svs_readback.hpp (readback_lib.host_readback) and the
keep-colour rule (test_keep_colour_cpu.keep_colour_rule)."""
import numpy as np

from readback_lib import content, host_readback, oracle_stego
from test_keep_colour_cpu import TABLES, gray_of, keep_colour_rule

KINDS = ("letterbox", "bright", "flat0", "noise")
CLIPPING = ("letterbox", "bright", "flat0")
MAIN_SETTINGS = ((20, 10), (8, 3), (16, 10))
RESIDUAL_SETTINGS = ((4, 3), (20, 63))
SETTINGS = MAIN_SETTINGS + RESIDUAL_SETTINGS
W15, W14 = TABLES["15-bit"], TABLES["14-bit"]


def colour_content(kind, h=64, w=96, seed=1):
    """one BGR frame of a class: letterbox - bars exactly (0, 0, 0) over a coloured interior; bright - saturated, every
    channel near 255; flat0 - black; noise - uniform colour noise"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat0":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "bright":
        return np.stack([content("bright", h, w, seed=seed + 17 * c) for c in range(3)], -1)
    if kind == "letterbox":
        y, x = np.mgrid[0:h, 0:w]
        base = content("natural", h, w, seed=seed).astype(np.int64)
        tint = np.stack([40 * np.sin(x / 23.0 + c) + 30 * np.cos(y / 13.0 - c) for c in range(3)], -1)
        f = np.clip(base[..., None] + tint, 1, 255).astype(np.uint8)
        bar = max(8, (h // 6) // 8 * 8)
        f[:bar] = 0
        f[h - bar:] = 0
        return f
    raise ValueError(kind)


def colour_frames(kind, f, h, w, seed=1):
    return np.stack([colour_content(kind, h, w, seed=seed + k) for k in range(f)])


def oracle_planes(gray, delta, n_ac, bits, bit_offset=0, n_bits=None):
    """the reference's stego of a batch of gray frames: frame k takes the next capacity bits of the window
    [bit_offset, bit_offset + n_bits) of `bits`"""
    bits = np.asarray(bits, np.uint8)
    n_bits = bits.size - bit_offset if n_bits is None else n_bits
    window = bits[bit_offset: bit_offset + n_bits]
    cap = (gray.shape[1] // 8) * (gray.shape[2] // 8) * min(max(int(n_ac), 0), 63)
    out = np.empty_like(gray)
    for k, g in enumerate(gray):
        part = window[k * cap: (k + 1) * cap]
        out[k] = oracle_stego(g, delta, n_ac, part) if part.size else g
    return out


def model(cover, delta, n_ac, bits, weights=W15, keep=False, bit_offset=0, n_bits=None):
    """the contract -> (BGR output, R's stego planes, (repaired, unrepaired), status per block, output without read-back)
    plain: B = G = R = the gray read-back's planes.  keep: P = the keep-colour embed's pixel (rule(cover, reference stego)),
    then rule(P, repaired gray) - which leaves every pixel whose gray the repair did not change as it is."""
    cover = np.asarray(cover, np.uint8)
    gray = gray_of(cover, weights)
    stego0 = oracle_planes(gray, delta, n_ac, bits, bit_offset, n_bits)
    bits = np.asarray(bits, np.uint8)
    n_bits = bits.size - bit_offset if n_bits is None else n_bits
    cap = gray.shape[0] * (gray.shape[1] // 8) * (gray.shape[2] // 8) * min(max(int(n_ac), 0), 63)
    planes, counts, status = host_readback(stego0, delta, n_ac, bits, bit_offset=bit_offset, n_bits=min(n_bits, cap))
    if not keep:
        return np.repeat(planes[..., None], 3, axis=-1), planes, counts, status, np.repeat(stego0[..., None], 3, axis=-1)
    before = keep_colour_rule(cover, stego0, weights)
    return keep_colour_rule(before, planes, weights), planes, counts, status, before
