"""Helpers of the SVS_READBACK tests (tests/test_readback_cpu.py, tests/test_readback_gpu.py): the content classes on which the
reference's own stego fails to read back, the oracle read-back, the host build of csrc/svs_readback.hpp
(tests/hostemu) and a NumPy model of the repair."""
import numpy as np

from oracle.qim_dct_oracle import _blocks_view, _fwd, _inv, _quant_index, frame_embed, frame_extract_bits
from testlib import host_readback_call

KINDS = ("noise", "natural", "letterbox", "bright", "flat0")
CLIPPING = ("letterbox", "bright", "flat0")
SETTINGS = ((20, 10), (8, 3), (16, 10), (4, 3), (20, 63))
ITERS = 16   # SVS_READBACK_ITERS


def content(kind, h=240, w=320, seed=1):
    """gray frame of one content class: uniform noise, a natural-like smooth frame, the same letterboxed (black bars over a
    third of the rows), bright (255 - dark) and flat black"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    nat = (128 + 60 * np.sin(x / 17.0) + 40 * np.cos(y / 11.0) + rng.normal(0, 6, (h, w))).clip(0, 255).astype(np.uint8)
    if kind == "natural":
        return nat
    if kind == "letterbox":
        f = nat.copy()
        bar = (h // 6) // 8 * 8
        f[:bar] = 0
        f[h - bar:] = 0
        return f
    if kind == "bright":
        return (255 - nat // 8).astype(np.uint8)
    if kind == "flat0":
        return np.zeros((h, w), np.uint8)
    raise ValueError(kind)


def payload(n_bits, seed=3):
    return np.random.default_rng(seed).integers(0, 2, n_bits).astype(np.uint8)


def failing_blocks(stego, bits, delta, n_ac):
    """bool per block that carries payload (raster order): the oracle does not read the block's bits back"""
    n = min(n_ac, 63)
    got = frame_extract_bits(stego, delta, n)[: bits.size]
    bad = np.zeros(-(-bits.size // n), bool)
    np.logical_or.at(bad, np.arange(bits.size) // n, got != bits)
    return bad


# ---- csrc/svs_readback.hpp on the host (tests/hostemu) ---------------------------------------------------------------
def host_readback(stego, delta, n_ac, bits, bit_offset=0, n_bits=None, block_key=None, first_frame=0):
    """the read-back pass of csrc/svs_readback.hpp on the host over the reference's stego of a call -> (stego after the pass,
    (repaired, unrepaired), status per block: 0 reads back, 1 repaired, 2 left, 3 carries no payload)"""
    return host_readback_call(stego, delta, n_ac, bits, bit_offset=bit_offset, n_bits=n_bits, block_key=block_key,
                              first_frame=int(first_frame))


# ---- NumPy model of the repair -----------------------------------------------------------------------------------------
def model_repair(stego, bits, delta, n_ac, iters=ITERS):
    """The repair of csrc/svs_readback.hpp restated with the oracle's transforms, in float32, on one gray frame in raster
    order -> (stego after the pass, (repaired, unrepaired)).  Every block whose bits the oracle does not read back moves
    towards the nearest lattice point of its wanted bits, over-relaxed, shifted off 0 / 255 where its range allows, rounded to
    nearest; it is kept only when the oracle reads it back."""
    n = min(n_ac, 63)
    h, w = stego.shape
    f32 = np.float32
    blocks = _blocks_view(f32(stego)).reshape(-1, 8, 8)
    nblk = -(-bits.size // n)
    want = np.zeros((nblk, n), np.int64)
    want.reshape(-1)[: bits.size] = bits
    nb = np.minimum(n, bits.size - np.arange(nblk) * n)                        # bits per block (the last one: the rest)
    used = np.arange(n)[None, :] < nb[:, None]
    bad = failing_blocks(stego, bits, delta, n)
    idx = np.nonzero(bad)[0]
    out = blocks.copy()
    repaired = 0
    d32 = f32(delta)
    for b in idx:
        x = blocks[b].copy()
        c = _fwd(x[None, None])[0, 0].reshape(64)
        q = _quant_index(c[1:1 + n], delta)
        wrong = (q & 1) != want[b]
        up = (c[1:1 + n] * (f32(1) / d32)) >= q.astype(f32)
        q = np.where(wrong, np.where(up, q + 1, q - 1), q)
        target = q.astype(f32) * d32
        for it in range(iters):
            scale = f32(1.0 + 0.5 * it)
            d = np.zeros(64, f32)
            d[1:1 + n] = np.where(used[b], (target - c[1:1 + n]) * scale, f32(0))
            y = x + _inv(d.reshape(1, 1, 8, 8))[0, 0]
            lo, hi = y.min(), y.max()
            s = f32(0)
            if lo < 0 and hi - lo <= 255:
                s = -lo
            elif hi > 255 and hi - lo <= 255:
                s = f32(255) - hi
            x = np.clip(np.rint(y + s), 0, 255).astype(f32)
            c = _fwd(x[None, None])[0, 0].reshape(64)
            got = _quant_index(c[1:1 + n], delta) & 1
            if np.all((got == want[b])[used[b]]):
                out[b] = x
                repaired += 1
                break
    frame = out.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w).astype(np.uint8)
    return frame, (repaired, int(idx.size) - repaired)


def oracle_stego(gray, delta, n_ac, bits):
    return frame_embed(gray, delta, bits, n_ac)[1]
