"""Helpers of the keyed read-back tests (tests/test_keyed_readback_cpu.py, tests/test_keyed_readback_gpu.py): the host build of
the keyed forms of csrc/svs_readback.hpp (tests/hostemu) and a NumPy model of the same check and
repair under a coefficient selection and a keyed dither, restated with the oracle's transforms and dither_lib's hash."""
import numpy as np

import dither_lib
from oracle.qim_dct_oracle import _blocks_view, _fwd, _inv, _quant_index
from readback_lib import ITERS, content
from testlib import host_readback_call

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)
DITHER_KEY = 0x0123456789ABCDEF


def prefix(n):
    return tuple(range(1, n + 1))


def zigzag(n, first=1):
    return tuple(ZIGZAG[first:first + n])


# the rows of the issue's table: (content, delta, selection).  96 x 160 frames, clip frame t = 3, payload cap - 7 bits
TABLE = (
    ("letterbox", 20, prefix(10)),
    ("letterbox", 20, zigzag(10)),
    ("letterbox", 8, zigzag(3)),
    ("letterbox", 8, zigzag(3, 6)),
    ("flat0", 20, zigzag(10)),
    ("flat0", 8, zigzag(3)),
    ("bright", 20, zigzag(10)),
    ("noise", 20, zigzag(10)),
    ("natural", 8, zigzag(3)),
    ("noise", 20, prefix(63)),
)
TABLE_SHAPE = (96, 160)
TABLE_T = 3


def table_frame(kind):
    return content(kind, *TABLE_SHAPE)


def table_case(kind, delta, index, dither, rule):
    """-> (bits, stego of the call without read-back, dither key or None) of one cell of the table, from the NumPy model"""
    g = table_frame(kind)
    cap = (g.shape[0] // 8) * (g.shape[1] // 8) * len(index)
    bits = dither_lib.payload(cap - 7)
    key = DITHER_KEY if dither else None
    stego, used = dither_lib.model_embed(g, delta, bits, rule=rule, index=index, key=key, t=TABLE_T)
    assert used == bits.size
    return bits, stego, key


# ---- the keyed forms on the host (tests/hostemu) ---------------------------------------------------------------------
def host_readback(stego, delta, n_ac, bits, index=None, dither_key=None, block_key=None, first_frame=0, bit_offset=0,
                  n_bits=None):
    """the keyed read-back pass on the host over the stego of the same call without read-back -> (stego after the pass,
    (repaired, unrepaired), status per physical block: 0 reads back, 1 repaired, 2 left, 3 carries no payload).  index None:
    the row-major prefix 1..n_ac.  Always the keyed forms (readback_step_keyed), also for a prefix without a dither, so that
    the tests can hold them to readback_step there."""
    return host_readback_call(stego, delta, n_ac, bits, index=index, dither_key=dither_key, block_key=block_key,
                              first_frame=int(first_frame), bit_offset=bit_offset, n_bits=n_bits, keyed_form=1)


# ---- NumPy model ---------------------------------------------------------------------------------------------------------
def failing_slots(stego, bits, delta, index, key=None, t=0, perm=None):
    """bool per stream slot that carries payload: model_extract (the receiver) does not read the slot's bits back"""
    n = len(index)
    got = dither_lib.model_extract(stego, delta, index=index, key=key, t=t, perm=perm)[: bits.size]
    bad = np.zeros(-(-bits.size // n), bool)
    np.logical_or.at(bad, np.arange(bits.size) // n, got != bits)
    return bad


def model_repair(stego, bits, delta, index, key=None, t=0, perm=None, iters=ITERS):
    """readback_lib.model_repair generalised: the payload coefficients of a block are index[0..], with a key the quantiser sees
    c - d and the targets are moved back by d (d of the block's PHYSICAL position), and slot j is block perm[j].  One gray
    frame -> (stego after the pass, (repaired, unrepaired))."""
    index = np.asarray(index, np.int64)
    n = index.size
    h, w = stego.shape
    f32 = np.float32
    n_blocks = (h // 8) * (w // 8)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    blocks = _blocks_view(f32(stego)).reshape(-1, 8, 8)
    nslot = -(-bits.size // n)
    want = np.zeros((nslot, n), np.int64)
    want.reshape(-1)[: bits.size] = bits
    nb = np.minimum(n, bits.size - np.arange(nslot) * n)
    used = np.arange(n)[None, :] < nb[:, None]
    bad = failing_slots(stego, bits, delta, index, key, t, perm)
    dtab = dither_lib.dither_table(key, t, n_blocks, delta) if key is not None else None
    out = blocks.copy()
    repaired = 0
    d32 = f32(delta)
    for j in np.nonzero(bad)[0]:
        b = perm[j]
        x = blocks[b].copy()
        dv = dtab[b, index] if dtab is not None else None
        c = _fwd(x[None, None])[0, 0].reshape(64)
        cp = c[index] - dv if dv is not None else c[index]
        assert cp.dtype == f32
        q = _quant_index(cp, delta)
        wrong = (q & 1) != want[j]
        up = (cp * (f32(1) / d32)) >= q.astype(f32)
        q = np.where(wrong, np.where(up, q + 1, q - 1), q)
        target = q.astype(f32) * d32
        if dv is not None:
            target = target + dv
        assert target.dtype == f32
        for it in range(iters):
            scale = f32(1.0 + 0.5 * it)
            e = np.zeros(64, f32)
            e[index] = np.where(used[j], (target - c[index]) * scale, f32(0))
            y = x + _inv(e.reshape(1, 1, 8, 8))[0, 0]
            lo, hi = y.min(), y.max()
            s = f32(0)
            if lo < 0 and hi - lo <= 255:
                s = -lo
            elif hi > 255 and hi - lo <= 255:
                s = f32(255) - hi
            x = np.clip(np.rint(y + s), 0, 255).astype(f32)
            c = _fwd(x[None, None])[0, 0].reshape(64)
            cp = c[index] - dv if dv is not None else c[index]
            got = _quant_index(cp, delta) & 1
            if np.all((got == want[j])[used[j]]):
                out[b] = x
                repaired += 1
                break
    frame = out.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w).astype(np.uint8)
    return frame, (repaired, int(bad.sum()) - repaired)
