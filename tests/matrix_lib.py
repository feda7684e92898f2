"""Helpers of the matrix-embedding tests (tests/test_matrix_cpu.py, tests/test_matrix_gpu.py): an independent NumPy receiver - the
Hamming syndrome of stepped_lib's NumPy parities -, an independent NumPy sender for the syndrome's single flip (search 0) - the
flipped parities handed to stepped_lib.model_embed as a payload of n bits a block -, the verdict functions for the pair search
(search 1: the parities a block changed and the float32 cost e of flipping a slot), and the host build of the matrix block
bodies of csrc/svs_block.hpp (tests/hostemu/matrix_emu.cpp).  The format is stated in include/svsdct.h, "matrix embedding"."""
import ctypes as C

import numpy as np

import dither_lib as dl
import soft_lib as sl
import stepped_lib as st
from testlib import build_emu
from oracle.qim_dct_oracle import BLOCK, _blocks_view, _fwd, bits_from_any

KS = (1, 2, 3, 4, 6)
TABLES = ("u20", "u16", "u7", "m75x2")
ORDER_KEY = st.ORDER_KEY
DITHER_KEY = st.DITHER_KEY
FIRST_FRAME = st.FIRST_FRAME


def slots(k):
    return (1 << k) - 1


def zigzag(k):
    """zig-zag scan positions 1 .. 2^k - 1 as flat row-major indices: not a prefix for k >= 2"""
    return tuple(int(v) for v in sl.ZIGZAG[:slots(k)])


def selection(k, zz):
    return zigzag(k) if zz else tuple(range(1, slots(k) + 1))


# name -> (order key, zig-zag selection?, dither key); rotated over the cases by the tests
OPTIONS = {
    "plain": (None, False, None),
    "order": (ORDER_KEY, False, None),
    "select": (None, True, None),
    "dither": (None, False, DITHER_KEY),
    "all": (ORDER_KEY, True, DITHER_KEY),
}


def n_blocks_of(plane):
    return (plane.shape[0] // BLOCK) * (plane.shape[1] // BLOCK)


def capacity(shape, k):
    f, h, w = shape
    return f * (h // 8) * (w // 8) * k


def payload_for(shape, k, seed=3):
    """a payload that ends inside the last frame and, for k >= 2, inside a block (n_bits is no multiple of k)"""
    cap = capacity(shape, k)
    n = cap - 3 * k - 1 if cap > 4 * k else max(1, k - 1)
    if k > 1 and n % k == 0:
        n -= 1
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


# ---- the receiver ------------------------------------------------------------------------------------------------------------
def parities(plane, table, k, index, key=None, t=0, perm=None):
    """-> uint8 [blocks in stream order][n]: stepped_lib's NumPy verdict of every selected coefficient"""
    n = slots(k)
    assert len(index) == n
    return st.model_extract(plane, table, index=index, key=key, t=t, perm=perm).reshape(-1, n)


def syndrome(par):
    """[blocks][n] parities -> the XOR over the set slots t of t + 1"""
    par = np.asarray(par).astype(np.int64)
    s = np.zeros(par.shape[0], np.int64)
    for t in range(par.shape[1]):
        s ^= par[:, t] * (t + 1)
    return s


def bits_of(values, k):
    """message values -> their k stream bits each, bit i first"""
    return ((np.asarray(values)[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint8).reshape(-1)


def model_extract(plane, table, k, index, key=None, t=0, perm=None):
    return bits_of(syndrome(parities(plane, table, k, index, key, t, perm)), k)


def model_batch_extract(frames, table, k, index, key=None, first_frame=0, order_key=None):
    nb = n_blocks_of(frames[0])
    return np.concatenate([model_extract(frames[f], table, k, index, key, first_frame + f, dl._perm(order_key, first_frame + f, nb))
                           for f in range(frames.shape[0])])


def messages(bits, k, touched):
    """the message values of the first `touched` stream positions: bits past the end count as 0"""
    padded = np.zeros(touched * k, np.int64)
    padded[:min(bits.size, touched * k)] = bits[:touched * k]
    return (padded.reshape(touched, k) << np.arange(k)[None, :]).sum(axis=1)


# ---- the sender, search 0 -----------------------------------------------------------------------------------------------------
def model_embed(plane, table, payload, k, index, rule="reference", key=None, t=0, perm=None):
    """one frame -> (stego, bits consumed): the cover's parities with the syndrome's single flip, written by stepped_lib's model
    as a payload of n bits a block over the blocks the budget reaches"""
    bits = bits_from_any(payload)
    nb = n_blocks_of(plane)
    n = slots(k)
    consumed = min(int(bits.size), nb * k)
    if consumed == 0:
        return plane.copy(), 0
    touched = -(-consumed // k)
    par = parities(plane, table, k, index, key, t, perm)[:touched].copy()
    j = syndrome(par) ^ messages(bits[:consumed], k, touched)
    hit = np.nonzero(j)[0]
    par[hit, j[hit] - 1] ^= 1
    stego, used = st.model_embed(plane, table, par.reshape(-1), rule=rule, index=index, key=key, t=t, perm=perm)
    assert used == touched * n
    return stego, consumed


def model_batch_embed(frames, table, bits, k, index, rule="reference", key=None, first_frame=0, order_key=None):
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    nb = n_blocks_of(frames[0])
    pos = 0
    for f in range(frames.shape[0]):
        if pos < bits.size:
            out[f], used = model_embed(frames[f], table, bits[pos:], k, index, rule, key, first_frame + f,
                                       dl._perm(order_key, first_frame + f, nb))
            pos += used
        else:
            out[f] = frames[f]
    return out, pos


# ---- the pair search's verdicts -----------------------------------------------------------------------------------------------
def rule_input(plane, table, index, key=None, t=0, perm=None):
    """-> float32 [blocks in stream order][n]: x = c - d of every selected coefficient"""
    nb = n_blocks_of(plane)
    index = np.asarray(index)
    perm = np.arange(nb) if perm is None else np.asarray(perm, np.int64)
    coef = _fwd(_blocks_view(np.float32(plane)).reshape(1, nb, BLOCK, BLOCK)).reshape(nb, BLOCK * BLOCK)[:, index]
    if key is not None:
        coef = coef - st.dither_values(key, t, nb, table)[:, index]
    assert coef.dtype == np.float32
    return coef[perm]


def rule_value(x, bit, table, index, rule):
    """stepped_target in NumPy float32: x [blocks][n], bit [blocks][n] -> the rule's value"""
    index = np.asarray(index)
    dk = st._steps_f32(table)[index][None, :]
    q = np.rint(x / dk).astype(np.int64)
    step = np.where(bit == 1, 1, -1)
    if rule != "reference":
        c0 = q.astype(np.float32) * dk
        step = np.where(x > c0, 1, np.where(x < c0, -1, step))
    ct = np.where((q & 1) != bit, q + step, q).astype(np.float32) * dk
    if rule == "minmove":
        r = st.band(table)[index][None, :]
        ct = np.minimum(np.maximum(x, ct - r), ct + r)
    assert ct.dtype == np.float32
    return ct


def flip_costs(plane, table, k, index, rule, key=None, t=0, perm=None):
    """-> (parities [blocks][n], e float32 [blocks][n]): a = flip - x; b = stay - x; e = a a - b b, one float32 operation a step"""
    x = rule_input(plane, table, index, key, t, perm)
    p = parities(plane, table, k, index, key, t, perm).astype(np.int64)
    a = rule_value(x, p ^ 1, table, index, rule) - x
    b = rule_value(x, p, table, index, rule) - x
    e = a * a - b * b
    assert e.dtype == np.float32
    return p, e


def psnr(a, b):
    return st.psnr_pooled(a, b)


# ---- the matrix block bodies on the host -------------------------------------------------------------------------------------------
PROTOTYPES = {
    "matrix_emu_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_uint32]),
    "matrix_emu_extract": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint64,
                                     C.c_uint32, C.c_void_p]),
    "matrix_emu_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p]),
}


def emu(build_dir=None):
    """tests/hostemu/matrix_emu.cpp, compiled once per process with -ffp-contract=off"""
    return build_emu("matrix_emu.cpp", PROTOTYPES, build_dir, ("-ffp-contract=off",))


def _perm_arg(perm):
    if perm is None:
        return None, None
    keep = np.ascontiguousarray(perm, np.int64)
    return keep, keep.ctypes.data


def host_embed(plane, table, payload, k, index, search=0, rule="reference", key=None, t=0, perm=None):
    """one frame through embed_block_matrix on the host -> (stego uint8, bits consumed)"""
    index = np.ascontiguousarray(index, np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    bits = np.ascontiguousarray(bits_from_any(payload), np.uint8)
    blocks = st._to_blocks(np.ascontiguousarray(plane, np.uint8))
    out = np.empty_like(blocks)
    keep, p = _perm_arg(perm)
    n_bits = min(int(bits.size), blocks.shape[0] * k)
    rc = emu().matrix_emu_embed(blocks.ctypes.data, out.ctypes.data, blocks.shape[0], table.ctypes.data, index.ctypes.data,
                                int(index.size), int(k), int(search), p, bits.ctypes.data, n_bits, st.RULE_KIND[rule],
                                int(key is not None), int(key or 0), int(t))
    assert rc == 0
    return st._from_blocks(out, *plane.shape), n_bits


def host_extract(plane, table, k, index, key=None, t=0, perm=None):
    index = np.ascontiguousarray(index, np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    blocks = st._to_blocks(np.ascontiguousarray(plane, np.uint8))
    out = np.zeros(blocks.shape[0] * k, np.uint8)
    keep, p = _perm_arg(perm)
    rc = emu().matrix_emu_extract(blocks.ctypes.data, blocks.shape[0], table.ctypes.data, index.ctypes.data, int(index.size), int(k), p,
                                  int(key is not None), int(key or 0), int(t), out.ctypes.data)
    assert rc == 0
    return out


def host_batch_embed(frames, table, bits, k, index, search=0, rule="reference", key=None, first_frame=0, order_key=None):
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    nb = n_blocks_of(frames[0])
    pos = 0
    for f in range(frames.shape[0]):
        if pos < bits.size:
            out[f], used = host_embed(frames[f], table, bits[pos:], k, index, search, rule, key, first_frame + f,
                                      dl._perm(order_key, first_frame + f, nb))
            pos += used
        else:
            out[f] = frames[f]
    return out, pos


def host_batch_extract(frames, table, k, index, key=None, first_frame=0, order_key=None):
    nb = n_blocks_of(frames[0])
    return np.concatenate([host_extract(frames[f], table, k, index, key, first_frame + f, dl._perm(order_key, first_frame + f, nb))
                           for f in range(frames.shape[0])])


PLAN_FIELDS = ("path", "rows", "qm", "n_ac", "keyed", "steps_on", "table_count", "use", "tile_floats")


def host_plan(embed, k, search, total, n_bits, flags=0, index=None, table=None):
    """the route of a matrix call (csrc/svs_route.hpp) -> dict of PLAN_FIELDS"""
    table = np.ascontiguousarray(st.uniform(20) if table is None else table, np.uint16)
    idx = None if index is None else np.ascontiguousarray(index, np.uint8)
    out = np.zeros(9, np.int64)
    rc = emu().matrix_emu_plan(int(embed), int(k), int(search), int(total), int(n_bits), int(flags),
                               None if idx is None else idx.ctypes.data, 0 if idx is None else int(idx.size), table.ctypes.data,
                               out.ctypes.data)
    assert rc == 0
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))
