"""Helpers of the per-coefficient-step tests (tests/test_stepped_cpu.py, tests/test_stepped_gpu.py): the NumPy model of the format
(include/svsdct.h, "per-coefficient QIM steps") - dither_lib.model_embed / model_extract with the call's delta replaced by a
float32 step per coefficient, every step one float32 operation in the header's order, built from the oracle's block view and its
pocketfft forward and inverse -, the tables, frames and options the GPU test runs, the host build of the stepped block bodies of
csrc/svs_block.hpp (tests/hostemu/stepped_emu.cpp), and the survival experiment of channel_lib with a table in place of delta."""
import ctypes as C

import numpy as np

import channel_lib as cl
import dither_lib as dl
import minmove_lib as ml
import soft_lib as sl
from testlib import build_emu
from oracle.qim_dct_oracle import BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _inv, bits_from_any
from svsdct import channel

RULES = ("reference", "nearest", "minmove")
RULE_KIND = {"reference": 0, "nearest": 1, "minmove": 2}


# ---- tables (restated here: svsdct/steps.py is code under test) ------------------------------------------------------------------
def uniform(d):
    t = np.full(64, int(d), np.uint16)
    t[0] = 0
    return t


def matched(codec_steps_or_quality, multiple=2, floor=0):
    """delta[k] = s_k * max(multiple, ceil(floor / s_k)), delta[0] = 0"""
    s = (channel.quality_steps(codec_steps_or_quality) if np.ndim(codec_steps_or_quality) == 0
         else np.asarray(codec_steps_or_quality)).astype(np.int64).reshape(64)
    t = s * np.maximum(int(multiple), -(-int(floor) // s))
    t[0] = 0
    return t.astype(np.uint16)


def odd_steps():
    """63 distinct odd steps that are no power of two (none is: they are odd and above 1), entry 0 unused"""
    t = np.zeros(64, np.uint16)
    t[1:] = cl.odd_steps()[:63]
    return t


TABLES = {
    "u20": uniform(20),
    "u16": uniform(16),
    "u7": uniform(7),
    "m75x2": matched(75, 2),
    "m50x3": matched(50, 3),
    "odd": odd_steps(),
    "all4095": uniform(4095),
}
UNIFORM = {"u20": 20, "u16": 16, "u7": 7}


# ---- the model ---------------------------------------------------------------------------------------------------------
def _steps_f32(table):
    t = np.asarray(table).reshape(64).astype(np.float32)
    return t


def band(table):
    """r_k = fmaxf(0, 0.5f * dk - MARGIN[k]) -> float32 [64]"""
    return np.maximum(np.float32(0.0), np.float32(0.5) * _steps_f32(table) - ml.margin_table())


def dither_values(key, t, n_blocks, table):
    """float32 [N][64]: d = r * dk, r the dithered calls' (dither_table at delta = 1 is r itself: r * 1.0f is exact)"""
    d = dl.dither_table(key, t, n_blocks, 1.0) * _steps_f32(table)[None, :]
    assert d.dtype == np.float32
    return d


def model_embed(gray, table, payload, n_ac=MAX_AC, rule="reference", index=None, key=None, t=0, perm=None, stats=None):
    """One frame; dither_lib.model_embed with dk = float32(table[k]) in place of delta.  Returns (stego uint8, bits consumed).
    stats (optional dict) gains `half`, the quantiser inputs (c - d) / dk exactly on a half-integer, and `zero`, the payload
    coefficients exactly 0 (added to what is there)."""
    assert rule in RULES
    _check_plane(gray)
    gray = np.ascontiguousarray(gray, np.uint8)
    bits = bits_from_any(payload)
    index = dl._index(n_ac, index)
    n_use = int(index.size)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    budget = int(bits.size)
    out_f = np.float32(gray)
    if budget == 0:
        return gray.copy(), 0
    if n_use == 0:
        touched, consumed = n_blocks, 0
    else:
        touched = min(n_blocks, -(-budget // n_use))
        consumed = min(budget, n_blocks * n_use)
    full = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)
    where = perm[:touched]
    coef = _fwd(full[where].reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK * BLOCK)
    if consumed:
        use = bits[:consumed].astype(np.int64)
        bi = np.arange(consumed) // n_use
        ki = index[np.arange(consumed) % n_use]
        dk = _steps_f32(table)[ki]
        c = coef[bi, ki]
        if key is not None:
            d = dither_values(key, t, n_blocks, table)[where[bi], ki]
            cq = c - d
        else:
            cq = c
        x = cq / dk
        assert cq.dtype == np.float32 and x.dtype == np.float32
        q = np.rint(x).astype(np.int64)
        wrong = (q & 1) != use
        step = np.where(use == 1, 1, -1)
        if rule != "reference":
            c0 = q.astype(np.float32) * dk
            step = np.where(cq > c0, 1, np.where(cq < c0, -1, step))
        ct = np.where(wrong, q + step, q).astype(np.float32) * dk
        if rule == "minmove":
            r = band(table)[ki]
            new = np.minimum(np.maximum(cq, ct - r), ct + r)
        else:
            new = ct
        assert new.dtype == np.float32
        if key is not None:
            new = np.where(new.view(np.uint32) == cq.view(np.uint32), c, new + d)
            assert new.dtype == np.float32
        coef[bi, ki] = new
        if stats is not None:
            stats["half"] = stats.get("half", 0) + int((np.abs(x - np.floor(x)) == 0.5).sum())
            stats["zero"] = stats.get("zero", 0) + int((c == 0).sum())
    rec = _inv(coef.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK, BLOCK)
    full[where] = rec
    out_f = full.reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
    return np.uint8(np.clip(out_f, 0, 255)), int(consumed)


def model_extract(gray, table, n_ac=MAX_AC, index=None, key=None, t=0, perm=None, stats=None):
    """One frame -> 0/1 bits in stream order: rintf((c - d) / dk) & 1"""
    _check_plane(gray)
    index = dl._index(n_ac, index)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    if index.size == 0:
        return np.zeros(0, np.uint8)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    blk = _blocks_view(np.float32(gray)).reshape(1, n_blocks, BLOCK, BLOCK)
    coef = _fwd(blk).reshape(n_blocks, BLOCK * BLOCK)[:, index]
    if key is not None:
        coef = coef - dither_values(key, t, n_blocks, table)[:, index]
    x = coef / _steps_f32(table)[index][None, :]
    assert x.dtype == np.float32
    if stats is not None:
        stats["half"] = stats.get("half", 0) + int((np.abs(x - np.floor(x)) == 0.5).sum())
    return (np.rint(x).astype(np.int64) & 1).astype(np.uint8)[perm].reshape(-1)


def model_batch_embed(frames, table, bits, n_ac=MAX_AC, rule="reference", index=None, key=None, first_frame=0, order_key=None):
    """the frame loop of oracle.batch_embed over model_embed: frame f is clip frame first_frame + f -> (stego, consumed)"""
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    pos = 0
    for f in range(frames.shape[0]):
        if pos < bits.size:
            out[f], used = model_embed(frames[f], table, bits[pos:], n_ac, rule, index, key, first_frame + f,
                                       dl._perm(order_key, first_frame + f, n_blocks))
            pos += used
        else:
            out[f] = frames[f]
    return out, pos


def model_batch_extract(frames, table, n_ac=MAX_AC, index=None, key=None, first_frame=0, order_key=None):
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    return np.concatenate([model_extract(frames[f], table, n_ac, index, key, first_frame + f,
                                         dl._perm(order_key, first_frame + f, n_blocks)) for f in range(frames.shape[0])])


# ---- what the GPU test runs (tests/test_stepped_gpu.py) -------------------------------------------------------------------------
SHAPES = cl.SHAPES              # (1, 8, 8) and kernel_matrix.SHAPES' (3, 48, 272) and (3, 40, 200)
PITCHED = cl.PITCHED
CONTENTS = ("full", "mid", "flat")
N_AC = 10
SELECTION = tuple(int(k) for k in sl.ZIGZAG[5:15])     # zig-zag scan positions 6 .. 15: not a prefix
ORDER_KEY = 0x0123456789ABCDEF
DITHER_KEY = 0xFEDCBA9876543210
FIRST_FRAME = 7
# name -> (order key, selection, dither key)
OPTIONS = {
    "plain": (None, None, None),
    "order": (ORDER_KEY, None, None),
    "select": (None, SELECTION, None),
    "dither": (None, None, DITHER_KEY),
    "all": (ORDER_KEY, SELECTION, DITHER_KEY),
}
BIT_OFFSET = 13                 # not a multiple of 32


def content(kind, shape):
    return cl.content(kind, shape)


def payload_for(shape, n_ac=N_AC, seed=3):
    """a payload that ends inside a block of the last frame: the capacity less 3 n_ac + 4 bits (one block: 6 bits)"""
    f, h, w = shape
    cap = f * (h // 8) * (w // 8) * n_ac
    n = cap - 3 * n_ac - 4 if cap > 4 * n_ac else 6
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


# ---- the stepped block bodies on the host ---------------------------------------------------------------------------------------
PROTOTYPES = {
    "stepped_emu_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                    C.c_int, C.c_uint64, C.c_uint32]),
    "stepped_emu_extract": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p]),
    "stepped_emu_plan": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}


def emu(build_dir=None):
    """tests/hostemu/stepped_emu.cpp, compiled once per process with -ffp-contract=off into build_dir (the CPU test passes a
    temporary directory and so compiles the file itself, as tests/test_requantise_cpu.py compiles channel_emu.cpp)"""
    return build_emu("stepped_emu.cpp", PROTOTYPES, build_dir, ("-ffp-contract=off",))


def _to_blocks(plane):
    h, w = plane.shape
    return np.ascontiguousarray(plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)).reshape(-1, 64)


def _from_blocks(blocks, h, w):
    return np.ascontiguousarray(blocks.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w))


def host_embed(gray, table, payload, n_ac=MAX_AC, rule="reference", index=None, key=None, t=0):
    """one frame through embed_block_stepped on the host, raster order -> stego uint8"""
    index = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    bits = np.ascontiguousarray(bits_from_any(payload), np.uint8)
    blocks = _to_blocks(np.ascontiguousarray(gray, np.uint8))
    out = np.empty_like(blocks)
    rc = emu().stepped_emu_embed(blocks.ctypes.data, out.ctypes.data, blocks.shape[0], table.ctypes.data, index.ctypes.data,
                                 int(index.size), bits.ctypes.data, int(bits.size), RULE_KIND[rule], int(key is not None),
                                 int(key or 0), int(t))
    assert rc == 0
    return _from_blocks(out, *gray.shape)


def host_extract(gray, table, n_ac=MAX_AC, index=None, key=None, t=0):
    index = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    blocks = _to_blocks(np.ascontiguousarray(gray, np.uint8))
    out = np.zeros(blocks.shape[0] * index.size, np.uint8)
    rc = emu().stepped_emu_extract(blocks.ctypes.data, blocks.shape[0], table.ctypes.data, index.ctypes.data, int(index.size),
                                   int(key is not None), int(key or 0), int(t), out.ctypes.data)
    assert rc == 0
    return out


PLAN_FIELDS = ("path", "rows", "qm", "stepped", "selected", "dithered", "keyed", "steps_on", "table_count", "use")


def host_plan(embed, n_ac, total, n_bits, flags=0, index=None, table=None):
    """the route of a stepped call (csrc/svs_route.hpp) -> dict of PLAN_FIELDS"""
    table = np.ascontiguousarray(uniform(20) if table is None else table, np.uint16)
    idx = None if index is None else np.ascontiguousarray(index, np.uint8)
    out = np.zeros(10, np.int64)
    rc = emu().stepped_emu_plan(int(embed), int(n_ac), int(total), int(n_bits), int(flags), None if idx is None else idx.ctypes.data,
                                0 if idx is None else int(idx.size), table.ctypes.data, out.ctypes.data)
    assert rc == 0
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


# ---- embed, requantise, read: the survival table ------------------------------------------------------------------------------
ZZ_1_10 = tuple(int(k) for k in sl.ZIGZAG[:10])
ZZ_2_11 = tuple(int(k) for k in sl.ZIGZAG[1:11])
ZZ_6_15 = tuple(int(k) for k in sl.ZIGZAG[5:15])
ROW_1_10 = tuple(range(1, 11))


def psnr_pooled(a, b):
    e = float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    return float("inf") if e == 0 else 10 * np.log10(255.0 ** 2 * a.size / e)


def survival(table, index, rule, qualities=cl.QUALITIES, seed=cl.SURVIVAL_SEED):
    """channel_lib.survival's experiment with a step table: three 96 x 160 frames of noise in [64, 192), cover drawn before the
    payload, one full-capacity copy per frame, through the channel at each quality -> (PSNR against the cover pooled over the
    frames, {quality: [bit errors of each copy]})"""
    rng = np.random.default_rng(seed)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    payload = rng.integers(0, 2, (h // 8) * (w // 8) * len(index)).astype(np.uint8)
    stego = np.stack([model_embed(g, table, payload, rule=rule, index=index)[0] for g in cover])
    errors = {}
    for q in qualities:
        got = cl.model_requantise(stego, channel.quality_steps(q))
        errors[q] = [int((model_extract(g, table, index=index) != payload).sum()) for g in got]
    return psnr_pooled(stego, cover), errors


# (label, selection, table or None for matched(75, 2), rule) - the rows of the README's table
SURVIVAL_ROWS = (
    ("1..10; uniform 20; reference", ROW_1_10, uniform(20), "reference"),
    ("1..10; uniform 40; reference", ROW_1_10, uniform(40), "reference"),
    ("1..10; matched; reference", ROW_1_10, None, "reference"),
    ("1..10; matched; nearest", ROW_1_10, None, "nearest"),
    ("zig-zag 1..10; uniform 20; reference", ZZ_1_10, uniform(20), "reference"),
    ("zig-zag 1..10; matched; reference", ZZ_1_10, None, "reference"),
    ("zig-zag 1..10; matched; nearest", ZZ_1_10, None, "nearest"),
    ("zig-zag 2..11; uniform 20; reference", ZZ_2_11, uniform(20), "reference"),
    ("zig-zag 2..11; matched; reference", ZZ_2_11, None, "reference"),
    ("zig-zag 2..11; matched; nearest", ZZ_2_11, None, "nearest"),
    ("zig-zag 6..15; uniform 20; reference", ZZ_6_15, uniform(20), "reference"),
    ("zig-zag 6..15; matched; reference", ZZ_6_15, None, "reference"),
)


def survival_table():
    """-> [(label, steps of the selection, PSNR, {quality: errors})] of SURVIVAL_ROWS"""
    rows = []
    for label, index, table, rule in SURVIVAL_ROWS:
        table = matched(75, 2) if table is None else table
        p, e = survival(table, index, rule)
        rows.append((label, [int(table[k]) for k in index], p, e))
    return rows


def format_survival(rows):
    lines = ["| selection; steps; rule | steps of the selection | PSNR dB | " + " | ".join(f"Q = {q}" for q in cl.QUALITIES) + " |",
             "|---|---|---|" + "---|" * len(cl.QUALITIES)]
    for label, st, p, e in rows:
        shown = str(st[0]) if len(set(st)) == 1 else ",".join(str(v) for v in st)
        lines.append(f"| {label} | {shown} | {p:.2f} | " + " | ".join("/".join(str(v) for v in e[q]) for q in cl.QUALITIES) + " |")
    return "\n".join(lines)
