"""Helpers of the stepped soft tests (tests/test_stepped_soft_cpu.py, tests/test_stepped_soft_gpu.py): the NumPy model of the
byte of svs_stepped_soft_extract* (include/svsdct.h) - soft_lib.model_bytes with the call's delta replaced by a float32 step per
coefficient, every step one float32 operation in the header's order, on stepped_lib's transforms and dither -, the tally and
the histogram folded from model bytes with svsdct.soft, the host build of the stepped soft block body
(tests/hostemu/stepped_soft_emu.cpp), and stepped_lib.survival's experiment read with the soft bytes."""
import ctypes as C

import numpy as np

import channel_lib as cl
import dither_lib as dl
import stepped_lib as st
from testlib import build_emu
from oracle.qim_dct_oracle import BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd
from svsdct import channel
from svsdct import soft as sv


# ---- the model ---------------------------------------------------------------------------------------------------------
def model_bytes(x, dk, stats=None):
    """float32 quantiser inputs x = c - d and their float32 steps dk (same shape) -> the soft bytes.  stats (optional dict) gains
    `half`, the inputs x / dk exactly on a half-integer, and `lattice`, the bytes with m = 127 whose x is exactly q * dk."""
    x, dk = np.asarray(x), np.asarray(dk)
    assert x.dtype == np.float32 and dk.dtype == np.float32
    r = x / dk                                              # float32 division
    q = np.rint(r).astype(np.int64)                         # round half to even: the stepped extract's own index
    x0 = q.astype(np.float32) * dk
    a = np.abs(x - x0)
    h = np.float32(0.5) * dk
    s = np.float32(254.0) / dk                              # one float32 division
    v = (h - a) * s
    assert r.dtype == x0.dtype == a.dtype == h.dtype == s.dtype == v.dtype == np.float32
    m = np.clip(np.trunc(v.astype(np.float64)), 0, 127).astype(np.int64)   # truncation toward zero, then the clamp
    if stats is not None:
        stats["half"] = stats.get("half", 0) + int((np.abs(r - np.floor(r)) == 0.5).sum())
        stats["lattice"] = stats.get("lattice", 0) + int(((a == 0) & (m == 127)).sum())
    return (((q & 1) << 7) | m).astype(np.uint8)


def model_soft(gray, table, n_ac=MAX_AC, index=None, key=None, t=0, perm=None, stats=None):
    """One frame -> the soft bytes in stream order (stepped_lib.model_extract with the byte in the place of the parity)"""
    _check_plane(gray)
    index = dl._index(n_ac, index)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    if index.size == 0:
        return np.zeros(0, np.uint8)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    blk = _blocks_view(np.float32(gray)).reshape(1, n_blocks, BLOCK, BLOCK)
    x = _fwd(blk).reshape(n_blocks, BLOCK * BLOCK)[:, index]
    if key is not None:
        x = x - st.dither_values(key, t, n_blocks, table)[:, index]
    dk = np.broadcast_to(st._steps_f32(table)[index][None, :], x.shape)
    return model_bytes(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dk), stats)[perm].reshape(-1)


def model_batch_soft(frames, table, n_ac=MAX_AC, index=None, key=None, first_frame=0, order_key=None, stats=None):
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    return np.concatenate([model_soft(frames[f], table, n_ac, index, key, first_frame + f,
                                      dl._perm(order_key, first_frame + f, n_blocks), stats) for f in range(frames.shape[0])])


def model_tally(soft, period, stream_bit0=0):
    """the tally of svs_stepped_soft_vote* from model bytes: the existing format (svsdct.soft.tally)"""
    return sv.tally(soft, period, stream_bit0)


def model_hist(soft, n_frames):
    """the rows of svs_stepped_soft_histogram* from model bytes: the existing format (svsdct.soft.byte_histogram)"""
    return sv.byte_histogram(soft, n_frames)


# ---- the stepped soft block body on the host --------------------------------------------------------------------------------
PLAN_FIELDS = ("path", "rows", "qm", "stepped", "soft", "vote", "hist", "keyed", "steps_on", "soft_on", "soft_vote", "soft_hist",
               "soft_table_count", "sel_count", "dith_on", "sizeof_soft_args")
KIND = {"soft": 0, "vote": 1, "hist": 2}
PATH_EXACT, QM_POW2 = 1, 2          # svs::ExtractPath::EXACT, svs::QM_POW2 (the kernel matrix names the instantiation <8, 2, ..>)


PROTOTYPES = {
    "stepped_soft_emu_bytes": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                         C.c_void_p]),
    "stepped_soft_emu_uniform": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                           C.c_void_p]),
    "stepped_soft_emu_plan": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64,
                                        C.c_void_p]),
}


def emu(build_dir=None):
    """tests/hostemu/stepped_soft_emu.cpp, compiled once per process with -ffp-contract=off into build_dir (the CPU test passes a
    temporary directory and so compiles the file itself, as stepped_lib.emu)"""
    return build_emu("stepped_soft_emu.cpp", PROTOTYPES, build_dir, ("-ffp-contract=off",))


def host_soft(gray, table, n_ac=MAX_AC, index=None, key=None, t=0):
    """one frame through extract_block_stepped_soft on the host, raster order -> the soft bytes"""
    index = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    blocks = st._to_blocks(np.ascontiguousarray(gray, np.uint8))
    out = np.full(blocks.shape[0] * index.size, 0xA5, np.uint8)
    rc = emu().stepped_soft_emu_bytes(blocks.ctypes.data, blocks.shape[0], table.ctypes.data, index.ctypes.data, int(index.size),
                                      int(key is not None), int(key or 0), int(t), out.ctypes.data)
    assert rc == 0
    return out


def host_uniform(gray, delta, n_ac=MAX_AC, index=None, key=None, t=0):
    """the same frame through extract_block_soft at one delta, as the route launches a soft call there"""
    index = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    blocks = st._to_blocks(np.ascontiguousarray(gray, np.uint8))
    out = np.full(blocks.shape[0] * index.size, 0xA5, np.uint8)
    rc = emu().stepped_soft_emu_uniform(blocks.ctypes.data, blocks.shape[0], float(delta), index.ctypes.data, int(index.size),
                                        int(key is not None), int(key or 0), int(t), out.ctypes.data)
    assert rc == 0
    return out


def host_plan(kind, n_ac, total=1000, flags=0, index=None, table=None, period=1, bit0=0):
    """the route and the launch tables of a stepped soft call (csrc/svs_route.hpp) -> dict of PLAN_FIELDS"""
    table = np.ascontiguousarray(st.uniform(20) if table is None else table, np.uint16)
    idx = None if index is None else np.ascontiguousarray(index, np.uint8)
    out = np.zeros(16, np.int64)
    rc = emu().stepped_soft_emu_plan(KIND[kind], int(n_ac), int(total), int(flags), None if idx is None else idx.ctypes.data,
                                     0 if idx is None else int(idx.size), table.ctypes.data, int(period), int(bit0), out.ctypes.data)
    assert rc == 0
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


# ---- embed, requantise, read soft: the survival table ----------------------------------------------------------------------
SURVIVAL_QUALITIES = (50, 40, 30)
# (label, selection, rule) - table matched(75, 2)
SURVIVAL_ROWS = (
    ("1..10; reference", st.ROW_1_10, "reference"),
    ("zig-zag 1..10; reference", st.ZZ_1_10, "reference"),
    ("zig-zag 1..10; nearest", st.ZZ_1_10, "nearest"),
    ("zig-zag 6..15; reference", st.ZZ_6_15, "reference"),
)


def survival_clip(index, seed=cl.SURVIVAL_SEED):
    """stepped_lib.survival's cover and payload: the cover drawn before the payload"""
    rng = np.random.default_rng(seed)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    payload = rng.integers(0, 2, (h // 8) * (w // 8) * len(index)).astype(np.uint8)
    return cover, payload


def survival(table, index, rule, qualities=SURVIVAL_QUALITIES, seed=cl.SURVIVAL_SEED):
    """stepped_lib.survival's experiment - three 96 x 160 frames of noise in [64, 192), one full-capacity copy per frame, through
    the channel at each quality - read with the model's soft bytes -> {quality: (errors of each copy alone, errors of the hard
    majority, errors of the soft vote soft.combine)}"""
    cover, payload = survival_clip(index, seed)
    stego = np.stack([st.model_embed(g, table, payload, rule=rule, index=index)[0] for g in cover])
    out = {}
    for q in qualities:
        got = cl.model_requantise(stego, channel.quality_steps(q))
        streams = [model_soft(g, table, index=index) for g in got]
        hard = np.array([s >> 7 for s in streams])
        single = [int((b != payload).sum()) for b in hard]
        majority = int(((2 * hard.sum(0) > len(streams)).astype(np.uint8) != payload).sum())
        bits, _ = sv.combine(np.concatenate(streams), payload.size)
        out[q] = (single, majority, int((bits != payload).sum()))
    return out


def format_survival(rows):
    """rows: [(label, {quality: (single, majority, soft)})]"""
    qs = list(rows[0][1])
    lines = ["| selection; rule | " + " | ".join(f"Q = {q}" for q in qs) + " |", "|---|" + "---|" * len(qs)]
    for label, e in rows:
        lines.append(f"| {label} | " + " | ".join("/".join(str(v) for v in e[q][0]) + f", {e[q][1]}, {e[q][2]}" for q in qs) + " |")
    return "\n".join(lines)
