"""Helpers of the stepped read-back tests (tests/test_stepped_readback_cpu.py, tests/test_stepped_readback_gpu.py): the host
build of the one-lane stepped forms of csrc/svs_readback.hpp (tests/hostemu/stepped_readback_emu.cpp), the cases both tiers
run, and the experiment table of the README (what the pass repairs on letterboxed frames, and what the requantisation channel
then leaves of the payload)."""
import ctypes as C

import numpy as np

import channel_lib as cl
import dither_lib as dl
import stepped_lib as stl
from testlib import build_emu
from keyed_readback_lib import DITHER_KEY, prefix, zigzag
from readback_lib import content
from svsdct import channel

ORDER_KEY = 0x0F1E2D3C4B5A6978
RULES = stl.RULES

# ---- the one-lane forms on the host ---------------------------------------------------------------------------------------
PROTOTYPES = {
    "stepped_readback_emu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64,
                                       C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p,
                                       C.c_void_p]),
    "stepped_readback_emu_reciprocals": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
}


def emu(build_dir=None):
    """tests/hostemu/stepped_readback_emu.cpp, compiled once per process with -ffp-contract=off (as stepped_lib.emu)"""
    return build_emu("stepped_readback_emu.cpp", PROTOTYPES, build_dir, ("-ffp-contract=off",))


def host_readback(stego0, table, n_ac, bits, index=None, dither_key=None, block_key=None, first_frame=0, bit_offset=0,
                  n_bits=None):
    """the stepped read-back pass on the host over a copy of `stego0`, the stego of svs_stepped_embed with the same arguments
    (one frame or a batch) -> (stego after the pass, (repaired, unrepaired), status per physical block: 0 reads back, 1
    repaired, 2 left, 3 carries no payload).  index None: the row-major prefix 1..n_ac."""
    frames = np.array(stego0 if stego0.ndim == 3 else stego0[None], np.uint8, order="C")
    f, h, w = frames.shape
    idx = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    bits = np.asarray(bits, np.uint8)
    packed = np.packbits(bits)
    packed = np.concatenate([packed, np.zeros((-packed.size) % 4 + 4, np.uint8)])
    n_bits = int(bits.size - bit_offset if n_bits is None else n_bits)
    status = np.zeros(f * (h // 8) * (w // 8), np.uint8)
    counts = np.zeros(2, np.uint64)
    rc = emu().stepped_readback_emu(frames.ctypes.data, f, h, w, table.ctypes.data, idx.ctypes.data, int(idx.size),
                                    packed.ctypes.data, packed.size, int(bit_offset), n_bits, int(dither_key is not None),
                                    int(dither_key or 0), int(block_key is not None), int(block_key or 0), int(first_frame),
                                    status.ctypes.data, counts.ctypes.data)
    assert rc == 0, "the host library refused the selection or the table"
    return (frames if stego0.ndim == 3 else frames[0]), (int(counts[0]), int(counts[1])), status


def reciprocals(n=4095):
    """-> (1.0f / dk, make_qim(dk).inv_delta_f) as float32 arrays for dk = 1..n"""
    own, qim = np.zeros(n, np.float32), np.zeros(n, np.float32)
    emu().stepped_readback_emu_reciprocals(n, own.ctypes.data, qim.ctypes.data)
    return own, qim


# ---- the model's stego and the independent verdict --------------------------------------------------------------------------
def model_stego(frames, table, bits, index, rule="reference", key=None, first_frame=0, order_key=None):
    """the stego of svs_stepped_embed from stepped_lib's NumPy model (frames [F,H,W]) -> (stego, bits consumed)"""
    return stl.model_batch_embed(frames, table, bits, len(index), rule, index, key, first_frame, order_key)


def bit_errors(frames, table, bits, index, key=None, first_frame=0, order_key=None):
    """payload bits that stepped_lib's NumPy extraction (the receiver, independent of the code under test) reads wrong"""
    got = stl.model_batch_extract(frames, table, len(index), index, key, first_frame, order_key)[: bits.size]
    return int((got != bits).sum())


def wrong_slots(frames, table, bits, index, key=None, first_frame=0, order_key=None):
    """bool per stream slot (a block's worth of bits) of the payload: the NumPy extraction reads a bit of it wrong"""
    n = len(index)
    got = stl.model_batch_extract(frames, table, n, index, key, first_frame, order_key)[: bits.size]
    bad = np.zeros(-(-bits.size // n), bool)
    np.logical_or.at(bad, np.arange(bits.size) // n, got != bits)
    return bad


# ---- the cases both tiers run ---------------------------------------------------------------------------------------------
def matched(q, m, floor=0):
    return stl.matched(q, m, floor)


TABLES = {
    "u20": stl.uniform(20),
    "m75x2": matched(75, 2),
    "m50x1": matched(50, 1),
    "m95x2f16": matched(95, 2, 16),
    "odd": stl.odd_steps(),
}
UNIFORM = {"u20": 20, "u16": 16, "u7": 7}
# (selection, dither, order, rule), rotated over tables and contents as test_keyed_readback_gpu.py rotates its CASES: dither x
# order x rule, prefix and non-prefix selections, 63 coefficients
OPTION_SETS = (
    (prefix(10), False, False, "reference"),
    (zigzag(10), True, False, "reference"),
    (zigzag(3, 6), True, True, "nearest"),
    (prefix(63), False, True, "minmove"),
    (zigzag(10), False, True, "reference"),
    (prefix(10), True, False, "minmove"),
    (zigzag(10), True, True, "minmove"),
    (prefix(63), True, False, "nearest"),
)
CONTENTS = ("letterbox", "bright", "flat0", "noise")
GPU_SHAPE = (3, 56, 136)
FIRST_FRAME = 5


def frames_of(kind, shape=GPU_SHAPE):
    f, h, w = shape
    return np.stack([content(kind, h, w, seed=3 + t) for t in range(f)])


def payload(n, seed=17):
    return np.random.default_rng(seed).integers(0, 2, int(n)).astype(np.uint8)


def gpu_cases():
    """(table name, content, selection, dither, order, rule): every table with every content once, the option sets rotated"""
    out = []
    i = 0
    for tname in TABLES:
        for kind in CONTENTS:
            out.append((tname, kind) + OPTION_SETS[i % len(OPTION_SETS)])
            i += 3          # 3 and 8 are coprime: every option set comes up, each table meets four different ones
    return out


# the delivery test of the GPU tier: one 96 x 160 letterboxed frame (keyed_readback_lib.table_frame, clip frame TABLE_T), dither,
# block key -> (table, selection, rule).  The issue's first setting; the CPU tier confirms that it leaves nothing unrepaired.
DELIVERY = (matched(75, 2), zigzag(10), "minmove")


# ---- the experiment (README.md, "stepped read-back") ------------------------------------------------------------------------
EXP_SHAPE = (3, 96, 160)
EXP_BITS = 2400
EXP_QUALITIES = (75, 50)
EXP_ROWS = tuple((tname, sname, rule)
                 for tname in ("u20", "m75x2")
                 for sname in ("row-major 1..10", "zig-zag 1..10")
                 for rule in ("reference", "nearest"))
EXP_SELECTIONS = {"row-major 1..10": prefix(10), "zig-zag 1..10": zigzag(10)}
ASSERTED_ROW = ("m75x2", "zig-zag 1..10", "reference")


def experiment_row(tname, sname, rule):
    """three letterboxed 96 x 160 frames, one 2 400-bit copy per frame -> dict of the row's cells"""
    table, index = TABLES[tname], EXP_SELECTIONS[sname]
    f, h, w = EXP_SHAPE
    cover = frames_of("letterbox", EXP_SHAPE)
    bits = payload(EXP_BITS, seed=29)
    plain = np.stack([stl.model_embed(cover[t], table, bits, len(index), rule, index)[0] for t in range(f)])
    failing = int(sum(wrong_slots(plain[t:t + 1], table, bits, index).sum() for t in range(f)))
    fixed = np.empty_like(plain)
    rep = left = 0
    for t in range(f):
        fixed[t], (r, u), _ = host_readback(plain[t], table, len(index), bits, index=index)
        rep, left = rep + r, left + u

    def errors(stack):
        return sum(bit_errors(stack[t:t + 1], table, bits, index) for t in range(f))

    row = {"failing": failing, "repaired": rep, "unrepaired": left, "direct": (errors(plain), errors(fixed)),
           "psnr": stl.psnr_pooled(fixed, plain)}
    for q in EXP_QUALITIES:
        s = channel.quality_steps(q)
        row[f"q{q}"] = (errors(cl.model_requantise(plain, s)), errors(cl.model_requantise(fixed, s)))
    return row


def experiment_table():
    return [((tname, sname, rule), experiment_row(tname, sname, rule)) for tname, sname, rule in EXP_ROWS]


def format_experiment(rows):
    names = {"u20": "uniform 20", "m75x2": "matched(75, 2)"}
    lines = ["| steps; selection; rule | blocks failing | repaired / unrepaired | bit errors read directly, without / with | "
             + " | ".join(f"after Q = {q}, without / with" for q in EXP_QUALITIES) + " | PSNR against the plain stepped stego, dB |",
             "|---|---|---|---|" + "---|" * len(EXP_QUALITIES) + "---|"]
    for (tname, sname, rule), r in rows:
        psnr = "inf" if np.isinf(r["psnr"]) else f"{r['psnr']:.2f}"
        lines.append(f"| {names[tname]}; {sname}; {rule} | {r['failing']} | {r['repaired']} / {r['unrepaired']} | "
                     f"{r['direct'][0]} / {r['direct'][1]} | "
                     + " | ".join(f"{r[f'q{q}'][0]} / {r[f'q{q}'][1]}" for q in EXP_QUALITIES) + f" | {psnr} |")
    return "\n".join(lines)
