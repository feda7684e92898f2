"""Helpers of the margin-pass tests (tests/test_readback_margin_cpu.py, tests/test_readback_margin_gpu.py): the host build of the
one-lane forms of the stepped read-back and the margin pass behind it (tests/hostemu/readback_margin_emu.cpp), the independent
verdict from stepped_soft_lib's NumPy soft bytes, the cases both tiers run, and the experiment table of the README (what the
requantisation channel leaves of a payload embedded with svs_stepped_embed_readback_margin* at several gates)."""
import ctypes as C

import numpy as np

import channel_lib as cl
import dither_lib as dl
import stepped_lib as stl
import stepped_readback_lib as srl
import stepped_soft_lib as ssl
from testlib import build_emu
from keyed_readback_lib import DITHER_KEY
from svsdct import channel

ORDER_KEY = srl.ORDER_KEY
GATES = (1, 32, 64, 96, 127)          # the CPU tier's
GPU_GATES = (32, 64, 127)
GPU_SHAPE = srl.GPU_SHAPE
FIRST_FRAME = srl.FIRST_FRAME

# ---- the one-lane forms on the host ---------------------------------------------------------------------------------------
PROTOTYPES = {
    "readback_margin_emu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64,
                                      C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
}


def emu(build_dir=None):
    """tests/hostemu/readback_margin_emu.cpp, compiled once per process with -ffp-contract=off (as stepped_readback_lib.emu)"""
    return build_emu("readback_margin_emu.cpp", PROTOTYPES, build_dir, ("-ffp-contract=off",))


def host_margin(stego0, table, n_ac, bits, gate, index=None, dither_key=None, block_key=None, first_frame=0, bit_offset=0,
                n_bits=None):
    """the stepped read-back and then the margin pass at `gate` on the host over a copy of `stego0`, the stego of
    svs_stepped_embed with the same arguments (one frame or a batch) -> (stego after both, (repaired, unrepaired, strengthened,
    weak), status of pass 1 per physical block: 0 reads back, 1 repaired, 2 left, 3 no payload; status of pass 2: 0 strong
    throughout, 1 strengthened, 2 weak, 3 no payload, 4 skipped for a wrong bit).  index None: the row-major prefix 1..n_ac."""
    frames = np.array(stego0 if stego0.ndim == 3 else stego0[None], np.uint8, order="C")
    f, h, w = frames.shape
    idx = np.ascontiguousarray(dl._index(n_ac, index), np.uint8)
    table = np.ascontiguousarray(table, np.uint16)
    bits = np.asarray(bits, np.uint8)
    packed = np.packbits(bits)
    packed = np.concatenate([packed, np.zeros((-packed.size) % 4 + 4, np.uint8)])
    n_bits = int(bits.size - bit_offset if n_bits is None else n_bits)
    status1 = np.zeros(f * (h // 8) * (w // 8), np.uint8)
    status2 = np.zeros_like(status1)
    counts = np.zeros(4, np.uint64)
    rc = emu().readback_margin_emu(frames.ctypes.data, f, h, w, table.ctypes.data, idx.ctypes.data, int(idx.size),
                                   packed.ctypes.data, packed.size, int(bit_offset), n_bits, int(dither_key is not None),
                                   int(dither_key or 0), int(block_key is not None), int(block_key or 0), int(first_frame),
                                   int(gate), status1.ctypes.data, status2.ctypes.data, counts.ctypes.data)
    assert rc == 0, "the host library refused the selection, the table or the gate"
    return (frames if stego0.ndim == 3 else frames[0]), tuple(int(c) for c in counts), status1, status2


# ---- the independent verdict: the receiver's soft bytes from NumPy ----------------------------------------------------------
def soft_slots(frames, table, bits, index, key=None, first_frame=0, order_key=None):
    """frames [F,H,W] -> per stream slot (a block's worth of payload bits): (a hard bit of it is wrong, its smallest m), from
    stepped_soft_lib's NumPy soft bytes - the receiver's, independent of the code under test.  bits: the payload from stream
    position 0."""
    n = len(index)
    soft = ssl.model_batch_soft(frames, table, n, index, key, first_frame, order_key)[: bits.size]
    slot = np.arange(bits.size) // n
    nslot = -(-bits.size // n)
    wrong = np.zeros(nslot, bool)
    np.logical_or.at(wrong, slot, (soft >> 7) != bits)
    m_min = np.full(nslot, 127, np.int64)
    np.minimum.at(m_min, slot, (soft & 127).astype(np.int64))
    return wrong, m_min


def slot_of_block(shape, n_bits, n, order_key=None, first_frame=0):
    """physical block (raster over the batch) -> its stream slot, -1 where it carries no payload"""
    f, h, w = shape
    bpf = (h // 8) * (w // 8)
    out = np.empty(f * bpf, np.int64)
    for t in range(f):
        perm = dl._perm(order_key, first_frame + t, bpf)            # stream slot -> physical block, or None
        slot = np.arange(bpf) if perm is None else np.argsort(np.asarray(perm))
        out[t * bpf:(t + 1) * bpf] = t * bpf + slot
    out[out * n >= n_bits] = -1
    return out


# ---- symbols and refusals: no case reaches the device ------------------------------------------------------------------------
def check_refusals(lib):
    """the library exports both calls; min_margin = 128 is refused, behind the steps check and ahead of the flags; unknown flags
    are refused; svs_stepped_embed* still refuses SVS_READBACK"""
    from svsdct import native
    from svsdct import steps as steps_mod
    for name in ("svs_stepped_embed_readback_margin_dev", "svs_stepped_embed_readback_margin"):
        assert name in native.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(native.MarginCounts) == 32
    planes = native.Planes.contiguous(1, 8, 8)
    table = steps_mod.steps_struct(stl.uniform(20))
    bad_table = steps_mod.steps_struct(stl.uniform(20))
    bad_table.delta[5] = 0
    done = C.c_uint64(7)

    def call(steps, gate, flags, name="svs_stepped_embed_readback_margin_dev", tail=(None, None)):
        rc = getattr(lib, name)(64, 64, C.byref(planes), None, None, None, C.byref(steps), 3, 128, 0, 3, gate, flags,
                                C.byref(done), *tail)
        return rc, lib.svs_last_error().decode()

    for name, tail in (("svs_stepped_embed_readback_margin_dev", (None, None)), ("svs_stepped_embed_readback_margin", (None,))):
        rc, msg = call(table, 128, 0, name, tail)
        assert rc == native.SVS_ERR_INVALID_ARG and "min_margin 128" in msg, (name, rc, msg)
        rc, msg = call(table, 64, 1 << 30, name, tail)                 # unknown flags
        assert rc == native.SVS_ERR_INVALID_ARG and "flags" in msg, (name, rc, msg)
        rc, msg = call(bad_table, 128, 1 << 30, name, tail)            # the steps check comes first
        assert rc == native.SVS_ERR_INVALID_ARG and "delta[5]" in msg, (name, rc, msg)
        rc, msg = call(table, 128, 1 << 30, name, tail)                # then the gate, ahead of the flags
        assert rc == native.SVS_ERR_INVALID_ARG and "min_margin 128" in msg, (name, rc, msg)
    rc = lib.svs_stepped_embed_dev(64, 64, C.byref(planes), None, None, None, C.byref(table), 3, 128, 0, 3, native.SVS_READBACK,
                                   C.byref(done), None)
    assert rc == native.SVS_ERR_INVALID_ARG and "flags" in lib.svs_last_error().decode()


# ---- the cases both tiers run: stepped_readback_lib's -----------------------------------------------------------------------
TABLES = srl.TABLES
OPTION_SETS = srl.OPTION_SETS
CONTENTS = srl.CONTENTS
frames_of = srl.frames_of
payload = srl.payload
gpu_cases = srl.gpu_cases


def case_stego(tname, kind, index, dither, order, rule, shape=GPU_SHAPE, short=7):
    """the plain stepped stego of a case -> (stego0, bits, keyword arguments of host_margin / the verdict's (key, first_frame,
    order_key))"""
    f, h, w = shape
    bits = payload(f * (h // 8) * (w // 8) * len(index) - short)
    key, okey = (DITHER_KEY if dither else None), (ORDER_KEY if order else None)
    s0, used = srl.model_stego(frames_of(kind, shape), TABLES[tname], bits, index, rule, key, FIRST_FRAME, okey)
    assert used == bits.size
    return s0, bits, dict(index=index, dither_key=key, block_key=okey, first_frame=FIRST_FRAME), (key, FIRST_FRAME, okey)


# ---- the experiment (README.md, "soft-margin pass") -------------------------------------------------------------------------
EXP_SHAPE = srl.EXP_SHAPE
EXP_BITS = srl.EXP_BITS
EXP_GATES = (0, 48, 64, 96)
EXP_QUALITIES = (85, 75, 50)
# (table, selection, content): reference rule, no dither, no order
EXP_ROWS = (
    ("m75x2", "row-major 1..10", "noise"),
    ("m75x2", "zig-zag 1..10", "letterbox"),
    ("m75x2", "row-major 1..10", "letterbox"),
    ("u20", "row-major 1..10", "noise"),
)
EXP_SELECTIONS = srl.EXP_SELECTIONS
NOISE_ROW = EXP_ROWS[0]
LETTERBOX_ROWS = EXP_ROWS[1:3]
ASSERTED_GATE, ASSERTED_Q = 64, 75


def experiment_clip(tname, sname, kind):
    """three 96 x 160 frames of readback_lib.content(kind, seed = 3 + t), one 2 400-bit copy per frame -> (cover, plain stepped
    stego, bits, table, index)"""
    table, index = TABLES[tname], EXP_SELECTIONS[sname]
    cover = frames_of(kind, EXP_SHAPE)
    bits = payload(EXP_BITS, seed=29)
    plain = np.stack([stl.model_embed(g, table, bits, len(index), "reference", index)[0] for g in cover])
    return cover, plain, bits, table, index


def experiment_stego(plain, table, index, bits, gate):
    """the clip after the read-back and the margin pass at `gate` (0: the read-back alone), frame by frame -> (stego, counts)"""
    out = np.empty_like(plain)
    total = np.zeros(4, np.int64)
    for t in range(plain.shape[0]):
        out[t], c, _, _ = host_margin(plain[t], table, len(index), bits, gate, index=index)
        total += c
    return out, tuple(int(c) for c in total)


def experiment_row(tname, sname, kind):
    cover, plain, bits, table, index = experiment_clip(tname, sname, kind)

    def errors(stack):
        return sum(srl.bit_errors(stack[t:t + 1], table, bits, index) for t in range(stack.shape[0]))

    row = {"plain": {q: errors(cl.model_requantise(plain, channel.quality_steps(q))) for q in EXP_QUALITIES}, "gates": {}}
    for g in EXP_GATES:
        stego, counts = experiment_stego(plain, table, index, bits, g)
        row["gates"][g] = {"counts": counts, "direct": errors(stego), "psnr": stl.psnr_pooled(stego, cover),
                           "q": {q: errors(cl.model_requantise(stego, channel.quality_steps(q))) for q in EXP_QUALITIES}}
    return row


def experiment_table():
    return [(key, experiment_row(*key)) for key in EXP_ROWS]


def format_experiment(rows):
    names = {"u20": "uniform 20", "m75x2": "matched(75, 2)"}
    gates = " / ".join(str(g) for g in EXP_GATES)
    lines = [f"| steps; selection; content | strengthened, weak at g = {' / '.join(str(g) for g in EXP_GATES[1:])} | "
             + " | ".join(f"Q = {q}: plain; g = {gates}" for q in EXP_QUALITIES)
             + f" | PSNR against the cover, dB, g = {gates} |",
             "|---|---|" + "---|" * len(EXP_QUALITIES) + "---|"]
    for (tname, sname, kind), r in rows:
        g = r["gates"]
        lines.append(f"| {names[tname]}; {sname}; `{kind}` | "
                     + " / ".join(f"{g[k]['counts'][2]}, {g[k]['counts'][3]}" for k in EXP_GATES[1:]) + " | "
                     + " | ".join(f"{r['plain'][q]}; " + " / ".join(str(g[k]["q"][q]) for k in EXP_GATES) for q in EXP_QUALITIES)
                     + " | " + " / ".join(f"{g[k]['psnr']:.2f}" for k in EXP_GATES) + " |")
    return "\n".join(lines)
