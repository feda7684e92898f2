"""The soft-margin pass behind the stepped read-back on the GPU (svs_stepped_embed_readback_margin*): the gated stepped body of
readback_kernel equals the host build of the same arithmetic (csrc/svs_readback.hpp via tests/hostemu/readback_margin_emu.cpp)
byte for byte and count for count, starting from the bytes of svs_stepped_embed - five tables, the rotated option sets, four
contents, three gates, on frames whose waves straddle frames and end ragged - in place, on pitched planes, at a bit offset that
is no multiple of 32, with a payload that ends inside a block, and over several staging chunks; gate 0 is
svs_stepped_embed_readback_dev; the product's own soft histogram finds no byte below the gate; and the device reproduces the
host model's error count after the requantisation channel.
On the parent commit every test of this file fails: the library has neither symbol, so native.load() cannot attach the
signatures (the refusal test, the gate-0 test and every parity test alike)."""
import ctypes as C

import numpy as np
import pytest

import channel_lib as cl
import dither_lib
import keyed_readback_lib as kl
import readback_margin_lib as rml
import stepped_readback_lib as srl
from test_gpu_parity import _Dev
from svsdct import batch, channel, native
from svsdct.native import Planes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KEY = kl.DITHER_KEY
ORDER_KEY = rml.ORDER_KEY
# 3 x 56 x 136: 119 blocks per frame, 357 in all - two workgroups, a partial last wave (37 blocks), waves that straddle frames
F, H, W = rml.GPU_SHAPE
FIRST = rml.FIRST_FRAME


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _keywords(index, dither, keyed, rule, first):
    kw = dict(first_frame=first, nearest=rule == "nearest", minmove=rule == "minmove")
    if not kl.prefix(len(index)) == tuple(index):
        kw["coeffs"] = list(index)
    if dither:
        kw["dither_key"] = KEY
    if keyed:
        kw["block_key"] = ORDER_KEY
    return kw


def embed_pair(frames, table, index, bits, gate, dither, keyed, rule, first=FIRST, **more):
    """(the stego of svs_stepped_embed, the new call's stego, its four counts) through the host-pointer calls"""
    kw = dict(_keywords(index, dither, keyed, rule, first), steps=table, **more)
    s0, used0 = batch.embed_frames(frames, 1.0, len(index), bits, **kw)
    s1, used1, counts = batch.embed_frames(frames, 1.0, len(index), bits, readback_margin=gate, **kw)
    assert used0 == used1
    return np.array(s0), np.array(s1), tuple(counts)


def emulate(s0, table, index, bits, gate, dither, keyed, first=FIRST, **kw):
    return rml.host_margin(s0, table, len(index), bits, gate, index=index, dither_key=KEY if dither else None,
                           block_key=ORDER_KEY if keyed else None, first_frame=first, **kw)


CASES = rml.gpu_cases()


# ---- (a) device equals host emulation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", rml.GPU_GATES)
@pytest.mark.parametrize("tname,kind,index,dither,keyed,rule", CASES,
                         ids=[f"{c[0]}-{c[1]}-{len(c[2])}@{c[2][0]}-{'d' if c[3] else 'p'}{'k' if c[4] else 'r'}-{c[5]}" for c in CASES])
def test_gpu_equals_host_emulation(tname, kind, index, dither, keyed, rule, gate):
    table = rml.TABLES[tname]
    frames = rml.frames_of(kind)
    bits = dither_lib.payload(batch.capacity_bits(F, H, W, len(index)) - 37)      # ends inside a block
    s0, s1, counts = embed_pair(frames, table, index, bits, gate, dither, keyed, rule)
    want, want_counts, _, _ = emulate(s0, table, index, bits, gate, dither, keyed)
    print(f"{tname}, {kind}, {len(index)} from {index[0]}, dither {dither}, keyed {keyed}, {rule}, g = {gate}: "
          f"host counts {want_counts}; GPU counts {counts}")
    assert np.array_equal(s1, want), np.argwhere(s1 != want)[:4]
    assert counts == want_counts


def test_the_parity_cases_strengthen_and_leave_weak_blocks():
    """the cases above are not vacuous: on the host, over a third of them, the pass strengthens blocks at gates 32 and 64 and leaves
    weak ones at 127 (where the stored block's own rounding keeps nearly every block from getting there)"""
    total = {g: np.zeros(4, np.int64) for g in rml.GPU_GATES}
    for tname, kind, index, dither, keyed, rule in CASES[::3]:
        s0, bits, kw, _ = rml.case_stego(tname, kind, index, dither, keyed, rule, short=37)
        for g in total:
            total[g] += rml.host_margin(s0, rml.TABLES[tname], len(index), bits, g, **kw)[1]
    print({g: tuple(int(v) for v in c) for g, c in total.items()})
    assert total[32][2] > 0 and total[64][2] > total[32][2] and total[127][3] > 0


# ---- (b) the _dev call in place and on pitched planes, at an odd bit offset, with counts that are added to -----------------
def _ref(x):
    return C.byref(x) if x is not None else None


def _device_calls(frames, table, index, stream, off, n_bits, gate, dither, keyed, rule, first, pitched=False,
                  preset=(5, 7, 11, 13), call="margin"):
    """svs_stepped_embed_dev in place, then the new device call (or, call = "readback", svs_stepped_embed_readback_dev) in place
    from the cover, on tight or pitched planes with sentinels in the padding -> (stego without the passes, stego with, the four
    counts added to `preset`)"""
    lib = native.load()
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    view = lambda a: np.lib.stride_tricks.as_strided(a, (f, h, w), (frame_pitch, row_pitch, 1))   # noqa: E731
    view(host)[...] = frames
    pad = np.ones(host.size, bool)
    view(pad)[...] = False
    packed = batch.pack_bits(stream)
    d, d_bits, d_counts = _Dev(host.size), _Dev(packed.size + 8), _Dev(32)
    d_bits.put(packed)
    dith = native.Dither(KEY, first, 0) if dither else None
    odr = batch.block_order(ORDER_KEY if keyed else None, first)
    sel = native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
    steps = batch._steps_arg(table)
    flags = batch.embed_flags(None, rule == "nearest", rule == "minmove")
    done = C.c_uint64(0)
    d.put(host)
    native.check(lib.svs_stepped_embed_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), _ref(dith), C.byref(steps),
                                           len(index), d_bits.ptr, off, n_bits, flags, C.byref(done), None), "svs_stepped_embed_dev")
    native.check(lib.svs_stream_synchronize(None), "sync")
    plain = d.get()
    d.put(host)
    d_counts.put(np.array(preset, np.uint64))
    if call == "margin":
        native.check(lib.svs_stepped_embed_readback_margin_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), _ref(dith),
                                                               C.byref(steps), len(index), d_bits.ptr, off, n_bits, gate, flags,
                                                               C.byref(done), d_counts.ptr, None),
                     "svs_stepped_embed_readback_margin_dev")
    else:
        native.check(lib.svs_stepped_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), _ref(dith),
                                                        C.byref(steps), len(index), d_bits.ptr, off, n_bits, flags, C.byref(done),
                                                        d_counts.ptr, None), "svs_stepped_embed_readback_dev")
    native.check(lib.svs_stream_synchronize(None), "sync")
    out = d.get()
    assert (plain[pad] == 0xAB).all() and (out[pad] == 0xAB).all()          # sentinel padding is untouched
    assert done.value == n_bits
    return view(plain).copy(), view(out).copy(), tuple(int(c) for c in d_counts.get(32, np.uint64))


@pytest.mark.parametrize("pitched", (False, True), ids=("tight", "pitched"))
def test_device_call_in_place_with_counts(pitched):
    table, index, off, gate = rml.TABLES["m75x2"], kl.zigzag(10), 45, 64
    frames = rml.frames_of("letterbox")
    n_bits = batch.capacity_bits(F, H, W, 10) - 13
    stream = dither_lib.payload(off + n_bits + 50)
    s0, s1, counts = _device_calls(frames, table, index, stream, off, n_bits, gate, True, True, "minmove", 2, pitched=pitched)
    want, c, _, _ = emulate(s0, table, index, stream, gate, True, True, first=2, bit_offset=off, n_bits=n_bits)
    print(f"host counts {c}")
    assert c[0] > 30 and c[2] > 0
    assert np.array_equal(s1, want) and counts == (c[0] + 5, c[1] + 7, c[2] + 11, c[3] + 13)


# ---- (c) gate 0 ------------------------------------------------------------------------------------------------------------
def test_gate_0_is_the_stepped_readback_call():
    """min_margin = 0: the bytes and the first two counts of svs_stepped_embed_readback_dev, the last two untouched; the counts are
    added to, not overwritten"""
    table, index, off = rml.TABLES["m75x2"], kl.zigzag(10), 45
    frames = rml.frames_of("letterbox")
    n_bits = batch.capacity_bits(F, H, W, 10) - 13
    stream = dither_lib.payload(off + n_bits + 50)
    args = (frames, table, index, stream, off, n_bits, 0, True, True, "minmove", 2)
    _, base, base_counts = _device_calls(*args, call="readback")
    _, new, new_counts = _device_calls(*args, call="margin")
    assert base_counts[0] > 5 + 30 and base_counts[2:] == (11, 13)           # the read-back call writes two counts
    assert np.array_equal(new, base) and new_counts == base_counts


# ---- (d) the host form over several staging chunks ------------------------------------------------------------------------
def test_host_call_over_several_staging_chunks():
    """five letterboxed 1080p frames travel as whole frames in several chunks: each chunk's first frame feeds the order and the
    dither, the four counts are summed"""
    f, h, w, index, off, gate = 5, 1080, 1920, kl.zigzag(10), 77, 64
    table = rml.TABLES["m75x2"]
    frames = rml.frames_of("letterbox", (f, h, w))
    cap = batch.capacity_bits(f, h, w, 10)
    bits = dither_lib.payload(off + cap - 1234)
    s0, s1, counts = embed_pair(frames, table, index, bits, gate, True, True, "minmove", bit_offset=off)
    want, want_counts, _, _ = emulate(s0, table, index, bits, gate, True, True, bit_offset=off)
    print(f"host counts {want_counts}")
    assert want_counts[0] > 10000 and want_counts[2] > 100
    assert counts == want_counts and np.array_equal(s1, want)


# ---- (e) the product's own receiver -----------------------------------------------------------------------------------------
def test_the_soft_histogram_of_the_output_is_empty_below_the_gate():
    """a full-capacity payload on a case that the host build ends with weak = unrepaired = 0: svs_stepped_soft_histogram_dev on the
    device call's output counts no byte with m < g, of either bit"""
    table, index, gate = rml.TABLES["m75x2"], kl.zigzag(10), 64
    frames = rml.frames_of("letterbox")
    n_bits = batch.capacity_bits(F, H, W, 10)
    stream = dither_lib.payload(n_bits)
    s0, s1, counts = _device_calls(frames, table, index, stream, 0, n_bits, gate, True, False, "reference", FIRST, preset=(0, 0, 0, 0))
    _, want_counts, _, _ = emulate(s0, table, index, stream, gate, True, False)
    assert counts == want_counts and counts[1] == 0 and counts[3] == 0 and counts[2] > 0
    d, d_hist = _Dev(s1.nbytes), _Dev(F * 1024)
    d.put(s1)
    d_hist.put(np.zeros(F * 256, np.uint32))
    n = batch.extract_histogram_device(d.ptr, Planes.contiguous(F, H, W), 1.0, 10, d_hist.ptr, first_frame=FIRST, coeffs=list(index),
                                       dither_key=KEY, steps=table)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    hist = d_hist.get(F * 1024, np.uint32).reshape(F, 256).astype(np.int64)
    assert n == n_bits and hist.sum() == n_bits
    low = hist[:, :gate] + hist[:, 128:128 + gate]
    print(f"counts {counts}; bytes with m < {gate}: {int(low.sum())}; smallest m present: {int(np.nonzero((hist[:, :128] + hist[:, 128:]).sum(0))[0][0])}")
    assert not low.any()
    # and the plain stepped stego does have such bytes: the assertion above is the pass's doing
    d.put(s0)
    d_hist.put(np.zeros(F * 256, np.uint32))
    batch.extract_histogram_device(d.ptr, Planes.contiguous(F, H, W), 1.0, 10, d_hist.ptr, first_frame=FIRST, coeffs=list(index),
                                   dither_key=KEY, steps=table)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    before = d_hist.get(F * 1024, np.uint32).reshape(F, 256).astype(np.int64)
    assert (before[:, :gate] + before[:, 128:128 + gate]).sum() > 0


# ---- (f) the round trip through the channel ---------------------------------------------------------------------------------
def test_the_device_reproduces_the_models_errors_after_the_channel():
    """the asserted row of the README's table - matched(75, 2), row-major 1..10, noise, g = 64, three 96 x 160 frames with one
    2 400-bit copy each: svs_stepped_embed_readback_margin_dev, svs_requantise_dev at Q = 75, svs_stepped_extract_dev on the
    device give exactly the host model's error count (tests/test_readback_margin_cpu.py asserts its size)"""
    tname, sname, kind = rml.NOISE_ROW
    gate, q = rml.ASSERTED_GATE, rml.ASSERTED_Q
    cover, plain, bits, table, index = rml.experiment_clip(tname, sname, kind)
    model, model_counts = rml.experiment_stego(plain, table, index, bits, gate)
    want = sum(srl.bit_errors(cl.model_requantise(model[t:t + 1], channel.quality_steps(q)), table, bits, index) for t in range(3))
    _, h, w = cover.shape
    planes = Planes.contiguous(1, h, w)
    packed = batch.pack_bits(bits)
    d, d_bits, d_counts, d_out = _Dev(h * w), _Dev(packed.size + 8), _Dev(32), _Dev(packed.size + 8)
    d_bits.put(packed)
    d_counts.put(np.zeros(4, np.uint64))
    errors = 0
    for t in range(3):
        d.put(cover[t])
        used = batch.embed_device(d.ptr, d.ptr, planes, 1.0, 10, d_bits.ptr, 0, bits.size, steps=table, readback_margin=gate,
                                  d_counts=d_counts.ptr)
        batch.requantise_device(d.ptr, d.ptr, planes, q)
        n = batch.extract_device(d.ptr, planes, 1.0, 10, d_out.ptr, packed.size + 8, steps=table)
        native.check(native.load().svs_stream_synchronize(None), "sync")
        assert used == bits.size and n == bits.size
        got = np.unpackbits(d_out.get(packed.size))[: bits.size]
        errors += int((got != bits).sum())
    counts = tuple(int(c) for c in d_counts.get(32, np.uint64))
    print(f"errors after Q = {q}: device {errors}, model {want}; counts device {counts}, model {model_counts}")
    assert counts == model_counts
    assert errors == want


# ---- (g) refusals: no device work -----------------------------------------------------------------------------------------
def test_refusals():
    """min_margin = 128; unknown flags; the steps check comes first; svs_stepped_embed* still refuses SVS_READBACK"""
    rml.check_refusals(native.load())
