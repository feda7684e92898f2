"""Per-coefficient QIM steps on the GPU (svs_stepped_embed* / svs_stepped_extract*, include/svsdct.h): the device output against
the NumPy model of the format (tests/stepped_lib.py) byte for byte and bit for bit - no tolerance: the model is pocketfft and the
exact kernels are pocketfft-identical - for every table, option set and rule of stepped_lib on clipping noise, mid noise and flat
frames (tests/test_stepped_cpu.py checks that these reach rounding ties and coefficients that are exactly 0); uniform tables against
the existing calls of the same build; the host forms across staging chunks; the round trip embed - channel - extract against the
model; and the frame pipeline."""
import functools

import numpy as np
import pytest

import channel_lib as cl
import stepped_lib as st
from test_gpu_parity import _Dev
from testlib import experiments_library, using_library
from svsdct import batch, native
from svsdct.native import Planes
from svsdct.pipeline import FramePipeline

pytestmark = pytest.mark.gpu

PAD = 0xAB
LAYOUTS = [(s, False) for s in st.SHAPES] + [(st.PITCHED, True)]
LAYOUT_IDS = [s + ("_pitched" if p else "") for s, p in LAYOUTS]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    frames = st.content(kind, st.SHAPES[shape])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def payload_of(shape):
    return st.payload_for(st.SHAPES[shape])


@functools.lru_cache(maxsize=None)
def model_of(shape, kind, table, option, rule):
    """-> (stego, bits consumed, the bits the model reads from that stego), computed once and shared"""
    order_key, index, key = st.OPTIONS[option]
    stego, used = st.model_batch_embed(frames_of(shape, kind), st.TABLES[table], payload_of(shape), st.N_AC, rule, index, key,
                                       st.FIRST_FRAME, order_key)
    bits = st.model_batch_extract(stego, st.TABLES[table], st.N_AC, index, key, st.FIRST_FRAME, order_key)
    stego.setflags(write=False)
    bits.setflags(write=False)
    return stego, used, bits


def geometry(frames, pitched):
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    return Planes(f, h, w, 0, row_pitch, frame_pitch)


def view(host, planes):
    return np.lib.stride_tricks.as_strided(host, (planes.n_frames, planes.height, planes.width), (planes.frame_pitch, planes.row_pitch, 1))


def planted(frames, planes, fill=PAD):
    host = np.full(planes.n_frames * planes.frame_pitch, fill, np.uint8)
    view(host, planes)[...] = frames
    return host


def padding_of(host, planes):
    mask = np.ones(host.size, bool)
    view(mask, planes)[...] = False
    return host[mask]


def offset_payload(bits):
    """the payload packed behind BIT_OFFSET bits of ones -> a device buffer"""
    packed = np.packbits(np.concatenate([np.ones(st.BIT_OFFSET, np.uint8), bits]))
    packed = np.concatenate([packed, np.zeros(-packed.size % 4 + 4, np.uint8)])
    d = _Dev(packed.size)
    d.put(packed)
    return d


def call_keywords(option, rule, table=None, delta=None):
    order_key, index, key = st.OPTIONS[option]
    kw = dict(order=batch.block_order(order_key, st.FIRST_FRAME) if order_key is not None else None,
              coeffs=list(index) if index is not None else None, dither_key=key, first_frame=st.FIRST_FRAME)
    if table is not None:
        kw["steps"] = table
    return kw


def rule_keywords(rule):
    return dict(nearest=rule == "nearest", minmove=rule == "minmove")


def device_embed(frames, d_bits, n_bits, delta, pitched=False, in_place=False, **kw):
    """one embed_device call -> (stego frames, bits embedded, the output buffer's padding, the input buffer after the call)"""
    planes = geometry(frames, pitched)
    host = planted(frames, planes)
    d_in = _Dev(host.size)
    d_in.put(host)
    d_out = d_in if in_place else _Dev(host.size)
    if not in_place:
        d_out.put(np.full(host.size, PAD, np.uint8))
    used = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, delta, st.N_AC, d_bits.ptr.value, st.BIT_OFFSET, n_bits,
                              mode="exact", **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    out = d_out.get()
    return view(out, planes).copy(), used, padding_of(out, planes), d_in.get()


def device_extract(frames, delta, pitched=False, **kw):
    planes = geometry(frames, pitched)
    d_in = _Dev(planes.n_frames * planes.frame_pitch)
    d_in.put(planted(frames, planes))
    cap = frames.shape[0] * (frames.shape[1] // 8) * (frames.shape[2] // 8) * st.N_AC
    nbytes = (cap + 7) // 8 + (-((cap + 7) // 8)) % 4 + 4
    d_out = _Dev(nbytes)
    d_out.put(np.full(nbytes, PAD, np.uint8))
    got = batch.extract_device(d_in.ptr.value, planes, delta, st.N_AC, d_out.ptr.value, nbytes, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    out = d_out.get()
    assert (out[(cap + 7) // 8:] == PAD).all(), "the extract wrote past its bits"
    return np.unpackbits(out[: (cap + 7) // 8], count=cap), got


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else f"{len(bad)} of {want.size} differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---- 1. the device against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.CONTENTS)
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_the_device_is_the_model(shape, pitched, kind):
    """every table x {no option, order, non-prefix selection, dither, all three} x three rules: stego bytes, the count, the
    padding, the input, and the bits the stepped extract reads from that stego.  The payload ends inside a block and starts at
    a bit offset that is no multiple of 32."""
    frames = frames_of(shape, kind)
    payload = payload_of(shape)
    d_bits = offset_payload(payload)
    source = planted(frames, geometry(frames, pitched))
    for table in st.TABLES:
        for option in st.OPTIONS:
            for rule in st.RULES:
                want, want_used, want_bits = model_of(shape, kind, table, option, rule)
                kw = call_keywords(option, rule, st.TABLES[table])
                got, used, padding, src = device_embed(frames, d_bits, payload.size, 1.0, pitched, **kw, **rule_keywords(rule))
                where = (shape, pitched, kind, table, option, rule)
                assert used == want_used == payload.size, where
                assert np.array_equal(got, want), (where, first_difference(got, want))
                assert (padding == PAD).all(), (where, "the call wrote into the padding")
                assert np.array_equal(src, source), (where, "the call wrote to its input")
            bits, n = device_extract(np.asarray(want), 1.0, pitched, **call_keywords(option, None, st.TABLES[table]))
            assert n == want_bits.size and np.array_equal(bits, want_bits), (shape, pitched, kind, table, option, first_difference(bits, want_bits))


def test_in_place_is_out_of_place():
    shape, kind = "odd", "full"
    frames, payload = frames_of(shape, kind), payload_of(shape)
    d_bits = offset_payload(payload)
    for table, option, rule in (("m75x2", "all", "minmove"), ("odd", "plain", "reference")):
        want, want_used, _ = model_of(shape, kind, table, option, rule)
        got, used, _, _ = device_embed(frames, d_bits, payload.size, 1.0, in_place=True, **call_keywords(option, rule, st.TABLES[table]),
                                       **rule_keywords(rule))
        assert used == want_used and np.array_equal(got, want), (table, option, rule, first_difference(got, want))


def test_an_empty_payload_copies_and_no_coefficients_round_trip():
    """n_bits = 0: the copy.  A selection-free call at n_ac = 0 with a payload: every block through the transforms, untouched
    coefficients - the reference's bytes for such a call (the existing call's)"""
    frames = frames_of("odd", "full")
    d_bits = offset_payload(np.ones(64, np.uint8))
    got, used, _, _ = device_embed(frames, d_bits, 0, 1.0, steps=st.TABLES["m75x2"])
    assert used == 0 and np.array_equal(got, frames)
    planes = geometry(frames, False)
    d_in, d_a, d_b = _Dev(frames.size), _Dev(frames.size), _Dev(frames.size)
    d_in.put(frames)
    assert batch.embed_device(d_in.ptr.value, d_a.ptr.value, planes, 1.0, 0, d_bits.ptr.value, 0, 40, mode="exact", steps=st.TABLES["m75x2"]) == 0
    assert batch.embed_device(d_in.ptr.value, d_b.ptr.value, planes, 20, 0, d_bits.ptr.value, 0, 40, mode="exact") == 0
    native.check(native.load().svs_stream_synchronize(None), "sync")
    assert np.array_equal(d_a.get(), d_b.get()) and not np.array_equal(d_a.get().reshape(frames.shape), frames)


# ---- 2. uniform tables against the existing calls of the same build ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(st.UNIFORM))
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_a_uniform_table_is_the_existing_call(shape, pitched, name):
    """every delta[k] = D against delta = D: svs_embed_dev(SVS_EXACT_POCKETFFT) / svs_embed_ordered_dev / svs_embed_select_dev /
    svs_embed_dithered_dev and their extracts, byte for byte and bit for bit.  D = 16 is a power of two: the existing call
    multiplies by 1 / D where the stepped side divides."""
    d = st.UNIFORM[name]
    payload = payload_of(shape)
    d_bits = offset_payload(payload)
    for kind in st.CONTENTS:
        frames = frames_of(shape, kind)
        for option in st.OPTIONS:
            for rule in st.RULES:
                where = (shape, pitched, name, kind, option, rule)
                got, used, _, _ = device_embed(frames, d_bits, payload.size, 1.0, pitched, **call_keywords(option, rule, st.TABLES[name]),
                                               **rule_keywords(rule))
                want, want_used, _, _ = device_embed(frames, d_bits, payload.size, d, pitched, **call_keywords(option, rule),
                                                     **rule_keywords(rule))
                assert used == want_used, where
                assert np.array_equal(got, want), (where, first_difference(got, want))
            bits, n = device_extract(got, 1.0, pitched, **call_keywords(option, None, st.TABLES[name]))
            want_bits, want_n = device_extract(got, d, pitched, mode="exact", **call_keywords(option, None))
            assert n == want_n and np.array_equal(bits, want_bits), (shape, pitched, name, kind, option)


# ---- 3. the host forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_kb", [8, 32, 4096])
@pytest.mark.parametrize("option", ["plain", "all"])
def test_the_host_forms_equal_the_device_forms_across_staging_chunks(option, chunk_kb, monkeypatch):
    """with the experiments library's SVS_STAGE_CHUNK_KB, a five-frame clip travels in bands of block rows (8 KB), in groups of
    frames (32 KB) or whole (4 MB); under an order or a dither the chunks are whole frames.  The model is the yardstick."""
    exp = experiments_library()
    monkeypatch.setenv("SVS_STAGE_CHUNK_KB", str(chunk_kb))
    f, h, w = 5, 64, 136
    frames = np.random.default_rng(chunk_kb).integers(0, 256, (f, h, w)).astype(np.uint8)
    payload = st.payload_for((f, h, w))
    order_key, index, key = st.OPTIONS[option]
    table = st.TABLES["m50x3"]
    want, want_used = st.model_batch_embed(frames, table, payload, st.N_AC, "nearest", index, key, st.FIRST_FRAME, order_key)
    want_bits = st.model_batch_extract(want, table, st.N_AC, index, key, st.FIRST_FRAME, order_key)
    kw = dict(block_key=order_key, first_frame=st.FIRST_FRAME, coeffs=list(index) if index else None, dither_key=key, steps=table)
    with using_library(exp):
        stego, used = batch.embed_frames(frames, 1.0, st.N_AC, payload, nearest=True, **kw)
        packed, n = batch.extract_frames(stego, 1.0, st.N_AC, **kw)
    assert used == want_used == payload.size
    assert np.array_equal(stego, want), first_difference(stego, want)
    assert n == want_bits.size and np.array_equal(np.unpackbits(packed, count=n), want_bits)
    d_bits = offset_payload(payload)
    device, dev_used, _, _ = device_embed(frames, d_bits, payload.size, 1.0, nearest=True, **call_keywords(option, "nearest", table))
    assert dev_used == used and np.array_equal(device, stego)


# ---- 4. embed, channel, extract: the numbers of the model ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def survival_clip():
    rng = np.random.default_rng(cl.SURVIVAL_SEED)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    payload = rng.integers(0, 2, (h // 8) * (w // 8) * 10).astype(np.uint8)
    return cover, payload


@pytest.mark.parametrize("index", [st.ROW_1_10, st.ZZ_6_15], ids=["rowmajor", "zigzag6"])
def test_round_trip_through_the_channel_on_the_device(index):
    """svs_stepped_embed_dev -> svs_requantise_dev at quality 75 and 50 -> svs_stepped_extract_dev at (3, 96, 160), one payload
    copy per frame, the table matched to quality 75: the per-copy error counts are the model's, exactly"""
    cover, payload = survival_clip()
    f, h, w = cover.shape
    table = st.matched(75, 2)
    _, want = st.survival(table, index, "reference", qualities=(75, 50))
    planes = Planes.contiguous(f, h, w)
    packed = np.packbits(np.tile(payload, f))
    d_bits = _Dev(packed.size + 8)
    d_bits.put(np.concatenate([packed, np.zeros(8, np.uint8)]))
    d_cover, d_stego, d_out = _Dev(cover.size), _Dev(cover.size), _Dev(packed.size + 8)
    d_cover.put(cover)
    for quality in (75, 50):
        used = batch.embed_device(d_cover.ptr.value, d_stego.ptr.value, planes, 1.0, 10, d_bits.ptr.value, 0, f * payload.size,
                                  coeffs=list(index), steps=table)
        assert used == f * payload.size
        batch.requantise_device(d_stego.ptr.value, d_stego.ptr.value, planes, quality)
        got = batch.extract_device(d_stego.ptr.value, planes, 1.0, 10, d_out.ptr.value, packed.size + 8, coeffs=list(index), steps=table)
        native.check(native.load().svs_stream_synchronize(None), "sync")
        bits = np.unpackbits(d_out.get()[: packed.size], count=got).reshape(f, payload.size)
        errors = [int((b != payload).sum()) for b in bits]
        print(f"quality {quality}: {errors}")
        assert errors == want[quality], (quality, errors, want[quality])


# ---- 5. the frame pipeline -----------------------------------------------------------------------------------------------------
def test_the_pipeline_gives_the_same_round_trip():
    cover, payload = survival_clip()
    f, h, w = cover.shape
    table = st.matched(75, 2)
    index = st.ZZ_6_15
    stream = np.tile(payload, f)
    want = np.stack([st.model_embed(g, table, payload, index=index)[0] for g in cover])
    with FramePipeline(h, w, f, 1.0, 10, depth=2, coeffs=list(index), steps=table) as pipe:
        pipe.set_payload(stream)
        pipe.input(0)[...] = cover
        assert pipe.submit_embed(0, f, 0) == stream.size
        stego = pipe.embed_result(0).copy()
        assert np.array_equal(stego, want), first_difference(stego, want)
        through = cl.model_requantise(stego, cl.channel.quality_steps(50))
        pipe.input(1)[...] = through
        assert pipe.submit_extract(1, f) == stream.size
        packed, n = pipe.extract_result(1)
        bits = np.unpackbits(np.array(packed), count=n).reshape(f, payload.size)
    _, model = st.survival(table, index, "reference", qualities=(50,))
    assert [int((b != payload).sum()) for b in bits] == model[50]
    with pytest.raises(ValueError):
        FramePipeline(h, w, f, 1.0, 10, steps=table, readback=True)
