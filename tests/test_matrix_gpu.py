"""Matrix embedding on the GPU (svs_matrix_embed* / svs_matrix_extract*, include/svsdct.h): the device output against the host build
of the same block bodies (tests/hostemu/matrix_emu.cpp, which tests/test_matrix_cpu.py holds against the NumPy sender and
receiver) byte for byte and bit for bit - no tolerance: both are the pocketfft-identical arithmetic - for both searches, k = 1, 2,
3, 4, 6, three tables, the three rules and a rotated set of order / selection / dither on clipping noise, mid noise and flat
frames; in place and pitched planes, a bit offset of 45 and a payload that ends inside a block; the host forms across staging
chunks; the k = 1 identity against the stepped calls of the same build; the round trip through svs_bit_errors_dev; the extract of
never-embedded frames against the NumPy syndrome of svs_stepped_extract_dev's bits; and the frame pipeline.
(3, 40, 200) has a partial last wave and an odd block row, (3, 48, 272) several workgroups: the smallest shapes at which the
budget edge, the wave-private LDS tile and the packing of k-bit runs across lanes can go wrong."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import matrix_lib as mx
import stepped_lib as st
from test_gpu_parity import _Dev
from testlib import experiments_library, using_library
from svsdct import batch, native
from svsdct.native import Planes
from svsdct.pipeline import FramePipeline

pytestmark = pytest.mark.gpu

PAD = 0xAB
BIT_OFFSET = 45
TABLES = ("u20", "u7", "m75x2")
LAYOUTS = [(s, False) for s in st.SHAPES] + [(st.PITCHED, True)]
LAYOUT_IDS = [s + ("_pitched" if p else "") for s, p in LAYOUTS]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    mx.emu()


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    frames = st.content(kind, st.SHAPES[shape])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def payload_of(shape, k):
    return mx.payload_for(st.SHAPES[shape], k)


def cases():
    """(table, k, rule, search, option): every table x k x rule x search, the option sets rotated over them; search 1 at k = 6 is
    refused (test_matrix_cpu.py), so k = 5 stands in for it there"""
    names = list(mx.OPTIONS)
    out = []
    for i, (table, k, rule, search) in enumerate(itertools.product(TABLES, mx.KS, st.RULES, (0, 1))):
        out.append((table, 5 if search and k == 6 else k, rule, search, names[(i + i // len(names)) % len(names)]))
    return out


@functools.lru_cache(maxsize=None)
def host_of(shape, kind, table, k, rule, search, option):
    """-> (stego, bits consumed, the bits the host build reads from that stego), computed once and shared"""
    order_key, zz, key = mx.OPTIONS[option]
    index = mx.selection(k, zz)
    stego, used = mx.host_batch_embed(frames_of(shape, kind), st.TABLES[table], payload_of(shape, k), k, index, search, rule, key,
                                      mx.FIRST_FRAME, order_key)
    bits = mx.host_batch_extract(stego, st.TABLES[table], k, index, key, mx.FIRST_FRAME, order_key)
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
    """the payload packed behind BIT_OFFSET bits of ones, ones behind it too -> a device buffer"""
    packed = np.packbits(np.concatenate([np.ones(BIT_OFFSET, np.uint8), bits, np.ones(64, np.uint8)]))
    packed = np.concatenate([packed, np.full(-packed.size % 4 + 4, 0xFF, np.uint8)])
    d = _Dev(packed.size)
    d.put(packed)
    return d


def keywords(k, search, option, table):
    order_key, zz, key = mx.OPTIONS[option]
    return dict(order=batch.block_order(order_key, mx.FIRST_FRAME) if order_key is not None else None,
                coeffs=list(mx.selection(k, zz)) if zz else None, dither_key=key, first_frame=mx.FIRST_FRAME, steps=table,
                matrix=(k, "pair") if search else k)


def rule_keywords(rule):
    return dict(nearest=rule == "nearest", minmove=rule == "minmove")


def device_embed(frames, d_bits, n_bits, k, pitched=False, in_place=False, n_ac=None, **kw):
    """one embed_device call -> (stego frames, bits embedded, the output buffer's padding, the input buffer after the call)"""
    planes = geometry(frames, pitched)
    host = planted(frames, planes)
    d_in = _Dev(host.size)
    d_in.put(host)
    d_out = d_in if in_place else _Dev(host.size)
    if not in_place:
        d_out.put(np.full(host.size, PAD, np.uint8))
    used = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, 1.0, mx.slots(k) if n_ac is None else n_ac, d_bits.ptr.value,
                              BIT_OFFSET, n_bits, mode="exact", **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    out = d_out.get()
    return view(out, planes).copy(), used, padding_of(out, planes), d_in.get()


def device_extract(frames, k, bits_per_block, pitched=False, n_ac=None, **kw):
    planes = geometry(frames, pitched)
    d_in = _Dev(planes.n_frames * planes.frame_pitch)
    d_in.put(planted(frames, planes))
    cap = frames.shape[0] * (frames.shape[1] // 8) * (frames.shape[2] // 8) * bits_per_block
    nbytes = (cap + 7) // 8 + (-((cap + 7) // 8)) % 4 + 4
    d_out = _Dev(nbytes)
    d_out.put(np.full(nbytes, PAD, np.uint8))
    got = batch.extract_device(d_in.ptr.value, planes, 1.0, mx.slots(k) if n_ac is None else n_ac, d_out.ptr.value, nbytes, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    out = d_out.get()
    assert (out[(cap + 7) // 8:] == PAD).all(), "the extract wrote past its bits"
    return np.unpackbits(out[: (cap + 7) // 8], count=cap), got


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else f"{len(bad)} of {want.size} differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---- 1. the device against the host build -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.CONTENTS)
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_the_device_is_the_host_build(shape, pitched, kind):
    """stego bytes, the count, the padding, the input, and the bits svs_matrix_extract_dev reads from that stego"""
    frames = frames_of(shape, kind)
    source = planted(frames, geometry(frames, pitched))
    seen = set()
    for table, k, rule, search, option in cases():
        payload = payload_of(shape, k)
        d_bits = offset_payload(payload)
        want, want_used, want_bits = host_of(shape, kind, table, k, rule, search, option)
        kw = keywords(k, search, option, st.TABLES[table])
        got, used, padding, src = device_embed(frames, d_bits, payload.size, k, pitched, **kw, **rule_keywords(rule))
        where = (shape, pitched, kind, table, k, rule, search, option)
        assert used == want_used == payload.size, where
        assert np.array_equal(got, want), (where, first_difference(got, want))
        assert (padding == PAD).all(), (where, "the call wrote into the padding")
        assert np.array_equal(src, source), (where, "the call wrote to its input")
        bits, n = device_extract(np.asarray(want), k, k, pitched, **kw)
        assert n == want_bits.size == mx.capacity(frames.shape, k), where
        assert np.array_equal(bits, want_bits), (where, first_difference(bits, want_bits))
        seen.add((option, search))
    assert seen == set(itertools.product(mx.OPTIONS, (0, 1)))


def test_in_place_is_out_of_place():
    shape, kind = "odd", "full"
    frames = frames_of(shape, kind)
    for table, k, rule, search, option in (("m75x2", 4, "minmove", 1, "all"), ("u7", 6, "reference", 0, "plain"), ("u20", 3, "nearest", 1, "order")):
        payload = payload_of(shape, k)
        want, want_used, _ = host_of(shape, kind, table, k, rule, search, option)
        got, used, _, _ = device_embed(frames, offset_payload(payload), payload.size, k, in_place=True,
                                       **keywords(k, search, option, st.TABLES[table]), **rule_keywords(rule))
        assert used == want_used and np.array_equal(got, want), (table, k, rule, search, option, first_difference(got, want))


def test_an_empty_payload_copies_and_a_full_one_fills_the_capacity():
    frames = frames_of("odd", "mid")
    k, table = 3, st.TABLES["u20"]
    d_bits = offset_payload(np.ones(64, np.uint8))
    got, used, _, _ = device_embed(frames, d_bits, 0, k, steps=table, matrix=k)
    assert used == 0 and np.array_equal(got, frames)
    cap = mx.capacity(frames.shape, k)
    full = np.random.default_rng(9).integers(0, 2, cap + 40).astype(np.uint8)
    got, used, _, _ = device_embed(frames, offset_payload(full), full.size, k, steps=table, matrix=(k, "pair"), minmove=True)
    want, want_used = mx.host_batch_embed(frames, table, full, k, mx.selection(k, False), 1, "minmove")
    assert used == want_used == cap and np.array_equal(got, want)


# ---- 2. the host forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_kb", [8, 32, 4096])
@pytest.mark.parametrize("option", ["plain", "all"])
def test_the_host_forms_equal_the_device_forms_across_staging_chunks(option, chunk_kb, monkeypatch):
    """with the experiments library's SVS_STAGE_CHUNK_KB a five-frame clip travels in several chunks; a matrix call stages whole
    frames, as the keyed calls do.  The host build is the yardstick."""
    exp = experiments_library()
    monkeypatch.setenv("SVS_STAGE_CHUNK_KB", str(chunk_kb))
    f, h, w = 5, 64, 136
    k, search, rule = 4, 1, "minmove"
    frames = np.random.default_rng(chunk_kb).integers(0, 256, (f, h, w)).astype(np.uint8)
    payload = mx.payload_for((f, h, w), k)
    order_key, zz, key = mx.OPTIONS[option]
    index = mx.selection(k, zz)
    table = st.TABLES["m75x2"]
    want, want_used = mx.host_batch_embed(frames, table, payload, k, index, search, rule, key, mx.FIRST_FRAME, order_key)
    want_bits = mx.host_batch_extract(want, table, k, index, key, mx.FIRST_FRAME, order_key)
    kw = dict(block_key=order_key, first_frame=mx.FIRST_FRAME, coeffs=list(index) if zz else None, dither_key=key, steps=table,
              matrix=(k, "pair"))
    with using_library(exp):
        stego, used = batch.embed_frames(frames, 1.0, mx.slots(k), payload, minmove=True, **kw)
        packed, n = batch.extract_frames(stego, 1.0, mx.slots(k), **kw)
    assert used == want_used == payload.size
    assert np.array_equal(stego, want), first_difference(stego, want)
    assert n == want_bits.size and np.array_equal(np.unpackbits(packed, count=n), want_bits)


# ---- 3. the k = 1 identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(st.UNIFORM))
def test_k_1_is_the_stepped_call_of_the_same_build(name):
    """svs_matrix_embed_dev at k = 1 against svs_stepped_embed_dev with the same one-coefficient selection, table, order, dither
    and rule, both searches; svs_matrix_extract_dev against svs_stepped_extract_dev.  D = 20, 16 and 7."""
    table = st.TABLES[name]
    for shape, kind in (("odd", "full"), ("even", "mid"), ("one_block", "flat")):
        frames = frames_of(shape, kind)
        payload = payload_of(shape, 1)
        d_bits = offset_payload(payload)
        for option, rule, coeff in itertools.product(("plain", "all"), st.RULES, (1, 9, 63)):
            order_key, _, key = mx.OPTIONS[option]
            common = dict(order=batch.block_order(order_key, mx.FIRST_FRAME) if order_key is not None else None, coeffs=[coeff],
                          dither_key=key, first_frame=mx.FIRST_FRAME, steps=table)
            want, want_used, _, _ = device_embed(frames, d_bits, payload.size, 1, **common, **rule_keywords(rule))
            where = (name, shape, kind, option, rule, coeff)
            for search in (0, 1):
                got, used, _, _ = device_embed(frames, d_bits, payload.size, 1, **common, **rule_keywords(rule),
                                               matrix=(1, "pair") if search else 1)
                assert used == want_used == payload.size, where
                assert np.array_equal(got, want), (where, search, first_difference(got, want))
            bits, n = device_extract(want, 1, 1, **common, matrix=1)
            want_bits, want_n = device_extract(want, 1, 1, **common)
            assert n == want_n and np.array_equal(bits, want_bits), where


# ---- 4. the round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,search", [(2, 0), (3, 1), (4, 1), (5, 1), (6, 0)])
def test_the_round_trip_has_no_bit_errors_on_mid_content(k, search):
    """svs_matrix_embed_dev -> svs_matrix_extract_dev -> svs_bit_errors_dev against the payload, on noise in [64, 192) under
    SVS_MINMOVE and the other rules: 0"""
    lib = native.load()
    frames = frames_of("even", "mid")
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    cap = mx.capacity(frames.shape, k)
    payload = np.random.default_rng(k).integers(0, 2, cap).astype(np.uint8)
    packed = np.packbits(payload)
    nbytes = packed.size + (-packed.size) % 4 + 4
    d_bits, d_out, d_in, d_stego, d_count = _Dev(nbytes), _Dev(nbytes), _Dev(frames.size), _Dev(frames.size), _Dev(8)
    d_bits.put(np.concatenate([packed, np.zeros(nbytes - packed.size, np.uint8)]))
    d_in.put(frames)
    for rule, option in itertools.product(st.RULES, ("plain", "all")):
        kw = keywords(k, search, option, st.TABLES["u20"])
        used = batch.embed_device(d_in.ptr.value, d_stego.ptr.value, planes, 1.0, mx.slots(k), d_bits.ptr.value, 0, cap, **kw,
                                  **rule_keywords(rule))
        got = batch.extract_device(d_stego.ptr.value, planes, 1.0, mx.slots(k), d_out.ptr.value, nbytes, **kw)
        assert used == got == cap
        d_count.put(np.zeros(8, np.uint8))
        native.check(lib.svs_bit_errors_dev(d_out.ptr, d_bits.ptr, cap, d_count.ptr, None), "svs_bit_errors_dev")
        native.check(lib.svs_stream_synchronize(None), "sync")
        assert int(d_count.get().view(np.uint64)[0]) == 0, (k, search, rule, option)


# ---- 5. the extract alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_the_extract_of_never_embedded_frames_is_the_syndrome_of_the_stepped_extracts_bits(shape, pitched):
    """the fold and the packing of k-bit runs, independently of the embed: svs_matrix_extract_dev against the NumPy syndrome of
    the n parities svs_stepped_extract_dev reads from the same frames"""
    for kind in ("full", "flat"):
        frames = frames_of(shape, kind)
        for i, (k, table) in enumerate(itertools.product(mx.KS + (5,), ("u20", "m75x2"))):
            option = list(mx.OPTIONS)[i % len(mx.OPTIONS)]
            kw = keywords(k, 0, option, st.TABLES[table])
            bits, n = device_extract(frames, k, k, pitched, **kw)
            kw.pop("matrix")
            parity, m = device_extract(frames, k, mx.slots(k), pitched, **kw)
            assert m == mx.capacity(frames.shape, mx.slots(k)) and n == mx.capacity(frames.shape, k)
            want = mx.bits_of(mx.syndrome(parity.reshape(-1, mx.slots(k))), k)
            assert np.array_equal(bits, want), (shape, pitched, kind, k, table, option, first_difference(bits, want))


# ---- 6. the frame pipeline -----------------------------------------------------------------------------------------------------
def test_the_pipeline_gives_the_host_builds_round_trip():
    frames = frames_of("even", "mid")
    f, h, w = frames.shape
    k, table, index = 3, st.TABLES["u20"], mx.zigzag(3)
    cap = mx.capacity(frames.shape, k)
    stream = np.random.default_rng(21).integers(0, 2, cap - 5).astype(np.uint8)
    want, want_used = mx.host_batch_embed(frames, table, stream, k, index, 1, "minmove")
    with FramePipeline(h, w, f, 1.0, mx.slots(k), depth=2, coeffs=list(index), steps=table, matrix=(k, "pair"), minmove=True) as pipe:
        assert pipe.frame_capacity * f == cap
        pipe.set_payload(stream)
        pipe.input(0)[...] = frames
        assert pipe.submit_embed(0, f, 0) == stream.size == want_used
        stego = pipe.embed_result(0).copy()
        assert np.array_equal(stego, want), first_difference(stego, want)
        pipe.input(1)[...] = stego
        assert pipe.submit_extract(1, f) == cap
        packed, n = pipe.extract_result(1)
        bits = np.unpackbits(np.array(packed), count=n)
    assert np.array_equal(bits[:stream.size], stream)
