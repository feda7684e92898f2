"""Keyed dither modulation on the GPU (svs_embed_dithered* / svs_extract_dithered*, include/svsdct.h): the device and the
host-pointer calls against the NumPy model of tests/dither_lib.py for stego bytes, counts and bits, on the smallest shapes at
which the kernels' block -> (frame, block index) arithmetic can go wrong, and the identities that catch a (t, i) that depends
on the launch."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dither_lib as dl
from test_gpu_parity import _Dev
from svsdct import batch, coeffs, native, pipeline
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

KEY = 0x0123456789ABCDEF
ORDER_KEY = 0xC0FFEE1234
# one block; two small frames; the budget ends inside frame 1; three workgroups of 256 blocks with a ragged tail of 88 and waves
# that straddle frames (120 blocks per frame); row_pitch > width and a padded frame_pitch
SHAPES = {"one_block": (1, 8, 8), "two_frames": (2, 16, 24), "budget_in_frame_1": (3, 24, 40), "three_workgroups": (5, 64, 120),
          "pitched": (2, 16, 24)}
DELTAS = (8, 20, 12.5, 0.1)          # QM_POW2, QM_F32, a non-power-of-two float32, QM_DOUBLE
N_ACS = (3, 10, 63)


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def bits_of(packed, n):
    return np.unpackbits(np.asarray(packed), count=n)


def cover(f, h, w, seed=1):
    frames = dl.noise((f, h, w), 0, 256, seed=seed)       # clips too: the model clips as the kernels do
    frames[0, :8, :8] = 128                              # a flat block
    return frames


def budget(shape, f, h, w, n):
    per_frame = (h // 8) * (w // 8) * n
    if shape == "budget_in_frame_1":
        return per_frame + per_frame // 2 + 1             # inside frame 1, and (n > 1) inside a block
    return f * per_frame - (n // 2 + 1 if f * per_frame > n else 0)   # the last block takes only part of its bits


def _flags(rule, mode=None):
    return batch.embed_flags(mode, rule == "nearest", rule == "minmove")


def device_roundtrip(frames, delta, n, stream, bit_offset, n_bits, rule, first, pitched, index=None, order_key=None):
    """svs_embed_dithered_dev in place and svs_extract_dithered_dev, on tight or pitched planes with sentinels in the padding
    -> (stego, bits embedded, extracted 0/1 bits)"""
    lib = native.load()
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    view = lambda a: np.lib.stride_tricks.as_strided(a, (f, h, w), (frame_pitch, row_pitch, 1))   # noqa: E731
    view(host)[...] = frames
    pad = np.ones(host.size, bool)
    view(pad)[...] = False
    d = _Dev(host.size)
    d.put(host)
    packed = batch.pack_bits(stream)
    d_bits = _Dev(packed.size)
    d_bits.put(packed)
    count = n if index is None else len(index)
    cap = batch.capacity_bits(f, h, w, count)
    nbytes = max(1, (cap + 7) // 8)
    d_out = _Dev(nbytes + 8)
    d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
    dith = native.Dither(KEY, first, 0)
    order = batch.block_order(order_key, first)
    sel = None if index is None else native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    done, got = C.c_uint64(0), C.c_uint64(0)
    native.check(lib.svs_embed_dithered_dev(d.ptr, d.ptr, C.byref(planes), ref(order), ref(sel), C.byref(dith), float(delta), n,
                                            d_bits.ptr, bit_offset, n_bits, _flags(rule), C.byref(done), None),
                 "svs_embed_dithered_dev")
    native.check(lib.svs_extract_dithered_dev(d.ptr, C.byref(planes), ref(order), ref(sel), C.byref(dith), float(delta), n,
                                              d_out.ptr, nbytes, batch.mode_flags(None), C.byref(got), None),
                 "svs_extract_dithered_dev")
    native.check(lib.svs_stream_synchronize(None), "svs_stream_synchronize")
    out, res = d.get(), d_out.get()
    assert (out[pad] == 0xAB).all() and (res[nbytes:] == 0x5A).all() and got.value == cap
    return view(out).copy(), int(done.value), bits_of(res[:nbytes], cap)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_and_host_calls_against_the_model(shape):
    f, h, w = SHAPES[shape]
    frames = cover(f, h, w)
    for j, (rule, n, delta) in enumerate(itertools.product(dl.RULES, N_ACS, DELTAS)):
        first = (0, 5)[j % 2]
        offset = (0, 37)[(j // 2) % 2]
        n_bits = budget(shape, f, h, w, n)
        stream = dl.payload(offset + n_bits, seed=j)
        want, want_used = dl.model_batch_embed(frames, delta, stream[offset:], n, rule, key=KEY, first_frame=first)
        want_bits = dl.model_batch_extract(want, delta, n, key=KEY, first_frame=first)
        what = (shape, rule, n, delta, first)
        assert want_used == n_bits
        stego, used = batch.embed_frames(frames, delta, n, stream, bit_offset=offset, dither_key=KEY, first_frame=first,
                                         nearest=rule == "nearest", minmove=rule == "minmove")
        assert used == n_bits and np.array_equal(stego, want), (what, np.argwhere(stego != want)[:4])
        packed, got = batch.extract_frames(stego, delta, n, dither_key=KEY, first_frame=first)
        assert got == want_bits.size and np.array_equal(bits_of(packed, got), want_bits), what
        stego, used, bits = device_roundtrip(frames, delta, n, stream, offset, n_bits, rule, first, shape == "pitched")
        assert used == n_bits and np.array_equal(stego, want), (what, np.argwhere(stego != want)[:4])
        assert np.array_equal(bits, want_bits), what


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_selection_with_the_dither(shape):
    """a coefficient selection (n_ac is ignored, the count rules), alone and under a keyed order, host and device calls"""
    f, h, w = SHAPES[shape]
    frames = cover(f, h, w, seed=3)
    zigzag6 = [int(k) for k in coeffs.selection("zigzag:6", 3)]
    for rule, index, delta, first, order_key in (("reference", zigzag6, 20, 5, None), ("nearest", [63, 1, 9, 62, 8], 12.5, 0, None),
                                                 ("minmove", zigzag6, 8, 0, ORDER_KEY), ("reference", [17], 0.1, 5, ORDER_KEY)):
        n = len(index)
        n_bits = budget(shape, f, h, w, n)
        stream = dl.payload(n_bits, seed=n)
        want, want_used = dl.model_batch_embed(frames, delta, stream, n, rule, index=index, key=KEY, first_frame=first,
                                               order_key=order_key)
        want_bits = dl.model_batch_extract(want, delta, n, index=index, key=KEY, first_frame=first, order_key=order_key)
        assert want_used == n_bits
        what = (shape, rule, index, delta, first, order_key)
        stego, used = batch.embed_frames(frames, delta, n, stream, dither_key=KEY, first_frame=first, coeffs=index,
                                         block_key=order_key, nearest=rule == "nearest", minmove=rule == "minmove")
        assert used == n_bits and np.array_equal(stego, want), (what, np.argwhere(stego != want)[:4])
        packed, got = batch.extract_frames(stego, delta, n, dither_key=KEY, first_frame=first, coeffs=index, block_key=order_key)
        assert got == want_bits.size and np.array_equal(bits_of(packed, got), want_bits), what
        stego, used, bits = device_roundtrip(frames, delta, 40, stream, 0, n_bits, rule, first, shape == "pitched", index=index,
                                             order_key=order_key)
        assert used == n_bits and np.array_equal(stego, want), (what, np.argwhere(stego != want)[:4])
        assert np.array_equal(bits, want_bits), what


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_keyed_order_with_the_dither(shape):
    f, h, w = SHAPES[shape]
    frames = cover(f, h, w, seed=2)
    for rule, n, first in (("reference", 10, 5), ("nearest", 3, 0), ("minmove", 63, 5)):
        n_bits = budget(shape, f, h, w, n)
        stream = dl.payload(n_bits, seed=n)
        want, want_used = dl.model_batch_embed(frames, 20, stream, n, rule, key=KEY, first_frame=first, order_key=ORDER_KEY)
        want_bits = dl.model_batch_extract(want, 20, n, key=KEY, first_frame=first, order_key=ORDER_KEY)
        assert want_used == n_bits
        what = (shape, rule, n, first)
        stego, used = batch.embed_frames(frames, 20, n, stream, dither_key=KEY, first_frame=first, block_key=ORDER_KEY,
                                         nearest=rule == "nearest", minmove=rule == "minmove", mode="fast")
        assert used == n_bits and np.array_equal(stego, want), (what, np.argwhere(stego != want)[:4])
        packed, got = batch.extract_frames(stego, 20, n, dither_key=KEY, first_frame=first, block_key=ORDER_KEY, mode="exact")
        assert np.array_equal(bits_of(packed, got), want_bits), what
        stego, used, bits = device_roundtrip(frames, 20, n, stream, 0, n_bits, rule, first, shape == "pitched", None, ORDER_KEY)
        assert used == n_bits and np.array_equal(stego, want) and np.array_equal(bits, want_bits), what


def test_splitting_a_call_changes_nothing():
    """frames [0, F) in one call == [0, a) and [a, F) with first_frame = a and the matching bit_offset: (t, i) must not depend
    on the launch"""
    f, h, w = SHAPES["three_workgroups"]
    frames = cover(f, h, w, seed=3)
    for n, a, order_key in ((10, 2, None), (3, 1, ORDER_KEY), (63, 4, None)):
        per_frame = batch.capacity_bits(1, h, w, n)
        stream = dl.payload(f * per_frame - 5, seed=n)
        whole, used = batch.embed_frames(frames, 20, n, stream, dither_key=KEY, first_frame=7, block_key=order_key)
        head, used_a = batch.embed_frames(frames[:a], 20, n, stream, dither_key=KEY, first_frame=7, block_key=order_key)
        tail, used_b = batch.embed_frames(frames[a:], 20, n, stream, bit_offset=a * per_frame, dither_key=KEY, first_frame=7 + a,
                                          block_key=order_key)
        assert used == used_a + used_b == stream.size
        assert np.array_equal(whole[:a], head) and np.array_equal(whole[a:], tail)
        assert np.array_equal(whole, dl.model_batch_embed(frames, 20, stream, n, key=KEY, first_frame=7, order_key=order_key)[0])
        packed, got = batch.extract_frames(whole, 20, n, dither_key=KEY, first_frame=7, block_key=order_key)
        pa, ga = batch.extract_frames(whole[:a], 20, n, dither_key=KEY, first_frame=7, block_key=order_key)
        pb, gb = batch.extract_frames(whole[a:], 20, n, dither_key=KEY, first_frame=7 + a, block_key=order_key)
        assert np.array_equal(bits_of(packed, got), np.concatenate([bits_of(pa, ga), bits_of(pb, gb)]))
        assert np.array_equal(bits_of(packed, got), dl.model_batch_extract(whole, 20, n, key=KEY, first_frame=7, order_key=order_key))


def test_in_place_equals_out_of_place():
    f, h, w = SHAPES["budget_in_frame_1"]
    frames = cover(f, h, w, seed=4)
    n_bits = budget("budget_in_frame_1", f, h, w, 10)
    stream = dl.payload(n_bits)
    in_place, used, _ = device_roundtrip(frames, 20, 10, stream, 0, n_bits, "reference", 5, False)
    d_src, d_dst, d_bits = _Dev(frames.size), _Dev(frames.size), _Dev(batch.pack_bits(stream).size)
    d_src.put(frames)
    d_dst.put(np.zeros(frames.size, np.uint8))
    d_bits.put(batch.pack_bits(stream))
    tight = Planes.contiguous(f, h, w)
    assert batch.embed_device(d_src.ptr.value, d_dst.ptr.value, tight, 20, 10, d_bits.ptr.value, 0, n_bits, dither_key=KEY,
                              first_frame=5) == n_bits == used
    native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
    assert np.array_equal(d_dst.get().reshape(f, h, w), in_place) and np.array_equal(d_src.get().reshape(f, h, w), frames)
    assert np.array_equal(in_place[2], frames[2])         # the frame past the budget: the cover's bytes


def test_dithered_extraction_of_a_stego_without_a_dither():
    f, h, w = SHAPES["two_frames"]
    frames = cover(f, h, w, seed=5)
    plain, _ = batch.embed_frames(frames, 20, 10, dl.payload(batch.capacity_bits(f, h, w, 10)))
    for src in (plain, frames):
        packed, got = batch.extract_frames(src, 20, 10, dither_key=KEY, first_frame=5)
        assert np.array_equal(bits_of(packed, got), dl.model_batch_extract(src, 20, 10, key=KEY, first_frame=5))


def test_pass_through_routes_give_the_bytes_of_the_call_without_a_dither():
    f, h, w = SHAPES["two_frames"]
    frames = cover(f, h, w, seed=6)
    bits = dl.payload(40)
    for delta, n, b in ((0, 10, bits), (-2.0, 10, bits), (20, 0, bits), (20, 10, bits[:0])):
        plain, used_plain = batch.embed_frames(frames, delta, n, b)
        dithered, used = batch.embed_frames(frames, delta, n, b, dither_key=KEY, first_frame=5)
        assert used == used_plain == 0 and np.array_equal(dithered, plain), (delta, n, b.size)
    packed, got = batch.extract_frames(frames, 0, 10, dither_key=KEY)
    assert got == batch.capacity_bits(f, h, w, 10) and not np.asarray(packed).any()
    assert batch.extract_frames(frames, 20, 0, dither_key=KEY)[1] == 0


def test_pipeline_over_two_submits_equals_the_one_shot_call():
    f, h, w = 4, 24, 40
    frames = cover(f, h, w, seed=7)
    n = 10
    per_frame = batch.capacity_bits(1, h, w, n)
    stream = dl.payload(f * per_frame - 3)
    want, used = batch.embed_frames(frames, 20, n, stream, dither_key=KEY, first_frame=0, block_key=ORDER_KEY)
    assert np.array_equal(want, dl.model_batch_embed(frames, 20, stream, n, key=KEY, order_key=ORDER_KEY)[0])
    with pipeline.FramePipeline(h, w, 2, 20, n, depth=2, dither_key=KEY, block_key=ORDER_KEY) as pipe:
        pipe.set_payload(stream)
        for k in range(2):
            pipe.input(k)[:] = frames[2 * k:2 * k + 2]
            pipe.submit_embed(k, 2, bit_offset=2 * k * per_frame, first_frame=2 * k)
        stego = np.concatenate([pipe.embed_result(k).copy() for k in range(2)])
        assert np.array_equal(stego, want)
        pieces = []
        for k in range(2):
            pipe.input(k)[:] = stego[2 * k:2 * k + 2]
            pipe.submit_extract(k, 2, first_frame=2 * k)
        for k in range(2):
            packed, got = pipe.extract_result(k)
            pieces.append(bits_of(packed.copy(), got))
    assert np.array_equal(np.concatenate(pieces), dl.model_batch_extract(want, 20, n, key=KEY, order_key=ORDER_KEY))
