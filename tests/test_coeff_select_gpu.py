"""Payload coefficient selection on the GPU (include/svsdct.h svs_coeffs): every entry point against the restatement of
tests/coeff_select_lib.py - oracle.frame_embed / frame_extract_bits with the coefficient lookup changed - for stego pixels,
counts and the bits extracted from stego and from cover."""
import ctypes as C

import numpy as np
import pytest

import coeff_select_lib as cs
import kernel_matrix as km
from oracle import qim_dct_oracle as orc
from test_gpu_parity import _Dev
from svsdct import batch, coeffs, native, order, pipeline, synth
from svsdct.native import Planes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def cover(f, h, w, seed):
    """synthetic content with flat, clipping and ramp blocks"""
    frames = synth.synthetic_frames(f, h, w, seed=seed, lo=0, span=256)
    frames[:, :16, :24] = 128
    frames[:, 8:16, 24:40] = 0
    frames[:, -8:, -16:] = 255
    frames[:, 16:24, :] = np.arange(w, dtype=np.uint8)[None, None, :] * 3
    return frames


def bits_of(packed, n):
    return np.unpackbits(np.asarray(packed), count=n)


def budget(f, h, w, count):
    """ends inside the last frame and (count > 1) inside a block"""
    cap = batch.capacity_bits(f, h, w, count)
    n = cap - (cap // f) // 3 - 1
    if count > 1 and n % count == 0:
        n -= 1
    assert cap * (f - 1) // f < n < cap and (count == 1 or n % count)
    return cap, n


@pytest.mark.parametrize("shape", sorted(km.SHAPES))
@pytest.mark.parametrize("kind,count", [("zigzag", 10), ("scattered", 33), ("reversed", 3)])
def test_device_and_host_calls_against_the_restatement(shape, kind, count):
    lib = native.load()
    f, h, w = km.SHAPES[shape]
    delta, index = 8, cs.KINDS[kind](count)
    sel = coeffs.native_coeffs(index)
    frames = cover(f, h, w, seed=count)
    cap, n_bits = budget(f, h, w, count)
    stream = synth.synthetic_bits(km.BIT_OFFSET + n_bits, seed=50 + count)
    want, want_used = cs.select_batch_embed(frames, delta, stream[km.BIT_OFFSET:], index)
    want_bits = cs.select_batch_extract(want, delta, index)
    cover_bits = cs.select_batch_extract(frames, delta, index)
    assert want_used == n_bits

    # host calls (the shared staging loops)
    stego, used = batch.embed_frames(frames, delta, count, stream, bit_offset=km.BIT_OFFSET, coeffs=index)
    assert used == n_bits and np.array_equal(stego, want), np.argwhere(stego != want)[:4]
    for src, ref in ((stego, want_bits), (frames, cover_bits)):
        packed, n = batch.extract_frames(src, delta, count, coeffs=index)
        assert n == cap and np.array_equal(bits_of(packed, n), ref)

    # device calls on pitched planes, in place, sentinel bytes in the padding and behind the packed bits
    row_pitch, frame_pitch = w + 24, (w + 24) * h + 64
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    np.lib.stride_tricks.as_strided(host, (f, h, w), (frame_pitch, row_pitch, 1))[...] = frames
    pad = np.ones(host.size, bool)
    np.lib.stride_tricks.as_strided(pad, (f, h, w), (frame_pitch, row_pitch, 1))[...] = False
    d = _Dev(host.size)
    d.put(host)
    packed = batch.pack_bits(stream)
    d_bits = _Dev(packed.size)
    d_bits.put(packed)
    nbytes = (cap + 7) // 8
    d_out = _Dev(nbytes + 8)
    got = C.c_uint64(0)
    for src_bits in (cover_bits, want_bits):            # extract from the cover, embed in place, extract from the stego
        d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
        native.check(lib.svs_extract_select_dev(d.ptr, C.byref(planes), None, C.byref(sel), float(delta), d_out.ptr, nbytes,
                                                batch.mode_flags(None), C.byref(got), None), "svs_extract_select_dev")
        res = d_out.get()
        assert got.value == cap and np.array_equal(bits_of(res[:nbytes], cap), src_bits)
        assert (res[nbytes:] == 0x5A).all()
        if src_bits is cover_bits:
            done = C.c_uint64(0)
            native.check(lib.svs_embed_select_dev(d.ptr, d.ptr, C.byref(planes), None, C.byref(sel), float(delta), d_bits.ptr,
                                                  km.BIT_OFFSET, n_bits, batch.mode_flags(None), C.byref(done), None),
                         "svs_embed_select_dev")
            out = d.get()
            assert done.value == n_bits
            assert np.array_equal(np.lib.stride_tricks.as_strided(out, (f, h, w), (frame_pitch, row_pitch, 1)), want)
            assert (out[pad] == 0xAB).all()
    # out of place through the Python device form
    d_src = _Dev(frames.size)
    d_src.put(frames)
    d_dst = _Dev(frames.size)
    d_dst.put(np.zeros(frames.size, np.uint8))
    tight = Planes.contiguous(f, h, w)
    assert batch.embed_device(d_src.ptr.value, d_dst.ptr.value, tight, delta, count, d_bits.ptr.value, km.BIT_OFFSET, n_bits,
                              coeffs=index) == n_bits
    assert np.array_equal(d_dst.get().reshape(f, h, w), want) and np.array_equal(d_src.get().reshape(f, h, w), frames)
    assert batch.extract_device(d_dst.ptr.value, tight, delta, count, d_out.ptr.value, nbytes, coeffs=index) == cap
    assert np.array_equal(bits_of(d_out.get()[:nbytes], cap), want_bits)


@pytest.mark.parametrize("delta", cs.DELTAS)
@pytest.mark.parametrize("count", (1, 10, 32, 33, 63))
def test_quantiser_classes_counts_and_nearest(delta, count):
    f, h, w = 2, 40, 72
    frames = cover(f, h, w, seed=3 * count)
    cap, n_bits = budget(f, h, w, count)
    payload = synth.synthetic_bits(n_bits, seed=count)
    for index in ((cs.zigzag(count, 2) if count < 63 else cs.zigzag(63)), cs.scattered(count)):
        for nearest in (False, True):
            want, want_used = cs.select_batch_embed(frames, delta, payload, index, nearest)
            stego, used = batch.embed_frames(frames, delta, count, payload, coeffs=index, nearest=nearest, mode="fast")
            assert used == want_used == n_bits
            assert np.array_equal(stego, want), (delta, count, nearest, np.argwhere(stego != want)[:4])
        packed, n = batch.extract_frames(stego, delta, count, coeffs=index, mode="exact")
        assert n == cap and np.array_equal(bits_of(packed, n), cs.select_batch_extract(stego, delta, index))
        packed, n = batch.extract_frames(frames, delta, count, coeffs=index)
        assert np.array_equal(bits_of(packed, n), cs.select_batch_extract(frames, delta, index))


@pytest.mark.parametrize("count", (3, 10, 40))
def test_keyed_order_with_a_selection(count):
    """the keyed operator is the operator on block-permuted frames (svsdct/order.py), selection included"""
    f, h, w = km.SHAPES["odd"]
    delta, index = 20, cs.zigzag(count, 3)
    key, first = km.KEY, km.FIRST_FRAME
    frames = cover(f, h, w, seed=count)
    cap, n_bits = budget(f, h, w, count)
    payload = synth.synthetic_bits(n_bits, seed=7)
    for nearest in (False, True):
        permuted, want_used = cs.select_batch_embed(order.permute_blocks(frames, key, first), delta, payload, index, nearest)
        want = order.unpermute_blocks(permuted, key, first)
        stego, used = batch.embed_frames(frames, delta, count, payload, coeffs=index, block_key=key, first_frame=first,
                                         nearest=nearest)
        assert used == want_used == n_bits and np.array_equal(stego, want)
    for src in (stego, frames):
        packed, n = batch.extract_frames(src, delta, count, coeffs=index, block_key=key, first_frame=first)
        assert n == cap
        assert np.array_equal(bits_of(packed, n), cs.select_batch_extract(order.permute_blocks(src, key, first), delta, index))


def test_routes_without_coefficients():
    f, h, w = 2, 40, 72
    frames = cover(f, h, w, seed=1)
    payload = synth.synthetic_bits(500, seed=2)
    index = cs.zigzag(5)
    for delta, idx, n_ac in ((0, index, 5), (-2.5, index, 5), (8, [], 0)):
        want, _ = cs.select_batch_embed(frames, delta, payload, idx)
        stego, used = batch.embed_frames(frames, delta, n_ac, payload, coeffs=idx)
        assert used == 0 and np.array_equal(stego, want)
        assert np.array_equal(stego, orc.batch_embed(frames, delta, payload, n_ac)[0])     # the route n_ac = 0 takes today
        plain, _ = batch.embed_frames(frames, delta, n_ac, payload)
        assert np.array_equal(stego, plain)
        packed, n = batch.extract_frames(frames, delta, n_ac, coeffs=idx)
        assert n == batch.capacity_bits(f, h, w, n_ac) and not bits_of(packed, n).any()
    stego, used = batch.embed_frames(frames, 8, 5, np.zeros(0, np.uint8), coeffs=index)   # an empty payload: a copy
    assert used == 0 and np.array_equal(stego, frames)


@pytest.mark.parametrize("n", (1, 3, 10, 15, 20, 63))
def test_prefix_selection_is_the_plain_call_in_every_mode(n):
    f, h, w = km.SHAPES["even"]
    frames = cover(f, h, w, seed=n)
    cap, n_bits = budget(f, h, w, n)
    payload = synth.synthetic_bits(n_bits, seed=n)
    for delta in (8, 7.3):
        for mode in ("fast", "guarded", "exact"):
            plain, used = batch.embed_frames(frames, delta, n, payload, mode=mode)
            for spec in (cs.prefix(n), "rowmajor"):
                stego, got = batch.embed_frames(frames, delta, n, payload, mode=mode, coeffs=spec)
                assert got == used == n_bits and np.array_equal(stego, plain), (n, delta, mode)
            p0, n0 = batch.extract_frames(plain, delta, n, mode=mode)
            p1, n1 = batch.extract_frames(plain, delta, n, mode=mode, coeffs=cs.prefix(n))
            assert n0 == n1 == cap and np.array_equal(p0, p1)


@pytest.mark.parametrize("delta", cs.DELTAS)
def test_gather_identity_on_an_ordinary_stego(delta):
    f, h, w = km.SHAPES["odd"]
    frames = cover(f, h, w, seed=11)
    stego, _ = batch.embed_frames(frames, delta, 10, synth.synthetic_bits(batch.capacity_bits(f, h, w, 10), seed=4))
    packed, n = batch.extract_frames(stego, delta, 63, mode="exact")
    all63 = bits_of(packed, n)
    assert np.array_equal(all63, orc.batch_extract_bits(stego, delta, 63))
    for index in (cs.zigzag(10), cs.zigzag(63), cs.scattered(33), cs.reversed_list(7), cs.zigzag(3, 6)):
        packed, n = batch.extract_frames(stego, delta, len(index), coeffs=index)
        assert np.array_equal(bits_of(packed, n), coeffs.gather(all63, index)), index


def test_frame_pipeline_with_a_selection_equals_one_shot_calls():
    f, h, w, count, delta = 5, 40, 72, 10, 8
    frames = cover(f, h, w, seed=21)
    per = batch.capacity_bits(1, h, w, count)
    payload = synth.synthetic_bits(4 * per + 37, seed=22)
    want, used = batch.embed_frames(frames, delta, count, payload, coeffs="zigzag", nearest=True, block_key=9)
    assert np.array_equal(want, order.unpermute_blocks(cs.select_batch_embed(order.permute_blocks(frames, 9), delta, payload,
                                                                               cs.zigzag(count), True)[0], 9))
    out = np.empty_like(frames)
    total = 0
    with pipeline.FramePipeline(h, w, 2, delta, count, depth=2, coeffs="zigzag", nearest=True, block_key=9) as pipe:
        assert pipe.coeffs == tuple(cs.zigzag(count))
        pipe.set_payload(payload)
        for k, first in enumerate(range(0, f, 2)):
            n = min(2, f - first)
            pipe.input(k % 2)[:n] = frames[first:first + n]
            total += pipe.submit_embed(k % 2, n, bit_offset=min(first * per, payload.size), first_frame=first)
            out[first:first + n] = pipe.embed_result(k % 2)
        assert total == used and np.array_equal(out, want)
        got = []
        for k, first in enumerate(range(0, f, 2)):
            n = min(2, f - first)
            pipe.input(k % 2)[:n] = out[first:first + n]
            pipe.submit_extract(k % 2, n, first_frame=first)
            packed, n_bits = pipe.extract_result(k % 2)
            got.append(bits_of(packed, n_bits))
    packed, n_bits = batch.extract_frames(want, delta, count, coeffs="zigzag", block_key=9)
    assert np.array_equal(np.concatenate(got), bits_of(packed, n_bits))


def test_error_positions_at_small_delta_equal_the_restatements():
    """delta = 4, n = 3 on noise in [16, 240): the reference's own stego loses bits; zig-zag loses fewer than row-major, and
    the GPU loses exactly the bits the restatement loses - positions compared, no threshold"""
    h, w, delta, n = 480, 640, 4, 3
    gray = np.random.default_rng(1).integers(16, 240, (1, h, w), dtype=np.uint8)
    payload = cs.payload(batch.capacity_bits(1, h, w, n), seed=2)
    for index in (cs.prefix(n), cs.zigzag(n), cs.zigzag(n, 6)):
        stego, used = batch.embed_frames(gray, delta, n, payload, coeffs=index)
        packed, n_bits = batch.extract_frames(stego, delta, n, coeffs=index)
        got = np.flatnonzero(bits_of(packed, n_bits) != payload)
        ref_stego = cs.select_batch_embed(gray, delta, payload, index)[0]
        want = np.flatnonzero(cs.select_batch_extract(ref_stego, delta, index) != payload)
        print(f"delta = {delta}, n = {n}, {index}: {got.size} bit errors (restatement {want.size})")
        assert used == payload.size and np.array_equal(stego, ref_stego) and np.array_equal(got, want)
