"""SVS_MINMOVE on the GPU: every embed entry point with the flag gives minmove_lib.model_embed's bytes - svs_embed_dev (into a
second buffer and in place), the host-pointer svs_embed and svs_embed_str, the ordered and select entry points (a key, and
zigzag:6), svs_embed_readback_dev (stego and counts of the read-back pass started from the model's stego), the fused colour
forms plain and keep-colour - in modes guarded and exact, for the quantiser classes and every kernel family, on both
kernel-matrix shapes with a bit offset and a budget that ends inside the last frame and inside a block; the unchanged receiver
returns the payload; every extract call refuses the flag and writes nothing; with the flag clear the calls give the oracle's
bytes as before; and the Python layers equal the C calls."""
import ctypes as C

import numpy as np
import pytest

import minmove_lib as ml
import nearest_lib as nl
from kernel_matrix import BIT_OFFSET, FIRST_FRAME, KEY, SHAPES
from oracle import qim_dct_oracle as orc
from readback_lib import host_readback
from test_gpu_parity import _Dev
from test_keep_colour_cpu import gray_of
from test_keep_colour_gpu import colour_cover
from svsdct import batch, coeffs, native, order
from svsdct.native import Planes
from svsdct.pipeline import FramePipeline

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

W15 = (3735, 19235, 9798, 15)
FLAGS = {"guarded": native.SVS_EXACT_GUARDED, "exact": native.SVS_EXACT_POCKETFFT}
DELTAS = (8, 20, 7.3, 40)                     # QM_POW2, QM_F32, QM_DOUBLE, QM_F32 with the widest bands
N_ACS = (1, 7, 10, 15, 20, 63)                # one row, one row full, the compile-time two-row form, two rows full, exact U = 8
MM = native.SVS_MINMOVE


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _frames(shape, seed=1):
    """noise, letterboxed, flat and smooth frames in one stack (the shapes have three frames)"""
    f, h, w = SHAPES[shape]
    kinds = ("noise", "letterbox", "flat", "smooth")
    return np.stack([nl.content(kinds[k % 4], h, w, seed=seed + k) for k in range(f)])


def _budget(frames, n_ac):
    """ends inside the last frame and, for n > 1, inside a block"""
    f, h, w = frames.shape
    cap = batch.capacity_bits(f, h, w, n_ac)
    return cap - batch.capacity_bits(1, h, w, n_ac) // 3 - (1 if min(n_ac, 63) > 1 else 0)


def _model(frames, delta, n_ac, bits, off, n_bits, key=None, first=0, index=None):
    src = frames if key is None else order.permute_blocks(frames, key, first)
    want, used = ml.model_batch(src, delta, bits[off:off + n_bits], n_ac, index=index)
    return (want if key is None else order.unpermute_blocks(want, key, first)), used


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", DELTAS)
def test_gray_calls_equal_the_model(delta, mode, shape):
    """svs_embed_dev (second buffer, in place), svs_embed, the ordered calls with a key, svs_embed_readback_dev - every n"""
    frames = _frames(shape)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in, d_out, d_counts = _Dev(frames.nbytes), _Dev(frames.nbytes), _Dev(16)
    for n_ac in N_ACS:
        n_bits = _budget(frames, n_ac)
        bits = nl.payload(BIT_OFFSET + n_bits, seed=n_ac)
        packed = batch.pack_bits(bits)
        d_bits = _Dev(packed.nbytes + 8)
        d_bits.put(packed)
        for key in (None, KEY):
            want, used = _model(frames, delta, n_ac, bits, BIT_OFFSET, n_bits, key, FIRST_FRAME)
            assert used == n_bits
            if key is None and delta >= 20:   # neither the reference's nor the nearest rule's pixels
                assert not np.array_equal(want, orc.batch_embed(frames, delta, bits[BIT_OFFSET:], n_ac)[0])
                assert not np.array_equal(want, nl.model_batch(frames, delta, bits[BIT_OFFSET:BIT_OFFSET + n_bits], n_ac)[0])
            o = batch.block_order(key, FIRST_FRAME)
            d_in.put(frames)
            d_out.put(np.zeros_like(frames))
            got = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                                     mode=mode, order=o, minmove=True)
            assert got == n_bits
            assert np.array_equal(d_out.get().reshape(frames.shape), want), (n_ac, key, "dev")
            assert np.array_equal(d_in.get().reshape(frames.shape), frames)
            batch.embed_device(d_in.ptr.value, d_in.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                               mode=mode, order=o, minmove=True, nearest=True)       # SVS_NEAREST as well changes nothing
            assert np.array_equal(d_in.get().reshape(frames.shape), want), (n_ac, key, "in place")
            stego, used_h = batch.embed_frames(frames, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode,
                                               block_key=key, first_frame=FIRST_FRAME, minmove=True)
            assert used_h == n_bits and np.array_equal(np.array(stego), want), (n_ac, key, "host")
            # the receiver is unchanged: the library's extraction of the flagged stego is the oracle's
            packed_out, n_out = batch.extract_frames(np.array(stego), delta, n_ac, mode=mode, block_key=key, first_frame=FIRST_FRAME)
            src = want if key is None else order.permute_blocks(want, key, FIRST_FRAME)
            assert np.array_equal(np.unpackbits(packed_out, count=n_out), orc.batch_extract_bits(src, delta, n_ac))
            # read-back on top: the pass of the gray read-back call, started from the model's stego
            rb_want, rb_counts, _ = host_readback(want, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, block_key=key,
                                                  first_frame=FIRST_FRAME)
            d_in.put(frames)
            d_counts.put(np.zeros(2, np.uint64))
            got = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                                     mode=mode, order=o, minmove=True, readback=True, d_counts=d_counts.ptr.value)
            assert got == n_bits
            assert tuple(int(v) for v in d_counts.get(16, np.uint64)) == rb_counts, (n_ac, key)
            assert np.array_equal(d_out.get().reshape(frames.shape), rb_want), (n_ac, key, "read-back")


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", DELTAS)
def test_select_calls_equal_the_model(delta, mode, shape):
    """zigzag:6 at every n of the list and a listed set, raster and keyed, host- and device-pointer form.  A scan that starts
    at position 6 has 58 positions left, so n = 63 cannot be zigzag:6: it runs the whole zig-zag scan ("zigzag", all 63 AC
    coefficients in scan order) instead, and 58, the longest count zigzag:6 allows, is added."""
    frames = _frames(shape, seed=5)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in, d_out = _Dev(frames.nbytes), _Dev(frames.nbytes)
    specs = [(n, "zigzag:6") for n in N_ACS if n + 6 <= 64] + [(63, "zigzag"), (58, "zigzag:6"), (3, (9, 2, 17))]
    assert sorted(n for n, _ in specs[:6]) == sorted(N_ACS)
    for n_ac, spec in specs:
        index = coeffs.selection(spec, n_ac)
        n_bits = _budget(frames, n_ac)
        bits = nl.payload(BIT_OFFSET + n_bits, seed=n_ac)
        packed = batch.pack_bits(bits)
        d_bits = _Dev(packed.nbytes + 8)
        d_bits.put(packed)
        for key in (None, KEY):
            want, used = _model(frames, delta, n_ac, bits, BIT_OFFSET, n_bits, key, FIRST_FRAME, index=list(index))
            assert used == n_bits
            stego, used_h = batch.embed_frames(frames, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode,
                                               block_key=key, first_frame=FIRST_FRAME, coeffs=index, minmove=True)
            assert used_h == n_bits and np.array_equal(np.array(stego), want), (spec, n_ac, key, "host")
            d_in.put(frames)
            got = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                                     mode=mode, order=batch.block_order(key, FIRST_FRAME), coeffs=index, minmove=True)
            assert got == n_bits and np.array_equal(d_out.get().reshape(frames.shape), want), (spec, n_ac, key, "dev")


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", DELTAS)
def test_str_form_equals_the_model(delta, mode, shape):
    """svs_embed_str, every n of the list"""
    lib = native.load()
    frames = _frames(shape, seed=4)
    f, h, w = frames.shape
    for n_ac in N_ACS:
        n_bits = _budget(frames, n_ac)
        bits = nl.payload(n_bits, seed=9 + n_ac)
        want, _ = _model(frames, delta, n_ac, bits, 0, n_bits)
        text = batch.bits_to_str(bits).encode()
        out, ref_out = np.empty_like(frames), np.empty_like(frames)
        done = C.c_uint64(0)
        native.check(lib.svs_embed_str(frames.ctypes.data, ref_out.ctypes.data, out.ctypes.data, C.byref(Planes.contiguous(f, h, w)),
                                       float(delta), n_ac, text, len(text), FLAGS[mode] | MM, C.byref(done)), "svs_embed_str")
        assert done.value == n_bits and np.array_equal(ref_out, frames), n_ac
        assert np.array_equal(out, want), n_ac


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", DELTAS)
def test_fused_colour_forms(delta, mode, shape):
    """every n of the list.  plain: B = G = R = the model of the fixed-point gray; keep-colour: gray(output) is the model and
    pixels whose gray did not change keep their bytes; with read-back on top the same holds from the gray read-back pass of
    the model's stego"""
    f, h, w = SHAPES[shape]
    cover = colour_cover(f, h, w, seed=3)
    cover[1, : h // 5 // 8 * 8 + 8] = 0                               # a black bar: blocks that do not read back
    gray = gray_of(cover, W15).astype(np.uint8)
    for n_ac in N_ACS:
        n_bits = _budget(gray, n_ac)
        bits = nl.payload(BIT_OFFSET + n_bits, seed=2 + n_ac)
        want, _ = _model(gray, delta, n_ac, bits, BIT_OFFSET, n_bits)
        kw = dict(bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode, minmove=True)
        plain, gray_ref, used = batch.embed_bgr_frames(cover, delta, n_ac, bits, **kw)
        assert used == n_bits and np.array_equal(np.array(gray_ref), gray), n_ac
        assert np.array_equal(np.array(plain), np.repeat(want[..., None], 3, axis=-1)), n_ac
        kept = np.array(batch.embed_bgr_frames(cover, delta, n_ac, bits, keep_colour=True, **kw)[0])
        assert np.array_equal(gray_of(kept, W15), want), n_ac
        same = want == gray
        assert np.array_equal(kept[same], cover[same]) and not np.array_equal(kept, np.array(plain)), n_ac
        rb_want, rb_counts, _ = host_readback(want, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits)
        out, _, _, counts = batch.embed_bgr_frames(cover, delta, n_ac, bits, readback=True, **kw)
        assert tuple(counts) == rb_counts and np.array_equal(np.array(out), np.repeat(rb_want[..., None], 3, axis=-1)), n_ac
        out, _, _, counts = batch.embed_bgr_frames(cover, delta, n_ac, bits, readback=True, keep_colour=True, **kw)
        assert tuple(counts) == rb_counts and np.array_equal(gray_of(np.array(out), W15), rb_want), n_ac


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", DELTAS)
def test_round_trip_on_content_that_does_not_clip(delta, mode, shape):
    """svs_extract_dev of the GPU stego returns the payload, 0 errors: noise in [64, 192) at delta = 40 and at n = 63, in
    [16, 240) otherwise; the precondition (no stego pixel at 0 or 255) is asserted"""
    lib = native.load()
    f, h, w = SHAPES[shape]
    planes = Planes.contiguous(f, h, w)
    for n_ac in N_ACS:
        frames = np.stack([ml.noclip_content(40 if n_ac == 63 else delta, h, w, seed=20 + k) for k in range(f)])
        cap = batch.capacity_bits(f, h, w, n_ac)
        n_bits = _budget(frames, n_ac)
        bits = nl.payload(BIT_OFFSET + n_bits, seed=n_ac)
        packed = batch.pack_bits(bits)
        d_gray, d_stego, d_bits, d_ext = _Dev(frames.nbytes), _Dev(frames.nbytes), _Dev(packed.nbytes + 8), _Dev(cap // 8 + 16)
        d_gray.put(frames)
        d_bits.put(packed)
        assert batch.embed_device(d_gray.ptr.value, d_stego.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                                  mode=mode, minmove=True) == n_bits
        stego = d_stego.get().reshape(frames.shape)
        assert stego.min() > 0 and stego.max() < 255                      # the precondition
        got = C.c_uint64(0)
        native.check(lib.svs_extract_dev(d_stego.ptr, C.byref(planes), float(delta), n_ac, d_ext.ptr, cap // 8 + 16, FLAGS[mode],
                                         C.byref(got), None), "svs_extract_dev")
        assert got.value == cap
        read = np.unpackbits(d_ext.get((cap + 7) // 8), count=cap)[:n_bits]
        assert np.array_equal(read, bits[BIT_OFFSET:]), (n_ac, int((read != bits[BIT_OFFSET:]).sum()))


def test_every_extract_call_refuses_the_flag_and_writes_nothing():
    lib = native.load()
    frames = _frames("odd")
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    P = C.byref(planes)
    n_ac = 3
    nbytes = batch.capacity_bits(f, h, w, 63) // 8 + 8
    d_gray, d_out = _Dev(frames.nbytes), _Dev(nbytes)
    d_gray.put(frames)
    d_out.put(np.full(nbytes, 0xAB, np.uint8))
    out = np.full(nbytes, 0xAB, np.uint8)
    got = C.c_uint64(77)
    sel = coeffs.native_coeffs((9, 2, 17))
    bo = batch.block_order(KEY, FIRST_FRAME)
    bad = native.SVS_ERR_INVALID_ARG
    for flag in (MM, MM | native.SVS_EXACT_GUARDED, MM | native.SVS_EXACT_POCKETFFT, MM | native.SVS_NEAREST):
        rcs = [lib.svs_extract_dev(d_gray.ptr, P, 8.0, n_ac, d_out.ptr, nbytes, flag, C.byref(got), None),
               lib.svs_extract_ordered_dev(d_gray.ptr, P, C.byref(bo), 8.0, n_ac, d_out.ptr, nbytes, flag, C.byref(got), None),
               lib.svs_extract_select_dev(d_gray.ptr, P, None, C.byref(sel), 8.0, d_out.ptr, nbytes, flag, C.byref(got), None),
               lib.svs_extract_dev(d_gray.ptr, P, 0.0, n_ac, d_out.ptr, nbytes, flag, C.byref(got), None),
               lib.svs_extract(frames.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
               lib.svs_extract_ordered(frames.ctypes.data, P, C.byref(bo), 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
               lib.svs_extract_select(frames.ctypes.data, P, None, C.byref(sel), 8.0, out.ctypes.data, out.size, flag, C.byref(got)),
               lib.svs_extract_str(frames.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got))]
        assert rcs == [bad] * 8, hex(flag)
    assert np.all(out == 0xAB) and np.all(d_out.get() == 0xAB)


@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta,n_ac", [(8, 3), (20, 10), (7.3, 15), (20, 20)])
def test_flag_clear_is_the_oracle_as_before(delta, n_ac, mode):
    """one case per kernel family (one row, two rows compile-time n, two rows, exact) and the fused colour kernel"""
    frames = _frames("even", seed=7)
    n_bits = _budget(frames, n_ac)
    bits = nl.payload(BIT_OFFSET + n_bits, seed=1)
    want = orc.batch_embed(frames, delta, bits[BIT_OFFSET:BIT_OFFSET + n_bits], n_ac)[0]
    stego, used = batch.embed_frames(frames, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode)
    assert used == n_bits and np.array_equal(np.array(stego), want)
    stego, used = batch.embed_frames(frames, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode, minmove=False)
    assert np.array_equal(np.array(stego), want)
    f, h, w = SHAPES["odd"]
    cover = colour_cover(f, h, w, seed=3)
    gray = gray_of(cover, W15).astype(np.uint8)
    n_bits = _budget(gray, n_ac)
    want = orc.batch_embed(gray, delta, bits[BIT_OFFSET:BIT_OFFSET + n_bits], n_ac)[0]
    plain = batch.embed_bgr_frames(cover, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode)[0]
    assert np.array_equal(np.array(plain), np.repeat(want[..., None], 3, axis=-1))


@pytest.mark.parametrize("delta,n_ac", [(20, 10), (40, 3)])
def test_python_layers_equal_the_c_calls(delta, n_ac):
    """batch.embed_frames / embed_device and FramePipeline(minmove=True) against svs_embed_dev called through ctypes"""
    lib = native.load()
    frames = _frames("even", seed=9)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    n_bits = batch.capacity_bits(f, h, w, n_ac) - 11
    bits = nl.payload(n_bits, seed=4)
    packed = batch.pack_bits(bits)
    d_in, d_out, d_bits = _Dev(frames.nbytes), _Dev(frames.nbytes), _Dev(packed.nbytes + 8)
    d_in.put(frames)
    d_bits.put(packed)
    done = C.c_uint64(0)
    native.check(lib.svs_embed_dev(d_in.ptr, d_out.ptr, C.byref(planes), float(delta), n_ac, d_bits.ptr, 0, n_bits,
                                   native.SVS_EXACT_GUARDED | MM, C.byref(done), None), "svs_embed_dev")
    c_call = d_out.get().reshape(frames.shape).copy()
    assert done.value == n_bits and np.array_equal(c_call, _model(frames, delta, n_ac, bits, 0, n_bits)[0])
    assert np.array_equal(np.array(batch.embed_frames(frames, delta, n_ac, bits, mode="guarded", minmove=True)[0]), c_call)
    per = batch.capacity_bits(1, h, w, n_ac)

    def through_pipeline(**kw):
        out = np.empty_like(frames)
        with FramePipeline(h, w, 2, delta, n_ac, depth=2, mode="guarded", **kw) as pipe:
            pipe.set_payload(bits)
            for k, first in enumerate(range(0, f, 2)):
                n = min(2, f - first)
                pipe.input(k % 2)[:n] = frames[first:first + n]
                pipe.submit_embed(k % 2, n, bit_offset=min(first * per, bits.size))
                out[first:first + n] = pipe.embed_result(k % 2)
        return out

    assert np.array_equal(through_pipeline(minmove=True), c_call)
    assert np.array_equal(through_pipeline(), orc.batch_embed(frames, delta, bits, n_ac)[0])
