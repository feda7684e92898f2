"""Keyed block order on the GPU: the ordered embed / extract calls against the reference on block-permuted frames,
    keyed embed(F) = P^-1(oracle embed(P(F)))      keyed extract(S) = oracle extract(P(S))
(svsdct/order.py) - stego pixels and bits, every kernel family and mode - plus round trips, wrong keys, split batches, the
device and host forms, pitched and in-place buffers, and the drop-in loops with SVS_BLOCK_KEY."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import fakes
from oracle import qim_dct_oracle as orc
from test_gpu_parity import _Dev
from test_pipeline import _install, _make_inputs
from svsdct import batch, native, order, synth
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

KEY = 0x0123456789ABCDEF


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def cover(f, h, w, seed):
    """synthetic content with flat, clipping and ramp blocks: guard replays and tie settles run in keyed mode too"""
    frames = synth.synthetic_frames(f, h, w, seed=seed, lo=0, span=256)
    frames[:, :16, :24] = 128
    frames[:, 8:16, 24:40] = 0
    frames[:, -8:, -16:] = 255
    frames[:, 16:24, :] = np.arange(w, dtype=np.uint8)[None, None, :] * 3
    return frames


def expected_embed(frames, delta, n_ac, payload, key, first_frame=0):
    stego, used = orc.batch_embed(order.permute_blocks(frames, key, first_frame), delta, payload, n_ac)
    return order.unpermute_blocks(stego, key, first_frame), used


def expected_bits(stego, delta, n_ac, key, first_frame=0):
    return orc.batch_extract_bits(order.permute_blocks(stego, key, first_frame), delta, n_ac)


# (frames, height, width): 16 blocks per row (the one-row kernel's two-block layout), 9 (one block per lane)
SHAPES = [(3, 32, 128), (2, 40, 72)]


@pytest.mark.parametrize("n_ac", [1, 3, 7, 8, 10, 15, 16, 20, 63])
@pytest.mark.parametrize("shape", SHAPES, ids=["two_blocks", "one_block"])
def test_keyed_embed_and_extract_equal_the_oracle_on_permuted_frames(n_ac, shape):
    f, h, w = shape
    frames = cover(f, h, w, seed=n_ac)
    cap = batch.capacity_bits(f, h, w, n_ac)
    payload = synth.synthetic_bits(cap - (cap // f) // 3 - 1, seed=100 + n_ac)      # ends mid-frame and (n > 1) mid-block
    for delta in (4, 8, 20, 5000):                                                   # 5000: outside the guard's range
        want, want_used = expected_embed(frames, delta, n_ac, payload, KEY, first_frame=5)
        want_bits = expected_bits(want, delta, n_ac, KEY, first_frame=5)
        for mode in ("fast", "guarded", "exact"):
            stego, used = batch.embed_frames(frames, delta, n_ac, payload, mode=mode, block_key=KEY, first_frame=5)
            assert used == want_used == payload.size
            assert np.array_equal(stego, want), (n_ac, delta, mode, np.argwhere(stego != want)[:4])
            packed, n_bits = batch.extract_frames(stego, delta, n_ac, mode=mode, block_key=KEY, first_frame=5)
            got = np.unpackbits(packed, count=n_bits)
            assert n_bits == cap and np.array_equal(got, want_bits), (n_ac, delta, mode)


@pytest.mark.parametrize("n_ac", [3, 10])
def test_wrong_key_unkeyed_and_wrong_frame_do_not_decode(n_ac):
    frames = synth.synthetic_frames(2, 64, 128, seed=3)
    cap = batch.capacity_bits(2, 64, 128, n_ac)
    payload = synth.synthetic_bits(cap // 3, seed=9)
    stego, _ = batch.embed_frames(frames, 20, n_ac, payload, block_key=7)
    for kw in ({}, {"block_key": 8}, {"block_key": 7, "first_frame": 1}):
        packed, n = batch.extract_frames(stego, 20, n_ac, **kw)
        got = np.unpackbits(packed, count=n)[: payload.size]
        assert (got != payload).mean() > 0.3, kw
    # keyed embed + keyed extract returns the payload as well as the reference's own round trip does (unkeyed, same frames)
    plain, _ = batch.embed_frames(frames, 20, n_ac, payload)
    packed, n = batch.extract_frames(stego, 20, n_ac, block_key=7)
    keyed_errors = int((np.unpackbits(packed, count=n)[: payload.size] != payload).sum())
    packed, n = batch.extract_frames(plain, 20, n_ac)
    plain_errors = int((np.unpackbits(packed, count=n)[: payload.size] != payload).sum())
    assert keyed_errors <= max(2 * plain_errors, payload.size // 1000), (keyed_errors, plain_errors)
    # two thirds of frame 0's capacity: raster order leaves its bottom rows alone, the keyed order spreads the bits over the
    # whole frame; frame 1 carries nothing either way (frames keep their stream ranges)
    assert np.array_equal(plain[0, 48:], frames[0, 48:])
    assert not np.array_equal(stego[0, 48:], frames[0, 48:])
    assert np.array_equal(stego[1], frames[1]) and np.array_equal(plain[1], frames[1])


def test_4k_keyed_equals_unkeyed_on_permuted_frames():
    """at 4K and full capacity (every block takes bits), keyed output = P^-1(unkeyed GPU output on P(F))"""
    f, h, w, n_ac, delta = 3, 2160, 3840, 3, 8
    frames = synth.synthetic_frames(f, h, w, seed=41)
    frames[1, :64, :] = 128
    payload = synth.synthetic_bits(batch.capacity_bits(f, h, w, n_ac), seed=42)
    stego, used = batch.embed_frames(frames, delta, n_ac, payload, block_key=(1 << 64) - 1, first_frame=1000)
    plain, used2 = batch.embed_frames(order.permute_blocks(frames, (1 << 64) - 1, 1000), delta, n_ac, payload)
    assert used == used2 == payload.size
    assert np.array_equal(stego, order.unpermute_blocks(plain, (1 << 64) - 1, 1000))
    packed, n = batch.extract_frames(stego, delta, n_ac, block_key=(1 << 64) - 1, first_frame=1000)
    assert np.array_equal(np.unpackbits(packed, count=n), payload)
    packed2, _ = batch.extract_frames(plain, delta, n_ac)
    assert np.array_equal(packed, packed2)


@pytest.mark.parametrize("n_ac", [3, 10, 20])
def test_split_batches_device_forms_pitched_and_in_place(n_ac):
    lib = native.load()
    f, h, w, delta = 4, 32, 128, 8
    frames = cover(f, h, w, seed=17)
    cap = batch.capacity_bits(f, h, w, n_ac)
    bit_offset = 37
    stream = synth.synthetic_bits(bit_offset + cap - 5, seed=18)
    whole, used = batch.embed_frames(frames, delta, n_ac, stream, bit_offset=bit_offset, block_key=KEY, first_frame=2)
    assert used == cap - 5
    want, _ = expected_embed(frames, delta, n_ac, stream[bit_offset:], KEY, first_frame=2)
    assert np.array_equal(whole, want)
    # two calls: frames [0, 1) and [1, 4) with first_frame offsets and the bit offset of frame 1
    per = cap // f
    a, _ = batch.embed_frames(frames[:1], delta, n_ac, stream, bit_offset=bit_offset, n_bits=per, block_key=KEY, first_frame=2)
    b, _ = batch.embed_frames(frames[1:], delta, n_ac, stream, bit_offset=bit_offset + per, block_key=KEY, first_frame=3)
    assert np.array_equal(np.concatenate([a, b]), whole)
    pa, na = batch.extract_frames(whole[:1], delta, n_ac, block_key=KEY, first_frame=2)
    pb, nb = batch.extract_frames(whole[1:], delta, n_ac, block_key=KEY, first_frame=3)
    pw, nw = batch.extract_frames(whole, delta, n_ac, block_key=KEY, first_frame=2)
    assert np.array_equal(np.concatenate([np.unpackbits(pa, count=na), np.unpackbits(pb, count=nb)]),
                          np.unpackbits(pw, count=nw))

    # device forms on pitched planes, in place, with the payload at a bit offset of a device buffer
    row_pitch, frame_pitch = 160, 160 * h + 64
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    view = np.lib.stride_tricks.as_strided(host, (f, h, w), (frame_pitch, row_pitch, 1))
    view[...] = frames
    d = _Dev(host.size)
    d.put(host)
    packed = batch.pack_bits(stream)
    d_bits = _Dev(packed.size)
    d_bits.put(packed)
    o = batch.block_order(KEY, 2)
    got = batch.embed_device(d.ptr.value, d.ptr.value, planes, delta, n_ac, d_bits.ptr.value, bit_offset, len(stream) - bit_offset,
                             order=o)
    assert got == cap - 5
    out = d.get()
    assert np.array_equal(np.lib.stride_tricks.as_strided(out, (f, h, w), (frame_pitch, row_pitch, 1)), whole)
    pad = np.ones(host.size, bool)
    np.lib.stride_tricks.as_strided(pad, (f, h, w), (frame_pitch, row_pitch, 1))[...] = False
    assert (out[pad] == 0xAB).all()                                        # padding untouched
    nbytes = (cap + 7) // 8
    d_out = _Dev(nbytes + 8)
    d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
    assert batch.extract_device(d.ptr.value, planes, delta, n_ac, d_out.ptr.value, nbytes, order=o) == cap
    res = d_out.get()
    assert np.array_equal(res[:nbytes], pw[:nbytes])
    assert (res[nbytes:] == 0x5A).all()                                    # nothing written past the packed bits
    # order = NULL: the unordered call's bytes
    plain, _ = batch.embed_frames(frames, delta, n_ac, stream, bit_offset=bit_offset)
    d.put(host)
    done = C.c_uint64(0)
    native.check(lib.svs_embed_ordered_dev(d.ptr, d.ptr, C.byref(planes), None, float(delta), n_ac, d_bits.ptr, bit_offset,
                                           len(stream) - bit_offset, batch.mode_flags(None), C.byref(done), None), "embed")
    native.check(lib.svs_stream_synchronize(None), "sync")
    assert np.array_equal(np.lib.stride_tricks.as_strided(d.get(), (f, h, w), (frame_pitch, row_pitch, 1)), plain)
    ref_packed, _ = batch.extract_frames(plain, delta, n_ac)
    out_null = np.zeros(nbytes + 4, np.uint8)
    gotn = C.c_uint64(0)
    native.check(lib.svs_extract_ordered(plain.ctypes.data, C.byref(Planes.contiguous(f, h, w)), None, float(delta), n_ac,
                                         out_null.ctypes.data, out_null.size, batch.mode_flags(None), C.byref(gotn)), "extract")
    assert np.array_equal(out_null[:nbytes], ref_packed[:nbytes])


def test_large_frames_host_form_stages_whole_frames():
    """a 4K frame is larger than a staging chunk: the keyed host call keeps it whole and equals the device call"""
    f, h, w, n_ac, delta = 2, 2160, 3840, 10, 20
    frames = synth.synthetic_frames(f, h, w, seed=61)
    payload = synth.synthetic_bits(batch.capacity_bits(f, h, w, n_ac) // 2 + 333, seed=62)
    stego, _ = batch.embed_frames(frames, delta, n_ac, payload, block_key=5, first_frame=9)
    d = _Dev(frames.nbytes)
    d.put(frames)
    packed = batch.pack_bits(payload)
    d_bits = _Dev(packed.size)
    d_bits.put(packed)
    batch.embed_device(d.ptr.value, d.ptr.value, Planes.contiguous(f, h, w), delta, n_ac, d_bits.ptr.value, 0, payload.size,
                       order=batch.block_order(5, 9))
    assert np.array_equal(d.get().reshape(frames.shape), stego)
    out, n = batch.extract_frames(stego, delta, n_ac, block_key=5, first_frame=9)
    assert np.array_equal(np.unpackbits(out, count=n)[: payload.size], payload)


def test_drop_in_loops_with_block_key(monkeypatch, tmp_path, capsys):
    emb, ext = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    monkeypatch.setattr(ext, "BATCH_FRAMES", 2)
    frames, secret, secret_path = _make_inputs(tmp_path, n_frames=9, size=(40, 56), secret=(12, 10), seed=23)
    receiver = fakes.FakeKey(b"bob")
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(receiver.public())
    delta, n_ac = 16, 12
    monkeypatch.setenv("SVS_BLOCK_KEY", "0xfeedface12345678")
    ok, g0, s0 = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "keyed"), delta, n_ac, pub)
    assert ok and g0.shape == s0.shape == (40, 56)
    out_png = str(tmp_path / "o.png")
    assert ext.ekstraksi_gambar_video_final(str(tmp_path / "keyed.avi"), out_png, delta, n_ac, receiver)
    assert np.array_equal(np.asarray(Image.open(out_png)), secret)
    monkeypatch.setattr(ext, "FUSED_COLOUR", True)                       # keyed: the host-conversion gray path
    assert ext.ekstraksi_gambar_video_final(str(tmp_path / "keyed.avi"), str(tmp_path / "o2.png"), delta, n_ac, receiver)
    monkeypatch.setattr(ext, "FUSED_COLOUR", False)
    # another key, or none: extraction fails cleanly
    for other in ("0xfeedface12345679", None):
        if other is None:
            monkeypatch.delenv("SVS_BLOCK_KEY")
        else:
            monkeypatch.setenv("SVS_BLOCK_KEY", other)
        assert ext.ekstraksi_gambar_video_final(str(tmp_path / "keyed.avi"), str(tmp_path / "x.png"), delta, n_ac,
                                                receiver) is False
    # invalid values: one line and the reference's failure value; with SVS_KEEP_COLOUR the embed is refused
    for bad in ("-3", "0x10000000000000000", "abc"):
        monkeypatch.setenv("SVS_BLOCK_KEY", bad)
        capsys.readouterr()
        assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "b"), delta, n_ac, pub) == (False, None, None)
        assert "SVS_BLOCK_KEY" in capsys.readouterr().out
        assert ext.ekstraksi_gambar_video_final(str(tmp_path / "keyed.avi"), str(tmp_path / "b.png"), delta, n_ac, receiver) is False
    monkeypatch.setenv("SVS_BLOCK_KEY", "1")
    monkeypatch.setattr(emb, "KEEP_COLOUR", True)
    capsys.readouterr()
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "k"), delta, n_ac, pub) == (False, None, None)
    assert "SVS_KEEP_COLOUR" in capsys.readouterr().out
    # with SVS_FUSED_COLOUR the keyed embed takes the gray path and the receiver still decodes
    monkeypatch.setattr(emb, "KEEP_COLOUR", False)
    monkeypatch.setattr(emb, "FUSED_COLOUR", True)
    ok, _, _ = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "fused"), delta, n_ac, pub)
    assert ok
    assert ext.ekstraksi_gambar_video_final(str(tmp_path / "fused.avi"), str(tmp_path / "f.png"), delta, n_ac, receiver)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "f.png"))), secret)
