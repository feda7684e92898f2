"""SVS_NEAREST on the GPU: every embed entry point with the flag gives nearest_lib.model_embed's bytes - the gray calls in the
device- and host-pointer forms, guarded and exact, the quantiser modes and coefficient counts of the CPU tier, both kernel-matrix
shapes, a budget that ends inside a frame and a block, a bit offset, in place, keyed, the _str form, the fused colour forms and
the read-back forms - a 16 x 4K batch agrees with the exact kernel, decodes without errors and has the higher PSNR, and the
drop-in loop round-trips a framed payload with SVS_NEAREST=1."""
import ctypes as C
import math

import numpy as np
import pytest

import fakes
import nearest_lib as nl
from kernel_matrix import BIT_OFFSET, FIRST_FRAME, KEY, SHAPES
from oracle import qim_dct_oracle as orc
from readback_lib import host_readback
from test_gpu_parity import _Dev
from test_keep_colour_cpu import gray_of
from test_keep_colour_gpu import colour_cover
from test_pipeline import _install, _make_inputs
from svsdct import batch, framing, native, order
from svsdct.native import Planes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

W15 = (3735, 19235, 9798, 15)
FLAGS = {"guarded": native.SVS_EXACT_GUARDED, "exact": native.SVS_EXACT_POCKETFFT}


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _frames(shape, seed=1):
    """noise, smooth, flat and letterboxed frames in one stack (the shapes have three frames)"""
    f, h, w = SHAPES[shape]
    kinds = ("noise", "letterbox", "flat", "smooth")
    return np.stack([nl.content(kinds[k % 4], h, w, seed=seed + k) for k in range(f)])


def _budget(frames, n_ac):
    """ends inside the last frame and, for n > 1, inside a block"""
    f, h, w = frames.shape
    cap = batch.capacity_bits(f, h, w, n_ac)
    return cap - batch.capacity_bits(1, h, w, n_ac) // 3 - (1 if min(n_ac, 63) > 1 else 0)


def _model(frames, delta, n_ac, bits, off, n_bits, key=None, first=0):
    src = frames if key is None else order.permute_blocks(frames, key, first)
    want, used = nl.model_batch(src, delta, bits[off:off + n_bits], n_ac)
    return (want if key is None else order.unpermute_blocks(want, key, first)), used


@pytest.mark.parametrize("shape", ["even", "odd"])
@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta", nl.DELTAS)
def test_gray_calls_equal_the_model(delta, mode, shape):
    """device-pointer call (into a second buffer, then in place) and host-pointer call, raster and keyed, every n of the list"""
    lib = native.load()
    frames = _frames(shape)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in, d_out = _Dev(frames.nbytes), _Dev(frames.nbytes)
    for n_ac in nl.N_ACS:
        n_bits = _budget(frames, n_ac)
        bits = nl.payload(BIT_OFFSET + n_bits, seed=n_ac)
        packed = batch.pack_bits(bits)
        d_bits = _Dev(packed.nbytes + 8)
        d_bits.put(packed)
        for key in (None, KEY):
            want, used = _model(frames, delta, n_ac, bits, BIT_OFFSET, n_bits, key, FIRST_FRAME)
            ref = orc.batch_embed(frames if key is None else order.permute_blocks(frames, key, FIRST_FRAME), delta,
                                  bits[BIT_OFFSET:], n_ac)[0]
            assert used == n_bits
            if delta >= 7:      # not the reference's pixels (below, a move of delta / 2 need not reach a pixel)
                assert not np.array_equal(want, ref if key is None else order.unpermute_blocks(ref, key, FIRST_FRAME))
            o = batch.block_order(key, FIRST_FRAME)
            d_in.put(frames)
            d_out.put(np.zeros_like(frames))
            got = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                                     mode=mode, order=o, nearest=True)
            assert got == n_bits
            assert np.array_equal(d_out.get().reshape(frames.shape), want), (n_ac, key, "dev")
            assert np.array_equal(d_in.get().reshape(frames.shape), frames)
            batch.embed_device(d_in.ptr.value, d_in.ptr.value, planes, delta, n_ac, d_bits.ptr.value, BIT_OFFSET, n_bits,
                               mode=mode, order=o, nearest=True)
            assert np.array_equal(d_in.get().reshape(frames.shape), want), (n_ac, key, "in place")
            stego, used_h = batch.embed_frames(frames, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode,
                                               block_key=key, first_frame=FIRST_FRAME, nearest=True)
            assert used_h == n_bits and np.array_equal(np.array(stego), want), (n_ac, key, "host")
            # the receiver is unchanged: the library's extraction of the flagged stego is the oracle's
            packed_out, n_out = batch.extract_frames(np.array(stego), delta, n_ac, mode=mode, block_key=key, first_frame=FIRST_FRAME)
            src = want if key is None else order.permute_blocks(want, key, FIRST_FRAME)
            assert np.array_equal(np.unpackbits(packed_out, count=n_out), orc.batch_extract_bits(src, delta, n_ac))
    # the flag is refused by the extract calls with device work pending or not, and unknown bits stay unknown behind the staging
    got_bits = C.c_uint64(0)
    out = np.zeros(batch.capacity_bits(f, h, w, 63) // 8 + 8, np.uint8)
    for flag in (native.SVS_NEAREST | FLAGS[mode], 0x4, 0x400, 0x80000000):
        assert lib.svs_extract(frames.ctypes.data, C.byref(planes), float(delta), 3, out.ctypes.data, out.size, flag,
                               C.byref(got_bits)) == native.SVS_ERR_INVALID_ARG


@pytest.mark.parametrize("delta,n_ac", [(8, 3), (20, 10), (7.3, 20)])
def test_str_form_equals_the_packed_call(delta, n_ac):
    lib = native.load()
    frames = _frames("even", seed=4)
    f, h, w = frames.shape
    n_bits = _budget(frames, n_ac)
    bits = nl.payload(n_bits, seed=9)
    want, _ = _model(frames, delta, n_ac, bits, 0, n_bits)
    packed_call, _ = batch.embed_frames(frames, delta, n_ac, bits, nearest=True)
    text = batch.bits_to_str(bits).encode()
    out, ref_out = np.empty_like(frames), np.empty_like(frames)
    done = C.c_uint64(0)
    native.check(lib.svs_embed_str(frames.ctypes.data, ref_out.ctypes.data, out.ctypes.data, C.byref(Planes.contiguous(f, h, w)),
                                   float(delta), n_ac, text, len(text), native.SVS_EXACT_GUARDED | native.SVS_NEAREST,
                                   C.byref(done)), "svs_embed_str")
    assert done.value == n_bits and np.array_equal(ref_out, frames)
    assert np.array_equal(out, np.array(packed_call)) and np.array_equal(out, want)


@pytest.mark.parametrize("mode", ["guarded", "exact"])
@pytest.mark.parametrize("delta,n_ac", [(8, 3), (20, 7), (7.3, 10), (20, 15), (8, 20), (0.1, 5)])
def test_fused_colour_forms(delta, n_ac, mode):
    """plain: B = G = R = the model of the fixed-point gray; keep-colour: gray(output) is the model and pixels whose gray did
    not change keep their bytes; with read-back on top the same holds from the gray read-back call's stego"""
    f, h, w = SHAPES["odd"]
    cover = colour_cover(f, h, w, seed=3)
    cover[1, : h // 5 // 8 * 8 + 8] = 0                               # a black bar: blocks that do not read back
    gray = gray_of(cover, W15).astype(np.uint8)
    n_bits = _budget(gray, n_ac)
    bits = nl.payload(BIT_OFFSET + n_bits, seed=2)
    want, _ = _model(gray, delta, n_ac, bits, BIT_OFFSET, n_bits)
    kw = dict(bit_offset=BIT_OFFSET, n_bits=n_bits, mode=mode, nearest=True)
    plain, gray_ref, used = batch.embed_bgr_frames(cover, delta, n_ac, bits, **kw)
    assert used == n_bits and np.array_equal(np.array(gray_ref), gray)
    assert np.array_equal(np.array(plain), np.repeat(want[..., None], 3, axis=-1))
    kept = np.array(batch.embed_bgr_frames(cover, delta, n_ac, bits, keep_colour=True, **kw)[0])
    assert np.array_equal(gray_of(kept, W15), want)
    same = want == gray
    assert np.array_equal(kept[same], cover[same]) and not np.array_equal(kept, np.array(plain))
    # read-back: the gray call from the model's stego
    rb_want, rb_counts, _ = host_readback(want, delta, n_ac, bits, bit_offset=BIT_OFFSET, n_bits=n_bits)
    out, _, _, counts = batch.embed_bgr_frames(cover, delta, n_ac, bits, readback=True, **kw)
    assert tuple(counts) == rb_counts and np.array_equal(np.array(out), np.repeat(rb_want[..., None], 3, axis=-1))
    out, _, _, counts = batch.embed_bgr_frames(cover, delta, n_ac, bits, readback=True, keep_colour=True, **kw)
    assert tuple(counts) == rb_counts and np.array_equal(gray_of(np.array(out), W15), rb_want)


@pytest.mark.parametrize("key", [None, KEY], ids=["raster", "keyed"])
@pytest.mark.parametrize("delta,n_ac", [(20, 10), (8, 3), (16, 20)])
@pytest.mark.parametrize("kind", ["letterbox", "saturated"])
def test_with_readback(kind, delta, n_ac, key):
    """both flags: the result and the counts are the gray read-back pass started from the model's stego; a block that reads
    back keeps the nearest-rule bytes; every accepted block decodes"""
    from readback_lib import content, payload
    if kind == "saturated":      # 248 .. 255: clips at 255
        frames = np.stack([(255 - np.random.default_rng(3 + k).integers(0, 256, (48, 96)) // 32).astype(np.uint8) for k in range(2)])
    else:
        frames = np.stack([content(kind, 48, 96, seed=3 + k) for k in range(2)])
    n_bits = batch.capacity_bits(2, 48, 96, n_ac) - 37
    bits = payload(n_bits)
    start, _ = _model(frames, delta, n_ac, bits, 0, n_bits, key, 3)
    want, want_counts, status = host_readback(start, delta, n_ac, bits, block_key=key, first_frame=3)
    stego, used, counts = batch.embed_frames(frames, delta, n_ac, bits, block_key=key, first_frame=3, readback=True, nearest=True)
    assert used == n_bits and tuple(counts) == want_counts
    if kind == "letterbox":      # the bars fail at every setting; saturated content at delta = 8, n = 3 has no failing block
        assert want_counts[0] > 20
    assert np.array_equal(np.array(stego), want)
    blocks = lambda a: order._blocks(a).reshape(-1, 8, 8)
    kept = status == 0
    assert kept.sum() > 0 and np.array_equal(blocks(want)[kept], blocks(start)[kept])
    # decode through the library; bits of blocks left unrepaired (status 2) may differ, every other payload bit must not
    packed, n = batch.extract_frames(want, delta, n_ac, block_key=key, first_frame=3)
    got = np.unpackbits(packed, count=n)[:n_bits]
    src_status = status.reshape(2, -1)
    if key is not None:
        src_status = np.stack([src_status[k][order.slot_to_block(key, 3 + k, src_status.shape[1])] for k in range(2)])
    ok = np.repeat(src_status.reshape(-1) != 2, n_ac)[:n_bits]
    assert np.array_equal(got[ok], bits[ok])


def _psnr(sse, h, w):
    return math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 * h * w / sse)


@pytest.mark.parametrize("delta,n_ac", [(20, 10), (8, 3)])
def test_full_size_batch(delta, n_ac):
    """16 x 3840x2160, guarded: equal to the exact kernel under the same flag, one frame equal to the model, 0 payload bit
    errors through svs_extract_dev, and a higher PSNR against the cover than the same call without the flag"""
    lib = native.load()
    f, h, w = 16, 2160, 3840
    planes = Planes.contiguous(f, h, w)
    cap = batch.capacity_bits(f, h, w, n_ac)
    nbytes = (cap + 7) // 8 + 8
    d_gray, d_a, d_b = _Dev(f * h * w), _Dev(f * h * w), _Dev(f * h * w)
    d_bits, d_ext, d_sse, d_err = _Dev(nbytes), _Dev(nbytes), _Dev(8 * f), _Dev(8)
    native.check(lib.svs_fill_synthetic_dev(d_gray.ptr, C.byref(planes), 1, 0, 16, 224, None), "fill")
    native.check(lib.svs_fill_bits_dev(d_bits.ptr, cap, 7, 0, None), "fill_bits")

    def sse(a, b):
        native.check(lib.svs_frame_sse_dev(a.ptr, b.ptr, C.byref(planes), d_sse.ptr, None), "sse")
        return d_sse.get(8 * f, np.uint64)

    def embed(dst, mode, nearest):
        used = batch.embed_device(d_gray.ptr.value, dst.ptr.value, planes, delta, n_ac, d_bits.ptr.value, 0, cap, mode=mode,
                                  nearest=nearest)
        assert used == cap

    embed(d_a, "guarded", False)
    sse_off = sse(d_gray, d_a)
    embed(d_a, "guarded", True)
    embed(d_b, "exact", True)
    assert not sse(d_a, d_b).any()
    sse_on = sse(d_gray, d_a)
    p_off, p_on = _psnr(int(sse_off.sum()) / f, h, w), _psnr(int(sse_on.sum()) / f, h, w)
    print(f"delta {delta} n {n_ac}: PSNR against the cover, 16 x 4K noise in [16, 240): {p_off:.2f} -> {p_on:.2f} dB")
    assert np.all(sse_on < sse_off)                                   # every frame's PSNR is higher with the flag
    got = C.c_uint64(0)
    native.check(lib.svs_extract_dev(d_a.ptr, C.byref(planes), float(delta), n_ac, d_ext.ptr, nbytes, native.SVS_EXACT_GUARDED,
                                     C.byref(got), None), "extract")
    native.check(lib.svs_bit_errors_dev(d_ext.ptr, d_bits.ptr, cap, d_err.ptr, None), "bit_errors")
    assert got.value == cap and int(d_err.get(8, np.uint64)[0]) == 0
    # the last frame against the model
    k = f - 1
    per = cap // f
    cover = np.empty((h, w), np.uint8)
    stego = np.empty((h, w), np.uint8)
    for dst, src in ((cover, d_gray), (stego, d_a)):
        native.check(lib.svs_memcpy_d2h(dst.ctypes.data, C.c_void_p(src.ptr.value + k * h * w), h * w, None), "d2h")
    native.check(lib.svs_stream_synchronize(None), "sync")
    bits = np.unpackbits(d_bits.get((cap + 7) // 8), count=cap)[k * per:(k + 1) * per]
    assert np.array_equal(stego, nl.model_embed(cover, delta, bits, n_ac)[1])


def test_drop_in_loop_round_trips_with_the_switch(monkeypatch, tmp_path, capsys):
    """a svsdct.framing stream through embed_process with SVS_NEAREST=1 comes back bit for bit through the unchanged receiver;
    the frames are the model's, not the reference's"""
    emb, ext = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    monkeypatch.setattr(emb, "NEAREST", True)
    frames, secret, secret_path = _make_inputs(tmp_path, n_frames=6, size=(96, 160), secret=(12, 10), seed=31)
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    delta, n_ac = 20, 10
    made = []
    real = emb._siapkan_payload
    monkeypatch.setattr(emb, "_siapkan_payload", lambda *a: made.append(real(*a)) or made[-1])
    ok, g0, s0 = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "near"), delta, n_ac, pub)
    assert ok and "SVS_NEAREST" in capsys.readouterr().out
    video = fakes.VIDEOS[str(tmp_path / "near.avi")]["frames"]
    gray = np.stack([fr[..., 0] for fr in video])
    packed, n = batch.extract_frames(gray, delta, n_ac)
    got = np.unpackbits(packed, count=n)[: made[-1].size]
    assert np.array_equal(got, made[-1])
    header = framing.parse_header(got)
    assert (header.width, header.height) == (12, 10)
    cap = batch.capacity_bits(1, 96, 160, n_ac)
    first = np.array(g0)
    assert np.array_equal(np.array(s0), nl.model_embed(first, delta, made[-1][:cap], n_ac)[1])
    assert not np.array_equal(np.array(s0), orc.frame_embed(first, delta, made[-1][:cap], n_ac)[1])
