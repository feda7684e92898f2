"""SVS_READBACK on the GPU: readback_kernel's output equals the host build of the same arithmetic (csrc/svs_readback.hpp via
tests/hostemu) byte for byte with the same counts - raster and keyed order, the device call in place, the host-pointer
call over several staging chunks - content without failures comes out byte-identical to the call without the flag,
letterboxed 1080p frames that the reference's stego cannot deliver decode exactly, and a framed payload survives the drop-in
video loop."""
import ctypes as C

import numpy as np
import pytest

import fakes
from oracle import qim_dct_oracle as orc
from readback_lib import content, host_readback, payload
from test_gpu_parity import _Dev
from test_pipeline import _install, _make_inputs
from svsdct import batch, framing, native, order
from svsdct.native import Planes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KEY = 0x0123456789ABCDEF


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def frames_of(kind, f, h, w, seed=1):
    return np.stack([content(kind, h, w, seed=seed + k) for k in range(f)])


def embed_pair(frames, delta, n_ac, bits, key=None, first_frame=0, **kw):
    """(unflagged stego, flagged stego, counts) through the host-pointer calls"""
    s0, used0 = batch.embed_frames(frames, delta, n_ac, bits, block_key=key, first_frame=first_frame, **kw)
    s1, used1, counts = batch.embed_frames(frames, delta, n_ac, bits, block_key=key, first_frame=first_frame, readback=True,
                                           **kw)
    assert used0 == used1
    return np.array(s0), np.array(s1), counts


@pytest.mark.parametrize("key", [None, KEY], ids=["raster", "keyed"])
@pytest.mark.parametrize("delta,n_ac", [(20, 10), (8, 3), (4, 3), (20, 63), (7.5, 5), (0.1, 12)])
@pytest.mark.parametrize("kind", ["letterbox", "bright", "flat0", "noise"])
def test_gpu_equals_host_emulation(kind, delta, n_ac, key):
    frames = frames_of(kind, 2, 48, 96)
    cap = batch.capacity_bits(2, 48, 96, n_ac)
    bits = payload(cap - 37)
    s0, s1, counts = embed_pair(frames, delta, n_ac, bits, key=key, first_frame=3)
    want, want_counts, _ = host_readback(s0, delta, n_ac, bits, block_key=key, first_frame=3)
    assert np.array_equal(s1, want)
    assert tuple(counts) == want_counts


@pytest.mark.parametrize("key", [None, KEY], ids=["raster", "keyed"])
def test_device_call_in_place_with_counts(key):
    lib = native.load()
    f, h, w, delta, n_ac, off = 3, 64, 128, 16, 10, 45
    frames = frames_of("letterbox", f, h, w, seed=7)
    planes = Planes.contiguous(f, h, w)
    cap = batch.capacity_bits(f, h, w, n_ac)
    bits = payload(off + cap)
    packed = batch.pack_bits(bits)
    d_frames, d_bits, d_counts = _Dev(frames.nbytes), _Dev(packed.nbytes + 8), _Dev(16)
    d_bits.put(packed)
    o = batch.block_order(key, 2)
    ref = C.byref(o) if o is not None else None
    # the reference's stego (the call without the flag, in place), then the flagged call in place from the cover
    d_frames.put(frames)
    done = C.c_uint64(0)
    native.check(lib.svs_embed_ordered_dev(d_frames.ptr, d_frames.ptr, C.byref(planes), ref, float(delta), n_ac, d_bits.ptr,
                                           off, cap, native.SVS_EXACT_GUARDED, C.byref(done), None), "embed")
    s0 = d_frames.get().reshape(frames.shape)
    d_frames.put(frames)
    d_counts.put(np.array([5, 7], np.uint64))                         # the call adds into the buffer
    native.check(lib.svs_embed_readback_dev(d_frames.ptr, d_frames.ptr, C.byref(planes), ref, float(delta), n_ac, d_bits.ptr,
                                            off, cap, native.SVS_EXACT_GUARDED, C.byref(done), d_counts.ptr, None), "readback")
    s1 = d_frames.get().reshape(frames.shape)
    counts = d_counts.get(16, np.uint64)
    want, want_counts, _ = host_readback(s0, delta, n_ac, bits, bit_offset=off, n_bits=cap, block_key=key, first_frame=2)
    assert want_counts[0] > 50
    assert np.array_equal(s1, want) and tuple(int(c) for c in counts) == (want_counts[0] + 5, want_counts[1] + 7)
    # the plain flagged call gives the same bytes and reports nothing
    d_frames.put(frames)
    native.check(lib.svs_embed_ordered_dev(d_frames.ptr, d_frames.ptr, C.byref(planes), ref, float(delta), n_ac, d_bits.ptr,
                                           off, cap, native.SVS_EXACT_GUARDED | native.SVS_READBACK, C.byref(done), None),
                 "flagged")
    assert np.array_equal(d_frames.get().reshape(frames.shape), want)


def test_host_call_over_several_staging_chunks():
    """two 4K frames travel as bands of block rows: every band's bit offset and budget, and the counts summed over them"""
    f, h, w, delta, n_ac, off = 2, 2160, 3840, 20, 10, 77
    frames = frames_of("letterbox", f, h, w, seed=11)
    cap = batch.capacity_bits(f, h, w, n_ac)
    bits = payload(off + cap - 1234)
    s0, s1, counts = embed_pair(frames, delta, n_ac, bits, bit_offset=off)
    want, want_counts, _ = host_readback(s0, delta, n_ac, bits, bit_offset=off)
    assert want_counts[0] > 10000 and want_counts[1] == 0
    assert tuple(counts) == want_counts and np.array_equal(s1, want)
    # and the _str form takes the flag (it reports no counts)
    ascii_payload = batch.bits_to_str(bits[off:])
    lib = native.load()
    out = np.empty_like(frames)
    done = C.c_uint64(0)
    native.check(lib.svs_embed_str(frames.ctypes.data, None, out.ctypes.data, C.byref(Planes.contiguous(f, h, w)), float(delta),
                                   n_ac, ascii_payload.encode(), len(ascii_payload), native.SVS_EXACT_GUARDED |
                                   native.SVS_READBACK, C.byref(done)), "svs_embed_str")
    assert np.array_equal(out, want)


@pytest.mark.parametrize("kind", ["noise", "natural"])
def test_content_without_failures_is_byte_identical(kind):
    f, h, w, delta, n_ac = 2, 1080, 1920, 8, 3
    frames = frames_of(kind, f, h, w, seed=5)
    bits = payload(batch.capacity_bits(f, h, w, n_ac))
    s0, s1, counts = embed_pair(frames, delta, n_ac, bits)
    assert tuple(counts) == (0, 0)
    assert np.array_equal(s0, s1)


@pytest.mark.parametrize("key", [None, KEY], ids=["raster", "keyed"])
def test_letterboxed_1080p_decodes_exactly(key):
    f, h, w, delta, n_ac = 2, 1080, 1920, 20, 10
    frames = frames_of("letterbox", f, h, w, seed=9)
    bits = payload(batch.capacity_bits(f, h, w, n_ac) * 3 // 4)
    s0, s1, counts = embed_pair(frames, delta, n_ac, bits, key=key)
    assert counts.repaired > 1000 and counts.unrepaired == 0

    def oracle_bits(stego):
        src = stego if key is None else order.permute_blocks(stego, key, 0)
        return orc.batch_extract_bits(src, delta, n_ac)[: bits.size]

    assert (oracle_bits(s0) != bits).sum() > 1000                     # the reference's stego does not deliver the payload
    assert np.array_equal(oracle_bits(s1), bits)                      # the flagged call's does, under the reference's extraction
    packed, n = batch.extract_frames(s1, delta, n_ac, block_key=key)  # and under the library's
    assert np.array_equal(np.unpackbits(packed, count=n)[: bits.size], bits)


def _letterbox_clip(tmp_path, n_frames, h, w):
    frames, secret, secret_path = _make_inputs(tmp_path, n_frames=n_frames, size=(h, w), secret=(12, 10), seed=31)
    bar = (h // 6) // 8 * 8
    for fr in frames:
        fr[:bar] = 0
        fr[h - bar:] = 0
    return frames, secret, secret_path


def test_drop_in_loop_stream_survives_with_readback(monkeypatch, tmp_path, capsys):
    """a svsdct.framing stream through embed_process with SVS_READBACK=1 into a letterboxed clip comes back bit for bit and
    its header parses; without the flag it comes back with bit errors"""
    emb, ext = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    _, secret, secret_path = _letterbox_clip(tmp_path, 6, 96, 160)
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    delta, n_ac = 20, 10
    made = []
    real = emb._siapkan_payload
    monkeypatch.setattr(emb, "_siapkan_payload", lambda *a: made.append(real(*a)) or made[-1])

    def stream_back(name):
        video = fakes.VIDEOS[str(tmp_path / (name + ".avi"))]["frames"]
        gray = np.stack([fr[..., 0] for fr in video])                  # COLOR_GRAY2BGR frames: B = G = R
        packed, n = batch.extract_frames(gray, delta, n_ac)
        return np.unpackbits(packed, count=n)[: made[-1].size]

    for flagged in (False, True):
        monkeypatch.setattr(emb, "READBACK", flagged)
        ok, _, _ = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / f"rb{int(flagged)}"), delta, n_ac,
                                                   pub)
        assert ok
        got = stream_back(f"rb{int(flagged)}")
        if flagged:
            assert np.array_equal(got, made[-1])
            header = framing.parse_header(got)
            assert (header.width, header.height) == (12, 10)
            assert "Read-back:" in capsys.readouterr().out
        else:
            assert (got != made[-1]).sum() > 0
