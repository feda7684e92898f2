"""Read-back and repair for the fused colour embed on the GPU (svs_embed_bgr_readback*): the kernel's bytes and counts equal
the model of tests/colour_readback_lib.py - plain and keep colour, both weight tables, the content classes, every mode, a
budget ending inside a block and a frame, a bit offset, partial waves and several workgroups - the device call pitched and in
place, the host call over several staging chunks, the plain form against the three existing calls, a letterboxed 1080p clip
that decodes only with read-back, and the drop-in loop end to end."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import fakes
from colour_readback_lib import KINDS, SETTINGS, W14, W15, colour_content, colour_frames, model
from readback_lib import content, host_readback, payload
from test_gpu_parity import _Dev
from test_keep_colour_cpu import gray_of
from test_pipeline import _install, _make_inputs
from svsdct import batch, native
from svsdct.native import Planes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _run(cover, delta, n_ac, bits, weights, keep, mode=None, **kw):
    w = None if weights is W15 else np.array(weights, np.uint32)
    return batch.embed_bgr_frames(cover, delta, n_ac, bits, weights=w, keep_colour=keep, mode=mode, readback=True, **kw)


@pytest.mark.parametrize("weights", [W15, W14], ids=["15-bit", "14-bit"])
@pytest.mark.parametrize("delta,n_ac", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_equals_model(kind, delta, n_ac, weights):
    """3 x 40 x 136 frames: 17 blocks per row, 255 blocks - a partial last wave and, with the bit offset and a budget that
    ends inside the last frame and inside a block, waves that straddle rows, frames and the end of the payload"""
    f, h, w, off = 3, 40, 136, 37
    cover = colour_frames(kind, f, h, w, seed=5)
    cap = batch.capacity_bits(f, h, w, n_ac)
    bits = payload(off + cap - cap // 7 - 1)
    for keep in (False, True):
        for mode in ("guarded", "exact"):
            out, gray, used, counts = _run(cover, delta, n_ac, bits, weights, keep, mode=mode, bit_offset=off)
            want, planes, want_counts, _, _ = model(cover, delta, n_ac, bits, weights, keep, bit_offset=off)
            assert used == bits.size - off
            assert tuple(counts) == want_counts, (keep, mode)
            assert np.array_equal(np.array(out), want), (keep, mode, int((np.array(out) != want).any(axis=-1).sum()))
            assert np.array_equal(np.array(gray), gray_of(cover, weights))              # the gray reference stays the cover's


def test_several_workgroups_and_plain_equals_the_three_calls():
    """2 x 240 x 320 letterboxed frames (2 400 blocks: ten workgroups): kernel = model, and the plain form equals
    gray_to_bgr(embed_readback(bgr_to_gray(cover))) through the existing calls, whose gray read-back still gives the host
    build's bytes"""
    from svsdct import colour
    f, h, w, delta, n_ac = 2, 240, 320, 20, 10
    cover = colour_frames("letterbox", f, h, w, seed=2)
    bits = payload(batch.capacity_bits(f, h, w, n_ac) - 1234)
    gray = colour.device_gray(cover)
    assert np.array_equal(gray, gray_of(cover, W15))
    s0, _ = batch.embed_frames(gray, delta, n_ac, bits)
    s1, _, gray_counts = batch.embed_frames(gray, delta, n_ac, bits, readback=True)
    want_planes, want_counts, _ = host_readback(np.array(s0), delta, n_ac, bits)
    assert np.array_equal(np.array(s1), want_planes) and tuple(gray_counts) == want_counts     # the gray pass: today's bytes
    assert want_counts[0] > 300
    for keep in (False, True):
        out, _, _, counts = _run(cover, delta, n_ac, bits, W15, keep)
        want, planes, model_counts, _, _ = model(cover, delta, n_ac, bits, W15, keep)
        assert tuple(counts) == model_counts == want_counts
        assert np.array_equal(np.array(out), want), keep
        assert np.array_equal(planes, want_planes)
        if not keep:
            assert np.array_equal(np.array(out), np.repeat(np.array(s1)[..., None], 3, axis=-1))


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_device_call_pitched_in_place_with_counts(keep):
    lib = native.load()
    f, h, w, delta, n_ac, off = 3, 64, 128, 16, 10, 45
    cover = colour_frames("letterbox", f, h, w, seed=7)
    cap = batch.capacity_bits(f, h, w, n_ac)
    bits = payload(off + cap)
    packed = batch.pack_bits(bits)
    d_bits, d_counts = _Dev(packed.nbytes + 8), _Dev(16)
    d_bits.put(packed)
    rp = 3 * w + 24
    fp = rp * h + 64
    src = np.full(f * fp, 0xA5, np.uint8)
    for k in range(f):
        for y in range(h):
            src[k * fp + y * rp: k * fp + y * rp + 3 * w] = cover[k, y].reshape(-1)
    d = _Dev(src.size)
    d.put(src)
    d_counts.put(np.array([5, 7], np.uint64))                                     # the call adds into the buffer
    planes = Planes.contiguous(f, h, w)
    used = batch.embed_bgr_device(d.ptr.value, d.ptr.value, 0, planes, delta, n_ac, d_bits.ptr.value, off, cap,
                                  in_pitches=(rp, fp), out_pitches=(rp, fp), keep_colour=keep, readback=True,
                                  d_counts=d_counts.ptr.value)
    native.check(lib.svs_stream_synchronize(None), "sync")
    assert used == cap
    want, _, want_counts, _, _ = model(cover, delta, n_ac, bits, W15, keep, bit_offset=off, n_bits=cap)
    assert want_counts[0] > 50
    got = d.get()
    for k in range(f):
        for y in range(h):
            a = k * fp + y * rp
            assert np.array_equal(got[a: a + 3 * w], want[k, y].reshape(-1)), (k, y)
            assert (got[a + 3 * w: a + rp] == 0xA5).all()                         # sentinels in the padding
        assert (got[k * fp + h * rp: (k + 1) * fp] == 0xA5).all()
    assert tuple(int(c) for c in d_counts.get(16, np.uint64)) == (want_counts[0] + 5, want_counts[1] + 7)


def test_host_call_over_several_staging_chunks():
    """two 4K frames (50 MB of BGR; csrc/svs_stage.hpp moves a batch in chunks of at most SVS_STAGE_CHUNK_BYTES = 8 MB, so
    the host call travels as seven or more bands of block rows) against the device call on the whole batch resident in
    device memory - one launch, no staging - and the counts against the host build of the gray pass"""
    lib = native.load()
    f, h, w, delta, n_ac, off = 2, 2160, 3840, 20, 10, 77
    cover = np.stack([colour_content("letterbox", h, w, seed=11 + k) for k in range(f)])
    cap = batch.capacity_bits(f, h, w, n_ac)
    bits = payload(off + cap - 4321)
    out, _, used, counts = _run(cover, delta, n_ac, bits, W15, True, bit_offset=off)
    assert used == bits.size - off
    packed = batch.pack_bits(bits)
    d, d_bits, d_counts = _Dev(cover.nbytes), _Dev(packed.nbytes + 8), _Dev(16)
    d.put(cover.reshape(-1))
    d_bits.put(packed)
    d_counts.put(np.zeros(2, np.uint64))
    assert batch.embed_bgr_device(d.ptr.value, d.ptr.value, 0, Planes.contiguous(f, h, w), delta, n_ac, d_bits.ptr.value, off,
                                  bits.size - off, keep_colour=True, readback=True, d_counts=d_counts.ptr.value) == used
    native.check(lib.svs_stream_synchronize(None), "sync")
    assert np.array_equal(np.array(out).reshape(-1), d.get())
    one = tuple(int(x) for x in d_counts.get(16, np.uint64))
    assert tuple(counts) == one and counts.repaired > 10000
    s0, _ = batch.embed_frames(gray_of(cover, W15), delta, n_ac, bits, bit_offset=off)
    _, want_counts, _ = host_readback(np.array(s0), delta, n_ac, bits, bit_offset=off)
    assert tuple(counts) == want_counts


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_content_without_failures_is_byte_identical(keep):
    f, h, w, delta, n_ac = 2, 1080, 1920, 8, 3
    cover = colour_frames("noise", f, h, w, seed=5)
    bits = payload(batch.capacity_bits(f, h, w, n_ac))
    base, _, _ = batch.embed_bgr_frames(cover, delta, n_ac, bits, keep_colour=keep)
    out, _, _, counts = _run(cover, delta, n_ac, bits, W15, keep)
    assert tuple(counts) == (0, 0)
    assert np.array_equal(np.array(out), np.array(base))


def test_letterboxed_1080p_keep_colour_decodes_only_with_read_back():
    f, h, w, delta, n_ac = 2, 1080, 1920, 20, 10
    cover = colour_frames("letterbox", f, h, w, seed=9)
    bits = payload(batch.capacity_bits(f, h, w, n_ac) * 3 // 4)

    def errors(bgr):
        packed, n = batch.extract_bgr_frames(np.array(bgr), delta, n_ac)
        return int((np.unpackbits(packed, count=n)[: bits.size] != bits).sum())

    base, _, _ = batch.embed_bgr_frames(cover, delta, n_ac, bits, keep_colour=True)
    out, _, _, counts = _run(cover, delta, n_ac, bits, W15, True)
    assert errors(base) > 1000                                        # the call without read-back does not deliver the payload
    assert counts.repaired > 1000 and counts.unrepaired == 0
    assert errors(out) == 0
    inner = np.array(out)[:, 200:-200]
    assert (inner[..., 0] != inner[..., 1]).mean() > 0.5             # and the frames kept their colours


def test_drop_in_loop_recovers_the_secret_in_colour(monkeypatch, tmp_path, capsys):
    """SVS_READBACK_COLOUR=1 SVS_KEEP_COLOUR=1 on a letterboxed colour clip: the receiver recovers the secret image, the frames
    that carry payload stay coloured; without the switch the same clip does not decode"""
    emb, ext = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    h, w = 96, 160
    frames, secret, secret_path = _make_inputs(tmp_path, n_frames=6, size=(h, w), secret=(12, 10), seed=31)
    bar = (h // 6) // 8 * 8
    for fr in frames:
        fr[:bar] = 0
        fr[h - bar:] = 0
    receiver = fakes.FakeKey(b"bob")
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(receiver.public())
    delta, n_ac = 20, 10
    monkeypatch.setattr(emb, "KEEP_COLOUR", True)
    for on in (False, True):
        monkeypatch.setattr(emb, "READBACK_COLOUR", on)
        capsys.readouterr()
        ok, _, _ = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / f"c{int(on)}"), delta, n_ac, pub)
        assert ok
        said = capsys.readouterr().out
        out_png = str(tmp_path / f"o{int(on)}.png")
        got = ext.ekstraksi_gambar_video_final(str(tmp_path / f"c{int(on)}.avi"), out_png, delta, n_ac, receiver)
        if on:
            assert "Read-back:" in said and " 0 blok tidak dapat diperbaiki" in said
            assert got and np.array_equal(np.asarray(Image.open(out_png)), secret)
            video = fakes.VIDEOS[str(tmp_path / "c1.avi")]["frames"]
            first = video[0][bar: h - bar]
            assert (first[..., 0] != first[..., 1]).mean() > 0.5
        else:
            assert "Read-back:" not in said
            assert not got
