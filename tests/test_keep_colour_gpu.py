"""SVS_KEEP_COLOUR, GPU tier: the fused colour embed with the cover's colours kept.  The kernel's output must be the rule of
csrc/svs_colour.hpp (as restated in NumPy by test_keep_colour_cpu.keep_colour_rule) applied to (cover, stego gray of the
default call), byte for byte, in every kernel family; its gray must be the stego plane, so extraction gives the payload; and
the drop-in video loop must use it only behind the cv2 check, with the first-frame return values still gray planes."""
import ctypes as C
import sys

import numpy as np
import pytest
from PIL import Image

import fakes
from test_keep_colour_cpu import TABLES, gray_of, keep_colour_rule
from test_gpu_parity import _Dev
from test_pipeline import _install, _make_inputs
from svsdct import batch, native, synth
from svsdct.native import Planes

pytestmark = pytest.mark.gpu
W15, W14 = TABLES["15-bit"], TABLES["14-bit"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def colour_cover(f, h, w, seed):
    """Noise, flat blocks of saturated colours (pure B / G / R, white, black, yellow, cyan, magenta), saturated colours with
    a little noise, and flat blocks of random colours: clipping of c + d is common."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    palette = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [0, 255, 255],
                        [255, 255, 0], [255, 0, 255], [250, 3, 252]], np.uint8)
    by, bx = h // 8, w // 8
    kind = rng.integers(0, 4, (f, by, bx))
    for k in range(f):
        for i in range(by):
            for j in range(bx):
                blk = x[k, 8 * i: 8 * i + 8, 8 * j: 8 * j + 8]
                if kind[k, i, j] == 1:
                    blk[:] = palette[rng.integers(len(palette))]
                elif kind[k, i, j] == 2:
                    noisy = palette[rng.integers(len(palette))].astype(np.int16) + rng.integers(-6, 7, (8, 8, 3))
                    blk[:] = np.clip(noisy, 0, 255)
                elif kind[k, i, j] == 3:
                    blk[:] = rng.integers(0, 256, 3)
    return x


def _keep_vs_default(cover, delta, n_ac, payload, mode=None, weights=None):
    plain, gray, used = batch.embed_bgr_frames(cover, delta, n_ac, payload, mode=mode, weights=weights)
    kept, gray_k, used_k = batch.embed_bgr_frames(cover, delta, n_ac, payload, mode=mode, weights=weights, keep_colour=True)
    assert used_k == used and np.array_equal(gray_k, gray)          # the gray reference is the cover's in both forms
    return plain, kept, used


@pytest.mark.parametrize("n_ac", [3, 10, 20])
def test_kernel_equals_the_rule(n_ac):
    """Every kernel family (one-row and two-row streaming, exact), every mode, small and large steps, a budget ending inside
    a block, delta <= 0 with a payload (every block round-trips): the output is keep_colour_rule(cover, stego gray)."""
    f, h, w = 2, 48, 88                                              # 11 blocks per row: waves straddle block rows and frames
    cover = colour_cover(f, h, w, seed=n_ac)
    cap = batch.capacity_bits(f, h, w, n_ac)
    clipped = 0
    for mode in ("fast", "guarded", "exact"):
        for delta in (0.3, 8, 20, 64):
            payload = synth.synthetic_bits(cap - 5, seed=int(delta * 10) + n_ac)   # the budget ends inside a block
            plain, kept, used = _keep_vs_default(cover, delta, n_ac, payload, mode=mode)
            assert used == payload.size
            t = plain[..., 0]
            assert np.array_equal(plain, np.repeat(t[..., None], 3, axis=3))
            want = keep_colour_rule(cover, t, W15)
            assert np.array_equal(kept, want), (mode, delta, int((kept != want).any(axis=-1).sum()))
            assert np.array_equal(gray_of(kept, W15), t)
            shifted = cover.astype(int) + (t.astype(int) - gray_of(cover, W15))[..., None]
            clipped += int(((shifted < 0) | (shifted > 255)).any(axis=-1).sum())
        plain, kept, used = _keep_vs_default(cover, 0.0, n_ac, np.ones(40, np.uint8), mode=mode)   # delta <= 0
        assert used == 0
        assert np.array_equal(kept, keep_colour_rule(cover, plain[..., 0], W15))
    assert clipped > 1000                                            # the exact rule's path was exercised
    # the 14-bit table
    payload = synth.synthetic_bits(cap // 2 + 3, seed=n_ac)
    plain, kept, used = _keep_vs_default(cover, 8, n_ac, payload, weights=np.array(W14, np.uint32))
    assert np.array_equal(kept, keep_colour_rule(cover, plain[..., 0], W14))
    assert np.array_equal(gray_of(kept, W14), plain[..., 0])


@pytest.mark.parametrize("n_ac,delta", [(3, 8), (10, 20), (20, 8)])
def test_round_trip_and_cover_past_the_budget(n_ac, delta):
    """The device BGR -> gray of the output is the default call's stego plane, extraction straight from the output gives the
    default output's bits (the embedded bits wherever the reference's own round trip keeps them: saturated blocks lose some
    in both forms), and every block past the payload budget is the cover's bytes exactly."""
    from svsdct import colour
    f, h, w = 3, 64, 96
    cover = colour_cover(f, h, w, seed=100 + n_ac)
    cap = batch.capacity_bits(f, h, w, n_ac)
    payload = synth.synthetic_bits(cap // 2 + 7, seed=n_ac)
    plain, kept, used = _keep_vs_default(cover, delta, n_ac, payload)
    assert used == payload.size
    assert np.array_equal(colour.device_gray(kept), plain[..., 0])
    packed, n_bits = batch.extract_bgr_frames(kept, delta, n_ac)
    want_packed, _ = batch.extract_bgr_frames(plain, delta, n_ac)
    assert n_bits == cap and np.array_equal(packed, want_packed)
    assert (np.unpackbits(packed, count=used) == payload).mean() > 0.9
    blocks = kept.reshape(f, h // 8, 8, w // 8, 8, 3).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 8, 8, 3)
    cover_blocks = cover.reshape(f, h // 8, 8, w // 8, 8, 3).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 8, 8, 3)
    first_free = -(-used // n_ac)                                   # blocks carry n_ac bits each, in raster order
    assert np.array_equal(blocks[first_free:], cover_blocks[first_free:])
    assert not np.array_equal(blocks[:first_free], cover_blocks[:first_free])
    # colour is kept: the payload blocks are not gray
    assert (kept[..., 0] != kept[..., 1]).mean() > 0.5


def test_pitched_in_place_and_host_calls():
    """Pitched buffers leave their padding untouched; bgr_in == bgr_out gives the same pixels; the host-pointer call, which
    moves 1080p frames in bands and 640 x 480 frames in groups, equals the rule on its own default output."""
    lib = native.load()
    f, h, w, n_ac, delta = 3, 24, 88, 10, 12
    cover = colour_cover(f, h, w, seed=5)
    payload = synth.synthetic_bits(batch.capacity_bits(f, h, w, n_ac) - 5, seed=9)
    plain, want, used = _keep_vs_default(cover, delta, n_ac, payload)
    packed = batch.pack_bits(payload)
    d_bits = _Dev(packed.size)
    d_bits.put(packed)
    irp, orp = 3 * w + 24, 3 * w + 8
    ifp, ofp = irp * h + 64, orp * (h + 2)
    src = np.full(f * ifp, 0xA5, np.uint8)
    for k in range(f):
        for y in range(h):
            src[k * ifp + y * irp: k * ifp + y * irp + 3 * w] = cover[k, y].reshape(-1)
    d_in, d_out = _Dev(src.size), _Dev(f * ofp)
    d_in.put(src)
    d_out.put(np.full(f * ofp, 0x5A, np.uint8))
    planes = Planes.contiguous(f, h, w)
    assert batch.embed_bgr_device(d_in.ptr.value, d_out.ptr.value, 0, planes, delta, n_ac, d_bits.ptr.value, 0, payload.size,
                                  in_pitches=(irp, ifp), out_pitches=(orp, ofp), keep_colour=True) == used
    native.check(lib.svs_stream_synchronize(None), "sync")
    out, mask = d_out.get(), np.ones(f * ofp, bool)
    for k in range(f):
        for y in range(h):
            a = k * ofp + y * orp
            assert np.array_equal(out[a: a + 3 * w], want[k, y].reshape(-1)), (k, y)
            mask[a: a + 3 * w] = False
    assert (out[mask] == 0x5A).all()
    assert np.array_equal(d_in.get(), src)                          # the input is only read
    # in place, pitched: the frames become the keep-colour output, the padding stays
    assert batch.embed_bgr_device(d_in.ptr.value, d_in.ptr.value, 0, planes, delta, n_ac, d_bits.ptr.value, 0, payload.size,
                                  in_pitches=(irp, ifp), out_pitches=(irp, ifp), keep_colour=True) == used
    native.check(lib.svs_stream_synchronize(None), "sync")
    got = d_in.get()
    for k in range(f):
        for y in range(h):
            a = k * ifp + y * irp
            assert np.array_equal(got[a: a + 3 * w], want[k, y].reshape(-1)), ("in place", k, y)
            assert (got[a + 3 * w: a + irp] == 0xA5).all()
    # the host-pointer call in bands (1080p) and frame groups (640 x 480)
    rng = np.random.default_rng(23)
    for (f, h, w, n_ac, delta) in ((3, 1080, 1920, 10, 20), (12, 480, 640, 3, 8)):
        cover = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
        cover[:, : h // 4] = cover[:, : h // 4] // 64 * 85                      # saturated band: clipping everywhere
        cap = batch.capacity_bits(f, h, w, n_ac)
        payload = synth.synthetic_bits(cap - cap // (2 * f) - 3, seed=f)
        plain, kept, used = _keep_vs_default(cover, delta, n_ac, payload)
        assert used == payload.size
        assert np.array_equal(kept, keep_colour_rule(cover, plain[..., 0], W15)), (f, h, w)


def test_flag_rejected_elsewhere():
    """SVS_KEEP_COLOUR is an option of the fused colour embed only; the gray-plane entry points reject it (svs_extract_bgr_dev
    has no flags word)."""
    lib = native.load()
    planes = Planes.contiguous(1, 8, 8)
    d = _Dev(4096)
    k = native.SVS_KEEP_COLOUR
    got = C.c_uint64(0)
    assert lib.svs_embed_dev(d.ptr, d.ptr, C.byref(planes), 8.0, 3, d.ptr, 0, 8, k, None, None) == native.SVS_ERR_INVALID_ARG
    assert lib.svs_extract_dev(d.ptr, C.byref(planes), 8.0, 3, d.ptr, 64, k, C.byref(got), None) == native.SVS_ERR_INVALID_ARG
    host = np.zeros(64, np.uint8)
    assert lib.svs_embed(host.ctypes.data, host.ctypes.data, C.byref(planes), 8.0, 3, host.ctypes.data, 0, 8, k, None) == \
        native.SVS_ERR_INVALID_ARG
    assert lib.svs_extract(host.ctypes.data, C.byref(planes), 8.0, 3, host.ctypes.data, 64, k, C.byref(got)) == \
        native.SVS_ERR_INVALID_ARG
    # accepted by both colour embed calls, alone and with a mode bit
    bgr = np.zeros((1, 8, 8, 3), np.uint8)
    for mode in (None, "exact"):
        out, _, used = batch.embed_bgr_frames(bgr, 8, 3, np.ones(3, np.uint8), mode=mode, keep_colour=True)
        assert used == 3
    assert lib.svs_embed_bgr_dev(d.ptr, 24, 192, d.ptr, 24, 192, None, C.byref(planes), None, 8.0, 3, d.ptr, 0, 8,
                                 k | 4, None, None) == native.SVS_ERR_INVALID_ARG     # other unknown bits still are not


def test_drop_in_loop_keeps_colour(monkeypatch, tmp_path, capsys):
    """SVS_KEEP_COLOUR=1 in the drop-in embed loop (fakes.py stands in for cv2): payload frames keep colour, their BGR2GRAY is
    the default run's stego frame, later frames are the cover's, the first-frame return values are the gray pair; the
    receiver recovers the secret image with and without the fused extraction.  A cv2 that matches no table gives the
    default output and says so."""
    emb, ext = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 3)
    frames, secret, secret_path = _make_inputs(tmp_path, n_frames=9, size=(40, 56), secret=(12, 10), seed=21)
    receiver = fakes.FakeKey(b"bob")
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(receiver.public())
    delta, n_ac = 16, 12
    monkeypatch.setattr(emb.os, "urandom", lambda n: bytes(range(n)))       # same salt and ephemeral key in every run
    monkeypatch.setattr(emb, "buat_pasangan_kunci_ecc", lambda: (fakes.FakeKey(b"eph"), fakes.FakeKey(b"eph").public()))
    ok, g_host, s_host = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "host"), delta, n_ac, pub)
    assert ok
    host = fakes.VIDEOS[str(tmp_path / "host.avi")]["frames"]
    cv2 = sys.modules["cv2"]
    monkeypatch.setattr(emb, "KEEP_COLOUR", True)
    capsys.readouterr()
    ok, g0, s0 = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "keep"), delta, n_ac, pub)
    assert ok and "warna video sampul dipertahankan" in capsys.readouterr().out
    kept = fakes.VIDEOS[str(tmp_path / "keep.avi")]["frames"]
    assert len(kept) == len(host) == 9
    carrying = [k for k in range(9) if not np.array_equal(host[k], frames[k][:40, :56])]
    assert 2 <= len(carrying) < 9 and carrying == list(range(len(carrying)))
    for k in range(9):
        if k in carrying:
            assert np.array_equal(cv2.cvtColor(kept[k], cv2.COLOR_BGR2GRAY), host[k][..., 0]), k
            assert (kept[k][..., 0] != kept[k][..., 1]).mean() > 0.5, k       # colour content stays colour
        else:
            assert np.array_equal(kept[k], host[k]) and np.array_equal(kept[k], frames[k][:40, :56]), k
    assert g0.shape == s0.shape == (40, 56)
    assert np.array_equal(g0, g_host) and np.array_equal(s0, s_host)
    for fused in (False, True):
        monkeypatch.setattr(ext, "FUSED_COLOUR", fused)
        out_png = str(tmp_path / f"o{int(fused)}.png")
        assert ext.ekstraksi_gambar_video_final(str(tmp_path / "keep.avi"), out_png, delta, n_ac, receiver)
        assert np.array_equal(np.asarray(Image.open(out_png)), secret)

    # an OpenCV whose conversion matches no table: today's output, and the reason on the console
    odd = fakes.make_fake_cv2()
    plain = odd.cvtColor
    odd.cvtColor = lambda img, code: (plain(img, code) ^ 1) if code == odd.COLOR_BGR2GRAY else plain(img, code)
    monkeypatch.setitem(sys.modules, "cv2", odd)
    capsys.readouterr()
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "odd"), delta, n_ac, pub)[0]
    said = capsys.readouterr().out
    assert "jalur warna terfusi tidak dipakai" in said and "tidak dipertahankan" in said
    oddv = fakes.VIDEOS[str(tmp_path / "odd.avi")]["frames"]
    assert len(oddv) == 9
    for k in range(9):
        if k in carrying:
            assert (oddv[k][..., 0] == oddv[k][..., 1]).all() and (oddv[k][..., 1] == oddv[k][..., 2]).all(), k
        else:
            assert np.array_equal(oddv[k], frames[k][:40, :56]), k
