"""Read-back and repair under a coefficient selection and a keyed dither on the GPU (svs_embed_dithered_readback*): the
keyed body of readback_kernel equals the host build of the same arithmetic (csrc/svs_readback.hpp via tests/hostemu)
byte for byte with the same counts, starting from the bytes of the same call without read-back - dither off and on, raster and
keyed order, both embed rules, every quantiser mode, on frames whose waves straddle frames and end ragged - in place, on
pitched planes and over several staging chunks; without a selection and a dither the calls are svs_embed_readback*; and a
dithered, selected, keyed clip that the plain calls cannot deliver decodes exactly."""
import ctypes as C

import numpy as np
import pytest

import dither_lib
import fakes
import keyed_readback_lib as kl
import readback_lib as rl
from test_gpu_parity import _Dev
from test_pipeline import _install
from test_readback_gpu import _letterbox_clip
from svsdct import batch, native
from svsdct.native import Planes

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KEY = kl.DITHER_KEY
ORDER_KEY = 0xC0FFEE1234
# 3 x 56 x 136: 119 blocks per frame, 357 in all - two workgroups, a partial last wave (37 blocks), waves that straddle frames
F, H, W = 3, 56, 136
FIRST = 3
SETTINGS = ((20, kl.prefix(10)), (20, kl.zigzag(10)), (8, kl.zigzag(3, 6)), (4, kl.zigzag(3)), (20, kl.prefix(63)),
            (7.5, (9, 2, 17, 40, 63)), (0.1, kl.prefix(12)))
KINDS = ("letterbox", "bright", "flat0", "noise")          # flat0: 64 failing lanes per wave, two worklist rounds
# (dither, keyed order, rule), rotated over kind x setting so that each value of each occurs with each kind and setting class
VARIANTS = ((True, False, "reference"), (True, True, "minmove"), (False, True, "reference"), (False, False, "minmove"))


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def frames_of(kind, f, h, w, seed=1):
    return np.stack([rl.content(kind, h, w, seed=seed + k) for k in range(f)])


def _keywords(index, dither, keyed, rule, first):
    kw = dict(first_frame=first, minmove=rule == "minmove")
    if not kl.prefix(len(index)) == tuple(index):
        kw["coeffs"] = list(index)
    if dither:
        kw["dither_key"] = KEY
    if keyed:
        kw["block_key"] = ORDER_KEY
    return kw


def embed_pair(frames, delta, index, bits, dither, keyed, rule, first=FIRST, **more):
    """(the stego of the call without read-back, the new call's stego, its counts) through the host-pointer calls"""
    kw = dict(_keywords(index, dither, keyed, rule, first), **more)
    s0, used0 = batch.embed_frames(frames, delta, len(index), bits, **kw)
    s1, used1, counts = batch.embed_frames(frames, delta, len(index), bits, readback_keyed=True, **kw)
    assert used0 == used1
    return np.array(s0), np.array(s1), counts


def emulate(s0, delta, index, bits, dither, keyed, first=FIRST, **kw):
    return kl.host_readback(s0, delta, len(index), bits, index=index, dither_key=KEY if dither else None,
                            block_key=ORDER_KEY if keyed else None, first_frame=first, **kw)


CASES = [(kind, j, VARIANTS[(i + j) % 4]) for i, kind in enumerate(KINDS) for j in range(len(SETTINGS))]


def test_the_cases_cover_every_switch():
    for pos, values in enumerate(((False, True), (False, True), ("reference", "minmove"))):
        for value in values:
            got = [(kind, j) for kind, j, v in CASES if _variant(j, v)[pos] == value]
            assert {k for k, _ in got} == set(KINDS) and len({j for _, j in got}) >= 4, (pos, value)
    assert {j for _, j, _ in CASES} == set(range(len(SETTINGS)))


def _variant(j, v):
    """a prefix selection without a dither is svs_embed_readback itself (tested below): the prefix settings get the dither"""
    dither, keyed, rule = v
    return (True if SETTINGS[j][1] == kl.prefix(len(SETTINGS[j][1])) else dither), keyed, rule


@pytest.mark.parametrize("kind,j,v", CASES, ids=[f"{k}-{SETTINGS[j][0]}-{len(SETTINGS[j][1])}@{SETTINGS[j][1][0]}" for k, j, _ in CASES])
def test_gpu_equals_host_emulation(kind, j, v):
    delta, index = SETTINGS[j]
    dither, keyed, rule = _variant(j, v)
    frames = frames_of(kind, F, H, W)
    cap = batch.capacity_bits(F, H, W, len(index))
    bits = dither_lib.payload(cap - 37)
    s0, s1, counts = embed_pair(frames, delta, index, bits, dither, keyed, rule)
    want, want_counts, status = emulate(s0, delta, index, bits, dither, keyed)
    print(f"{kind}, delta {delta}, {len(index)} from {index[0]}, dither {dither}, keyed {keyed}, {rule}: "
          f"{int((status == 1).sum() + (status == 2).sum())} failing -> {want_counts[1]} left; GPU counts {tuple(counts)}")
    assert np.array_equal(s1, want), np.argwhere(s1 != want)[:4]
    assert tuple(counts) == want_counts


def _device_calls(frames, delta, index, stream, off, n_bits, dither, keyed, rule, first, pitched=False, preset=(5, 7)):
    """svs_embed_dithered_dev / svs_embed_select_dev in place, then the new device call in place from the cover, on tight or
    pitched planes with sentinels in the padding -> (stego without read-back, stego with, counts added to `preset`)"""
    lib = native.load()
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    view = lambda a: np.lib.stride_tricks.as_strided(a, (f, h, w), (frame_pitch, row_pitch, 1))   # noqa: E731
    view(host)[...] = frames
    pad = np.ones(host.size, bool)
    view(pad)[...] = False
    packed = batch.pack_bits(stream)
    d, d_bits, d_counts = _Dev(host.size), _Dev(packed.size + 8), _Dev(16)
    d_bits.put(packed)
    dith = native.Dither(KEY, first, 0) if dither else None
    odr = batch.block_order(ORDER_KEY if keyed else None, first)
    sel = native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    flags = batch.embed_flags(None, False, rule == "minmove")
    done = C.c_uint64(0)
    d.put(host)
    if dither:
        native.check(lib.svs_embed_dithered_dev(d.ptr, d.ptr, C.byref(planes), ref(odr), C.byref(sel), C.byref(dith), float(delta),
                                                len(index), d_bits.ptr, off, n_bits, flags, C.byref(done), None), "dithered")
    else:
        native.check(lib.svs_embed_select_dev(d.ptr, d.ptr, C.byref(planes), ref(odr), C.byref(sel), float(delta), d_bits.ptr,
                                              off, n_bits, flags, C.byref(done), None), "select")
    native.check(lib.svs_stream_synchronize(None), "sync")
    plain = d.get()
    d.put(host)
    d_counts.put(np.array(preset, np.uint64))
    native.check(lib.svs_embed_dithered_readback_dev(d.ptr, d.ptr, C.byref(planes), ref(odr), C.byref(sel), ref(dith),
                                                     float(delta), len(index), d_bits.ptr, off, n_bits, flags, C.byref(done),
                                                     d_counts.ptr, None), "svs_embed_dithered_readback_dev")
    native.check(lib.svs_stream_synchronize(None), "sync")
    out = d.get()
    assert (plain[pad] == 0xAB).all() and (out[pad] == 0xAB).all()          # sentinel padding is untouched
    assert done.value == n_bits
    return view(plain).copy(), view(out).copy(), tuple(int(c) for c in d_counts.get(16, np.uint64))


@pytest.mark.parametrize("dither,keyed", ((True, True), (False, False), (True, False)), ids=("dither-keyed", "select", "dither"))
def test_device_call_in_place_with_counts(dither, keyed):
    delta, index, off = 20, kl.zigzag(10), 45
    frames = frames_of("letterbox", F, H, W, seed=7)
    n_bits = batch.capacity_bits(F, H, W, 10) - 13
    stream = dither_lib.payload(off + n_bits + 50)
    s0, s1, counts = _device_calls(frames, delta, index, stream, off, n_bits, dither, keyed, "minmove", 2)
    want, want_counts, _ = emulate(s0, delta, index, stream, dither, keyed, first=2, bit_offset=off, n_bits=n_bits)
    assert want_counts[0] > 30
    assert np.array_equal(s1, want) and counts == (want_counts[0] + 5, want_counts[1] + 7)


def test_pitched_planes():
    delta, index, off = 8, kl.zigzag(3, 6), 45
    frames = frames_of("letterbox", F, H, W, seed=5)
    n_bits = batch.capacity_bits(F, H, W, 3) - 2
    stream = dither_lib.payload(off + n_bits)
    s0, s1, counts = _device_calls(frames, delta, index, stream, off, n_bits, True, True, "reference", FIRST, pitched=True)
    want, want_counts, _ = emulate(s0, delta, index, stream, True, True, bit_offset=off, n_bits=n_bits)
    assert want_counts[0] > 30
    assert np.array_equal(s1, want) and counts == (want_counts[0] + 5, want_counts[1] + 7)


@pytest.mark.parametrize("n_ac", (3, 10, 63))
def test_without_selection_and_dither_the_call_is_svs_embed_readback(n_ac):
    """all three NULL, and a prefix selection alone: svs_embed_readback_dev, byte for byte and count for count"""
    lib = native.load()
    delta = 20
    frames = frames_of("letterbox", F, H, W, seed=3)
    planes = Planes.contiguous(F, H, W)
    n_bits = batch.capacity_bits(F, H, W, n_ac) - 5
    packed = batch.pack_bits(dither_lib.payload(n_bits))
    d, d_bits, d_counts = _Dev(frames.nbytes), _Dev(packed.size + 8), _Dev(16)
    d_bits.put(packed)
    done = C.c_uint64(0)
    sel = native.Coeffs(n_ac, (C.c_uint8 * 63)(*range(1, n_ac + 1)))
    results = []
    for odr in (None, batch.block_order(ORDER_KEY, FIRST)):
        ref = C.byref(odr) if odr is not None else None
        for call in ("readback", "null", "prefix"):
            d.put(frames)
            d_counts.put(np.zeros(2, np.uint64))
            if call == "readback":
                rc = lib.svs_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), ref, float(delta), n_ac, d_bits.ptr, 0, n_bits,
                                                native.SVS_EXACT_GUARDED, C.byref(done), d_counts.ptr, None)
            else:
                rc = lib.svs_embed_dithered_readback_dev(d.ptr, d.ptr, C.byref(planes), ref, C.byref(sel) if call == "prefix" else None,
                                                         None, float(delta), 0 if call == "prefix" else n_ac, d_bits.ptr, 0, n_bits,
                                                         native.SVS_EXACT_GUARDED, C.byref(done), d_counts.ptr, None)
            native.check(rc, call)
            native.check(lib.svs_stream_synchronize(None), "sync")
            results.append((d.get(), tuple(int(c) for c in d_counts.get(16, np.uint64)), done.value))
        base = results[-3]
        assert sum(base[1]) > 30 and base[2] == n_bits
        for other in results[-2:]:
            assert np.array_equal(other[0], base[0]) and other[1:] == base[1:]


@pytest.mark.parametrize("kind", ("noise", "natural"))
def test_content_without_failures_is_byte_identical(kind):
    f, h, w, delta, index = 2, 240, 320, 20, kl.zigzag(10)
    frames = dither_lib.noise((f, h, w), 16, 240, seed=5) if kind == "noise" else frames_of("natural", f, h, w, seed=5)
    bits = dither_lib.payload(batch.capacity_bits(f, h, w, 10))
    s0, s1, counts = embed_pair(frames, delta, index, bits, True, False, "reference")
    assert tuple(counts) == (0, 0)
    assert np.array_equal(s0, s1)


def test_delivery_on_the_letterboxed_frame():
    """the 96 x 160 letterbox frame of the CPU table (t = 3; dither, block key, zig-zag 10, minimum move): svs_extract_dithered
    of the plain stego has wrong bits, of the new call's none"""
    delta, index = 20, kl.zigzag(10)
    frame = kl.table_frame("letterbox")[None]
    bits = dither_lib.payload(240 * 10 - 7)
    s0, s1, counts = embed_pair(frame, delta, index, bits, True, True, "minmove", first=kl.TABLE_T)

    def received(stego):
        packed, n = batch.extract_frames(stego, delta, 10, coeffs=list(index), dither_key=KEY, block_key=ORDER_KEY,
                                         first_frame=kl.TABLE_T)
        return np.unpackbits(packed, count=n)[: bits.size]

    wrong = int((received(s0) != bits).sum())
    print(f"wrong bits without read-back: {wrong}; counts with: {tuple(counts)}")
    assert wrong > 0
    assert counts.repaired > 0 and counts.unrepaired == 0
    assert np.array_equal(received(s1), bits)


def test_host_call_over_several_staging_chunks():
    """five letterboxed 1080p frames travel as whole frames in several chunks: each chunk's first frame feeds the order and the
    dither, the counts are summed"""
    f, h, w, delta, index, off = 5, 1080, 1920, 20, kl.zigzag(10), 77
    frames = frames_of("letterbox", f, h, w, seed=11)
    cap = batch.capacity_bits(f, h, w, 10)
    bits = dither_lib.payload(off + cap - 1234)
    s0, s1, counts = embed_pair(frames, delta, index, bits, True, True, "minmove", bit_offset=off)
    want, want_counts, _ = emulate(s0, delta, index, bits, True, True, bit_offset=off)
    assert want_counts[0] > 10000 and want_counts[1] == 0
    assert tuple(counts) == want_counts and np.array_equal(s1, want)


def test_drop_in_loop_delivers_with_the_keyed_readback(monkeypatch, tmp_path, capsys):
    """a framed payload through embed_process into a letterboxed clip with a dither, a zig-zag selection, a block key and the
    minimum-move rule: it comes back bit for bit with SVS_READBACK_KEYED=1 and with bit errors without it"""
    emb, _ = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    _, secret, secret_path = _letterbox_clip(tmp_path, 6, 96, 160)
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    delta, n_ac = 20, 10
    monkeypatch.setenv("SVS_DITHER_KEY", hex(KEY))
    monkeypatch.setenv("SVS_COEFFS", "zigzag")
    monkeypatch.setenv("SVS_BLOCK_KEY", hex(ORDER_KEY))
    monkeypatch.setenv("SVS_MINMOVE", "1")
    monkeypatch.setattr(emb, "MINMOVE", True)                             # the module reads its 0 / 1 switches at import
    for name in ("READBACK", "READBACK_COLOUR", "FUSED_COLOUR", "KEEP_COLOUR", "NEAREST"):
        monkeypatch.setattr(emb, name, False)
    made = []
    real = emb._siapkan_payload
    monkeypatch.setattr(emb, "_siapkan_payload", lambda *a: made.append(real(*a)) or made[-1])

    def stream_back(name):
        video = fakes.VIDEOS[str(tmp_path / (name + ".avi"))]["frames"]
        gray = np.stack([fr[..., 0] for fr in video])                  # COLOR_GRAY2BGR frames: B = G = R
        packed, n = batch.extract_frames(gray, delta, n_ac, coeffs="zigzag", dither_key=KEY, block_key=ORDER_KEY)
        return np.unpackbits(packed, count=n)[: made[-1].size]

    errors = {}
    for switched in (False, True):
        monkeypatch.setenv("SVS_READBACK_KEYED", "1" if switched else "0")
        monkeypatch.setattr(emb, "READBACK_KEYED", switched)
        ok, _, _ = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / f"krb{int(switched)}"), delta, n_ac, pub)
        assert ok
        out = capsys.readouterr().out
        assert ("Read-back:" in out) == switched
        if switched:
            assert "0 blok tidak dapat diperbaiki" in out
        errors[switched] = int((stream_back(f"krb{int(switched)}") != made[-1]).sum())
    print(f"payload bit errors without / with SVS_READBACK_KEYED: {errors[False]} / {errors[True]}")
    assert errors[False] > 0 and errors[True] == 0
