"""Read-back and repair under per-coefficient steps on the GPU (svs_stepped_embed_readback*): the stepped body of
readback_kernel equals the host build of the same arithmetic (csrc/svs_readback.hpp via tests/hostemu/stepped_readback_emu.cpp)
byte for byte with the same counts, starting from the bytes of svs_stepped_embed - uniform, matched and odd tables, dither off
and on, raster and keyed order, the three embed rules, on frames whose waves straddle frames and end ragged and whose flat-0
content fills two worklist rounds - in place, on pitched planes and over several staging chunks; a uniform table gives the
keyed read-back's bytes and counts; and a letterboxed clip that the plain stepped call cannot deliver decodes exactly."""
import ctypes as C

import numpy as np
import pytest

import dither_lib
import fakes
import keyed_readback_lib as kl
import stepped_lib as stl
import stepped_readback_lib as srl
from test_gpu_parity import _Dev
from test_pipeline import _install
from test_readback_gpu import _letterbox_clip
from svsdct import batch, native
from svsdct.native import Planes
from svsdct.pipeline import FramePipeline

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KEY = kl.DITHER_KEY
ORDER_KEY = srl.ORDER_KEY
# 3 x 56 x 136: 119 blocks per frame, 357 in all - two workgroups, a partial last wave (37 blocks), waves that straddle frames
F, H, W = srl.GPU_SHAPE
FIRST = srl.FIRST_FRAME


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _keywords(index, dither, keyed, rule, first):
    kw = dict(first_frame=first, nearest=rule == "nearest", minmove=rule == "minmove")
    if not kl.prefix(len(index)) == tuple(index):
        kw["coeffs"] = list(index)
    if dither:
        kw["dither_key"] = KEY
    if keyed:
        kw["block_key"] = ORDER_KEY
    return kw


def embed_pair(frames, table, index, bits, dither, keyed, rule, first=FIRST, **more):
    """(the stego of svs_stepped_embed, the new call's stego, its counts) through the host-pointer calls"""
    kw = dict(_keywords(index, dither, keyed, rule, first), steps=table, **more)
    s0, used0 = batch.embed_frames(frames, 1.0, len(index), bits, **kw)
    s1, used1, counts = batch.embed_frames(frames, 1.0, len(index), bits, readback_stepped=True, **kw)
    assert used0 == used1
    return np.array(s0), np.array(s1), counts


def emulate(s0, table, index, bits, dither, keyed, first=FIRST, **kw):
    return srl.host_readback(s0, table, len(index), bits, index=index, dither_key=KEY if dither else None,
                             block_key=ORDER_KEY if keyed else None, first_frame=first, **kw)


CASES = srl.gpu_cases()


def test_the_cases_cover_every_switch():
    assert {c[0] for c in CASES} == set(srl.TABLES) and {c[1] for c in CASES} == set(srl.CONTENTS)
    assert {c[2:] for c in CASES} == set(srl.OPTION_SETS)
    for pos, values in ((3, (False, True)), (4, (False, True)), (5, srl.RULES)):
        assert {c[pos] for c in CASES} == set(values)
    assert {len(c[2]) for c in CASES} == {3, 10, 63}


# ---- (a) device equals host emulation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname,kind,index,dither,keyed,rule", CASES,
                         ids=[f"{c[0]}-{c[1]}-{len(c[2])}@{c[2][0]}-{'d' if c[3] else 'p'}{'k' if c[4] else 'r'}-{c[5]}" for c in CASES])
def test_gpu_equals_host_emulation(tname, kind, index, dither, keyed, rule):
    table = srl.TABLES[tname]
    frames = srl.frames_of(kind)
    cap = batch.capacity_bits(F, H, W, len(index))
    bits = dither_lib.payload(cap - 37)
    s0, s1, counts = embed_pair(frames, table, index, bits, dither, keyed, rule)
    want, want_counts, status = emulate(s0, table, index, bits, dither, keyed)
    print(f"{tname}, {kind}, {len(index)} from {index[0]}, dither {dither}, keyed {keyed}, {rule}: "
          f"{int((status == 1).sum() + (status == 2).sum())} failing -> {want_counts[1]} left; GPU counts {tuple(counts)}")
    assert np.array_equal(s1, want), np.argwhere(s1 != want)[:4]
    assert tuple(counts) == want_counts


# ---- (b) the uniform identity on the device -------------------------------------------------------------------------------
def _dev_buffers(frames, stream):
    packed = batch.pack_bits(stream)
    d, d_bits, d_counts = _Dev(frames.nbytes), _Dev(packed.size + 8), _Dev(16)
    d_bits.put(packed)
    return d, d_bits, d_counts


def _ref(x):
    return C.byref(x) if x is not None else None


@pytest.mark.parametrize("keyed", (False, True), ids=("raster", "keyed"))
@pytest.mark.parametrize("d_uniform", (20, 16, 7))
def test_uniform_table_is_the_keyed_readback_call(d_uniform, keyed):
    """svs_stepped_embed_readback_dev with every delta[k] = D against svs_embed_dithered_readback_dev at delta = D: a zig-zag
    selection, a dither and the minimum-move rule, without and with an order; bytes, counts and *n_embedded"""
    lib = native.load()
    index = kl.zigzag(10)
    frames = srl.frames_of("letterbox")
    planes = Planes.contiguous(F, H, W)
    n_bits = batch.capacity_bits(F, H, W, 10) - 5
    d, d_bits, d_counts = _dev_buffers(frames, dither_lib.payload(n_bits))
    done = C.c_uint64(0)
    sel = native.Coeffs(10, (C.c_uint8 * 63)(*index))
    dith = native.Dither(KEY, FIRST, 0)
    odr = batch.block_order(ORDER_KEY, FIRST) if keyed else None
    table = batch._steps_arg(stl.uniform(d_uniform))
    flags = batch.embed_flags(None, False, True)
    results = []
    for call in ("keyed", "stepped"):
        d.put(frames)
        d_counts.put(np.zeros(2, np.uint64))
        if call == "keyed":
            rc = lib.svs_embed_dithered_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), C.byref(dith),
                                                     float(d_uniform), 10, d_bits.ptr, 0, n_bits, flags, C.byref(done), d_counts.ptr, None)
        else:
            rc = lib.svs_stepped_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), C.byref(dith),
                                                    C.byref(table), 10, d_bits.ptr, 0, n_bits, flags, C.byref(done), d_counts.ptr, None)
        native.check(rc, call)
        native.check(lib.svs_stream_synchronize(None), "sync")
        results.append((d.get(), tuple(int(c) for c in d_counts.get(16, np.uint64)), done.value))
    base, new = results
    assert sum(base[1]) > 30 and base[2] == n_bits
    assert np.array_equal(new[0], base[0]) and new[1:] == base[1:]


@pytest.mark.parametrize("n_ac", (3, 10, 63))
def test_uniform_table_without_selection_and_dither_is_svs_embed_readback(n_ac):
    lib = native.load()
    delta = 20
    frames = srl.frames_of("letterbox")
    planes = Planes.contiguous(F, H, W)
    n_bits = batch.capacity_bits(F, H, W, n_ac) - 5
    d, d_bits, d_counts = _dev_buffers(frames, dither_lib.payload(n_bits))
    done = C.c_uint64(0)
    table = batch._steps_arg(stl.uniform(delta))
    for odr in (None, batch.block_order(ORDER_KEY, FIRST)):
        results = []
        for call in ("readback", "stepped"):
            d.put(frames)
            d_counts.put(np.zeros(2, np.uint64))
            if call == "readback":
                rc = lib.svs_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), float(delta), n_ac, d_bits.ptr, 0, n_bits,
                                                native.SVS_EXACT_GUARDED, C.byref(done), d_counts.ptr, None)
            else:
                rc = lib.svs_stepped_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), None, None, C.byref(table), n_ac,
                                                        d_bits.ptr, 0, n_bits, native.SVS_EXACT_GUARDED | native.SVS_READBACK,
                                                        C.byref(done), d_counts.ptr, None)
            native.check(rc, call)
            native.check(lib.svs_stream_synchronize(None), "sync")
            results.append((d.get(), tuple(int(c) for c in d_counts.get(16, np.uint64)), done.value))
        base, new = results
        assert sum(base[1]) > 30 and base[2] == n_bits
        assert np.array_equal(new[0], base[0]) and new[1:] == base[1:]


# ---- (c) the _dev call in place and on pitched planes ---------------------------------------------------------------------
def _device_calls(frames, table, index, stream, off, n_bits, dither, keyed, rule, first, pitched=False, preset=(5, 7)):
    """svs_stepped_embed_dev in place, then the new device call in place from the cover, on tight or pitched planes with
    sentinels in the padding -> (stego without read-back, stego with, counts added to `preset`)"""
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
    steps = batch._steps_arg(table)
    flags = batch.embed_flags(None, rule == "nearest", rule == "minmove")
    done = C.c_uint64(0)
    d.put(host)
    native.check(lib.svs_stepped_embed_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), _ref(dith), C.byref(steps),
                                           len(index), d_bits.ptr, off, n_bits, flags, C.byref(done), None), "svs_stepped_embed_dev")
    native.check(lib.svs_stream_synchronize(None), "sync")
    plain = d.get()
    d.put(host)
    d_counts.put(np.array(preset, np.uint64))
    native.check(lib.svs_stepped_embed_readback_dev(d.ptr, d.ptr, C.byref(planes), _ref(odr), C.byref(sel), _ref(dith),
                                                    C.byref(steps), len(index), d_bits.ptr, off, n_bits, flags, C.byref(done),
                                                    d_counts.ptr, None), "svs_stepped_embed_readback_dev")
    native.check(lib.svs_stream_synchronize(None), "sync")
    out = d.get()
    assert (plain[pad] == 0xAB).all() and (out[pad] == 0xAB).all()          # sentinel padding is untouched
    assert done.value == n_bits
    return view(plain).copy(), view(out).copy(), tuple(int(c) for c in d_counts.get(16, np.uint64))


@pytest.mark.parametrize("pitched", (False, True), ids=("tight", "pitched"))
def test_device_call_in_place_with_counts(pitched):
    table, index, off = srl.TABLES["m75x2"], kl.zigzag(10), 45
    frames = srl.frames_of("letterbox")
    n_bits = batch.capacity_bits(F, H, W, 10) - 13
    stream = dither_lib.payload(off + n_bits + 50)
    s0, s1, counts = _device_calls(frames, table, index, stream, off, n_bits, True, True, "minmove", 2, pitched=pitched)
    want, want_counts, _ = emulate(s0, table, index, stream, True, True, first=2, bit_offset=off, n_bits=n_bits)
    assert want_counts[0] > 30
    assert np.array_equal(s1, want) and counts == (want_counts[0] + 5, want_counts[1] + 7)


# ---- (d) content without failures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("noise", "natural"))
def test_content_without_failures_is_byte_identical(kind):
    f, h, w, index = 2, 240, 320, kl.zigzag(10)
    frames = dither_lib.noise((f, h, w), 64, 192, seed=5) if kind == "noise" else srl.frames_of("natural", (f, h, w))
    bits = dither_lib.payload(batch.capacity_bits(f, h, w, 10))
    s0, s1, counts = embed_pair(frames, srl.TABLES["u20"], index, bits, True, False, "reference")
    assert tuple(counts) == (0, 0)
    assert np.array_equal(s0, s1)


# ---- (e) delivery ----------------------------------------------------------------------------------------------------------
def test_delivery_on_the_letterboxed_frame():
    """one 96 x 160 letterboxed frame, matched(75, 2), zig-zag 1..10, dither, block key, minimum-move rule - the issue's first
    setting: the host emulation leaves nothing unrepaired there (tests/test_stepped_readback_cpu.py
    test_the_delivery_setting_leaves_nothing_unrepaired), so none of the fall-back settings is used.  svs_stepped_extract of the
    plain stepped stego has wrong bits, of the new call's none"""
    table, index, rule = srl.DELIVERY
    frame = kl.table_frame("letterbox")[None]
    bits = dither_lib.payload(240 * 10 - 7)
    s0, s1, counts = embed_pair(frame, table, index, bits, True, True, rule, first=kl.TABLE_T)

    def received(stego):
        packed, n = batch.extract_frames(stego, 1.0, 10, coeffs=list(index), dither_key=KEY, block_key=ORDER_KEY,
                                         first_frame=kl.TABLE_T, steps=table)
        return np.unpackbits(packed, count=n)[: bits.size]

    wrong = int((received(s0) != bits).sum())
    print(f"wrong bits without read-back: {wrong}; counts with: {tuple(counts)}")
    assert wrong > 0
    assert counts.repaired > 0 and counts.unrepaired == 0
    assert np.array_equal(received(s1), bits)


# ---- (f) the host form over several staging chunks ------------------------------------------------------------------------
def test_host_call_over_several_staging_chunks():
    """five letterboxed 1080p frames travel as whole frames in several chunks: each chunk's first frame feeds the order and the
    dither, the counts are summed"""
    f, h, w, index, off = 5, 1080, 1920, kl.zigzag(10), 77
    table = srl.TABLES["m75x2"]
    frames = srl.frames_of("letterbox", (f, h, w))
    cap = batch.capacity_bits(f, h, w, 10)
    bits = dither_lib.payload(off + cap - 1234)
    s0, s1, counts = embed_pair(frames, table, index, bits, True, True, "minmove", bit_offset=off)
    want, want_counts, _ = emulate(s0, table, index, bits, True, True, bit_offset=off)
    assert want_counts[0] > 10000
    assert tuple(counts) == want_counts and np.array_equal(s1, want)


# ---- (g) FramePipeline and the drop-in loop -------------------------------------------------------------------------------
def test_frame_pipeline_with_the_stepped_readback():
    """two batches of two letterboxed frames through FramePipeline(steps=..., readback_stepped=True): the stego and the summed
    counts are those of batch.embed_frames over the four frames"""
    table, index = srl.TABLES["m75x2"], kl.zigzag(10)
    frames = srl.frames_of("letterbox", (4, 56, 136))
    bits = dither_lib.payload(batch.capacity_bits(4, 56, 136, 10) - 11)
    want, used, want_counts = batch.embed_frames(frames, 1.0, 10, bits, steps=table, coeffs=list(index), dither_key=KEY,
                                                 block_key=ORDER_KEY, first_frame=0, minmove=True, readback_stepped=True)
    want = np.array(want)
    with FramePipeline(56, 136, 2, 1.0, 10, depth=2, steps=table, coeffs=list(index), dither_key=KEY, block_key=ORDER_KEY,
                       minmove=True, readback_stepped=True) as pipe:
        pipe.set_payload(bits)
        got = []
        for k in range(2):
            pipe.input(k)[:] = frames[2 * k:2 * k + 2]
            pipe.submit_embed(k, 2, bit_offset=k * pipe.batch_capacity, first_frame=2 * k)
        for k in range(2):
            got.append(np.array(pipe.embed_result(k)))
        counts = pipe.readback_counts()
    assert want_counts.repaired > 30
    assert np.array_equal(np.concatenate(got), want) and tuple(counts) == tuple(want_counts)


def test_drop_in_loop_delivers_with_the_stepped_readback(monkeypatch, tmp_path, capsys):
    """a framed payload through embed_process into a letterboxed clip with SVS_STEPS=q75x2, a zig-zag selection, a dither, a
    block key and the minimum-move rule: it comes back bit for bit with SVS_READBACK_STEPPED=1 and with bit errors without it"""
    emb, _ = _install(monkeypatch, "gpu")
    monkeypatch.setattr(emb, "BATCH_FRAMES", 2)
    _, secret, secret_path = _letterbox_clip(tmp_path, 6, 96, 160)
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    n_ac = 10
    monkeypatch.setenv("SVS_STEPS", "q75x2")
    monkeypatch.setenv("SVS_DITHER_KEY", hex(KEY))
    monkeypatch.setenv("SVS_COEFFS", "zigzag")
    monkeypatch.setenv("SVS_BLOCK_KEY", hex(ORDER_KEY))
    monkeypatch.setenv("SVS_MINMOVE", "1")
    monkeypatch.setattr(emb, "MINMOVE", True)                             # the module reads its 0 / 1 switches at import
    for name in ("READBACK", "READBACK_COLOUR", "READBACK_KEYED", "FUSED_COLOUR", "KEEP_COLOUR", "NEAREST"):
        monkeypatch.setattr(emb, name, False)
    made = []
    real = emb._siapkan_payload
    monkeypatch.setattr(emb, "_siapkan_payload", lambda *a: made.append(real(*a)) or made[-1])

    def stream_back(name):
        video = fakes.VIDEOS[str(tmp_path / (name + ".avi"))]["frames"]
        gray = np.stack([fr[..., 0] for fr in video])                  # COLOR_GRAY2BGR frames: B = G = R
        packed, n = batch.extract_frames(gray, 1.0, n_ac, coeffs="zigzag", dither_key=KEY, block_key=ORDER_KEY,
                                         steps=stl.matched(75, 2))
        return np.unpackbits(packed, count=n)[: made[-1].size]

    errors = {}
    for switched in (False, True):
        monkeypatch.setenv("SVS_READBACK_STEPPED", "1" if switched else "0")
        monkeypatch.setattr(emb, "READBACK_STEPPED", switched)
        ok, _, _ = emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / f"srb{int(switched)}"), 20, n_ac, pub)
        assert ok
        out = capsys.readouterr().out
        assert ("Read-back:" in out) == switched
        if switched:
            assert "0 blok tidak dapat diperbaiki" in out
        errors[switched] = int((stream_back(f"srb{int(switched)}") != made[-1]).sum())
    print(f"payload bit errors without / with SVS_READBACK_STEPPED: {errors[False]} / {errors[True]}")
    assert errors[False] > 0 and errors[True] == 0
