"""CPU tier of the payload coefficient selection (include/svsdct.h svs_coeffs): the restatement is pinned to the oracle, the
host build of the selected block bodies to the restatement, and the library's validation, routing and Python layer are
checked without a GPU.  tests/test_coeff_select_gpu.py runs the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coeff_select_lib as cs
from oracle import qim_dct_oracle as orc
from svsdct import batch, coeffs, native, pipeline
from testlib import REPO

COPY, ROUND_TRIP, EXACT, STREAMING = 0, 1, 2, 3          # svs::EmbedPath
X_ZEROS, X_EXACT, X_FAST = 0, 1, 2                       # svs::ExtractPath
INVALID = native.SVS_ERR_INVALID_ARG


# ---- the restatement is the oracle with one lookup changed -------------------------------------------------------------
@pytest.mark.parametrize("delta", cs.DELTAS + (0,))
@pytest.mark.parametrize("n", (0, 1, 3, 10, 63))
def test_restatement_with_a_prefix_is_the_oracle(delta, n):
    gray = cs.content("clip", h=32, w=48)[0]
    bits = cs.payload(6 * n * 24 // 7 + 5)               # ends inside a block for n > 1
    want = orc.frame_embed(gray, delta, bits, n)
    got = cs.select_embed(gray, delta, bits, cs.prefix(n))
    assert got[2] == want[2] and np.array_equal(got[1], want[1])
    assert np.array_equal(cs.select_extract_bits(want[1], delta, cs.prefix(n)), orc.frame_extract_bits(want[1], delta, n))
    assert np.array_equal(cs.select_embed(gray, delta, np.zeros(0, np.uint8), cs.prefix(n))[1], gray)


@pytest.mark.parametrize("delta", (8, 7.3, 0))
def test_loop_form_with_a_prefix_is_the_oracles_loops_and_equals_the_restatement(delta):
    gray = cs.content("clip", h=16, w=24, seed=4)[0]
    bits = cs.payload(40)
    want = orc.frame_operator_loops(gray, "embed", delta, bits, 7)
    got = cs.select_loops(gray, "embed", delta, bits, cs.prefix(7))
    assert got[2] == want[2] and np.array_equal(got[1], want[1])
    assert orc.bits_to_str(cs.select_loops(want[1], "extract", delta, None, cs.prefix(7))) == \
        orc.frame_operator_loops(want[1], "extract", delta, None, 7)
    for index in (cs.zigzag(7), cs.zigzag(7, 6), cs.scattered(7), cs.reversed_list(7)):
        loops = cs.select_loops(gray, "embed", delta, bits, index)
        vec = cs.select_embed(gray, delta, bits, index)
        assert loops[2] == vec[2] and np.array_equal(loops[1], vec[1]), index
        assert np.array_equal(cs.select_loops(vec[1], "extract", delta, None, index), cs.select_extract_bits(vec[1], delta, index))


def test_literal_zigzag_table_is_a_scan():
    assert sorted(cs.ZIGZAG) == list(range(64)) and cs.ZIGZAG[:8] == [0, 1, 8, 16, 9, 2, 3, 10] and cs.ZIGZAG[-1] == 63
    rows, cols = np.divmod(np.array(cs.ZIGZAG), 8)
    assert np.all(np.diff(rows + cols) >= 0)             # anti-diagonal by anti-diagonal
    assert list(coeffs.ZIGZAG) == cs.ZIGZAG


# ---- the host build of the selected bodies against the restatement ---------------------------------------------------------
@pytest.mark.parametrize("delta", cs.DELTAS)
@pytest.mark.parametrize("count", cs.COUNTS)
@pytest.mark.parametrize("kind", sorted(cs.KINDS))
def test_host_bodies_equal_the_restatement(delta, count, kind):
    index = cs.KINDS[kind](count)
    frames = cs.content("noise", f=2, h=32, w=48, seed=count)
    frames[0, :8, :16] = 255
    frames[0, 8:16, :8] = 0
    cap = 2 * 24 * count
    bits = cs.payload(cap + 64, seed=count)
    for n_bits, bit_offset in ((cap + 11, 0), (cap - 24 * count // 2 - (1 if count > 1 else 0), 37)):
        for nearest in (False, True):
            want, used = cs.select_batch_embed(frames, delta, bits[bit_offset:bit_offset + n_bits], index, nearest)
            got, done, plan = cs.host_embed(frames, delta, index, bits, bit_offset, n_bits, flags=2, nearest=nearest)
            assert done == used == min(n_bits, cap)
            assert np.array_equal(got, want), (delta, count, kind, n_bits, nearest)
            if index != cs.prefix(count):            # zigzag(1) and reversed(1) are the prefix [1]
                assert plan["path"] == EXACT and plan["rows"] == 8 and plan["selected"] == 1
        if count > 1 and bit_offset:
            assert used % count, "the budget must end inside a block"
    stego = cs.select_batch_embed(frames, delta, bits[:cap], index)[0]
    for src in (stego, frames):
        got, plan = cs.host_extract(src, delta, index)
        assert np.array_equal(got, cs.select_batch_extract(src, delta, index)), (delta, count, kind)


@pytest.mark.parametrize("content", ("noise", "flat", "clip"))
@pytest.mark.parametrize("delta", cs.DELTAS)
def test_gather_identity_on_the_host(content, delta):
    frames = cs.content(content, f=1, h=32, w=48, seed=9)
    all63 = orc.batch_extract_bits(frames, delta, 63).reshape(-1, 63)
    for index in (cs.zigzag(10), cs.zigzag(63), cs.scattered(33), cs.reversed_list(5), cs.zigzag(3, 6)):
        want = all63[:, np.array(index) - 1].reshape(-1)
        assert np.array_equal(cs.host_extract(frames, delta, index)[0], want)
        assert np.array_equal(cs.select_batch_extract(frames, delta, index), want)
        assert np.array_equal(coeffs.gather(all63.reshape(-1), index), want)


def test_host_routes_without_coefficients():
    frames = cs.content("clip", f=1, h=16, w=24)
    bits = cs.payload(100)
    for delta, index in ((0, cs.zigzag(5)), (-1.0, cs.zigzag(5)), (8, [])):
        want = cs.select_batch_embed(frames, delta, bits, index)
        got, done, plan = cs.host_embed(frames, delta, index, bits)
        assert done == want[1] == 0 and np.array_equal(got, want[0]) and plan["path"] == ROUND_TRIP and not plan["selected"]
        assert np.array_equal(got, orc.batch_embed(frames, delta, bits, 0 if not index else 5)[0])
        got, done, plan = cs.host_embed(frames, delta, index, bits, n_bits=0)
        assert done == 0 and np.array_equal(got, frames) and plan["path"] == COPY
    got, plan = cs.host_extract(frames, 0, cs.zigzag(5))
    assert plan["path"] == X_ZEROS and got.size == 6 * 5 and not got.any()


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_prefix_plans_as_n_ac_and_anything_else_plans_exact():
    import nearest_lib
    frames = cs.content("noise", f=1, h=16, w=24)
    bits = cs.payload(6 * 63)
    for n in (1, 3, 7, 8, 10, 15, 16, 63):
        for flags in (0, 1, 2):
            _, _, plan = cs.host_embed(frames, 8, cs.prefix(n), bits, flags=flags)
            path, _, _ = nearest_lib.plan(8, n, 6, bits.size, pocketfft=bool(flags & 1), nearest=False)
            assert plan["path"] == path and not plan["selected"], (n, flags)
            assert (path == STREAMING) == (n <= 15 and not flags & 1)
            assert plan["rows"] == (min((n >> 3) + 1, 2 if n <= 15 else 8) if n <= 15 else 8)
            _, xplan = cs.host_extract(frames, 8, cs.prefix(n), flags=flags)
            assert not xplan["selected"] and xplan["rows"] == (n >> 3) + 1
            assert xplan["path"] == (X_FAST if n >= 8 and not flags & 1 else X_EXACT), (n, flags)
        for index in (cs.zigzag(n), cs.reversed_list(n)) if n > 1 else (cs.zigzag(1, 2),):
            for flags in (0, 1, 2):
                _, _, plan = cs.host_embed(frames, 8, index, bits, flags=flags)
                assert (plan["path"], plan["rows"], plan["selected"]) == (EXACT, 8, 1), (index, flags)
                _, xplan = cs.host_extract(frames, 8, index, flags=flags)
                assert (xplan["path"], xplan["rows"], xplan["selected"]) == (X_EXACT, 8, 1), (index, flags)


def test_table_is_the_inverse_of_the_selection():
    for index in (cs.zigzag(63), cs.scattered(10), cs.prefix(1), []):
        ok, slot, count = cs.host_table(index)
        assert ok and count == len(index)
        for k in range(64):
            assert slot[k] == (index.index(k) if k in index else 255)
    for bad in ([0], [64], [3, 3], [1, 2, 200]):
        assert not cs.host_table(bad)[0], bad


# ---- the library: svs_coeffs_scan, validation, flags, exports -----------------------------------------------------------------
def _scan(scan, first, count):
    c = native.Coeffs()
    rc = native.load().svs_coeffs_scan(C.byref(c), scan, first, count)
    return rc, c.count, list(c.index)


def test_svs_coeffs_scan_against_the_literal_table():
    for first in (1, 2, 6, 40, 63):
        for count in (0, 1, 3, 10, 64 - first):
            if first + count > 64:
                continue
            rc, n, idx = _scan(native.SVS_SCAN_ZIGZAG, first, count)
            assert rc == 0 and n == count and idx == cs.ZIGZAG[first:first + count] + [0] * (63 - count)
            rc, n, idx = _scan(native.SVS_SCAN_ROW_MAJOR, first, count)
            assert rc == 0 and n == count and idx == list(range(first, first + count)) + [0] * (63 - count)
    assert _scan(native.SVS_SCAN_ZIGZAG, 1, 63)[2] == cs.ZIGZAG[1:]
    for scan, first, count in ((2, 1, 3), (-1, 1, 3), (1, 0, 3), (1, -2, 3), (1, 1, 64), (1, 2, 63), (1, 64, 1), (0, 1, -1)):
        assert _scan(scan, first, count)[0] == INVALID, (scan, first, count)
    assert native.load().svs_coeffs_scan(None, 1, 1, 3) == INVALID


def _coeffs_struct(count, index, tail=None):
    c = native.Coeffs()
    c.count = count
    for i, k in enumerate(index):
        c.index[i] = k
    if tail is not None:
        c.index[tail[0]] = tail[1]
    return c


def _select_calls(c, flags_embed=0, flags_extract=0):
    """the four entry points with a valid 8 x 8 plane and NULL data pointers: validation comes before any device work"""
    lib = native.load()
    planes = native.Planes.contiguous(1, 8, 8)
    cref = C.byref(c) if c is not None else None
    done = C.c_uint64(0)
    return (lib.svs_embed_select_dev(None, None, C.byref(planes), None, cref, 8.0, None, 0, 8, flags_embed, C.byref(done), None),
            lib.svs_embed_select(None, None, C.byref(planes), None, cref, 8.0, None, 0, 8, flags_embed, C.byref(done)),
            lib.svs_extract_select_dev(None, C.byref(planes), None, cref, 8.0, None, 0, flags_extract, C.byref(done), None),
            lib.svs_extract_select(None, C.byref(planes), None, cref, 8.0, None, 0, flags_extract, C.byref(done)))


def test_invalid_selections_are_refused_before_any_device_work():
    bad = [None,
           _coeffs_struct(1, [0]),                       # DC
           _coeffs_struct(2, [5, 0]),
           _coeffs_struct(1, [64]),
           _coeffs_struct(1, [255]),
           _coeffs_struct(3, [9, 2, 9]),                 # duplicate
           _coeffs_struct(2, [9, 2], tail=(2, 7)),       # non-zero tail
           _coeffs_struct(2, [9, 2], tail=(62, 1)),
           _coeffs_struct(64, list(range(1, 64))),       # count > 63
           _coeffs_struct(200, list(range(1, 64)))]
    for c in bad:
        assert _select_calls(c) == (INVALID,) * 4, None if c is None else (c.count, list(c.index)[:4])
    msg = native.load().svs_last_error().decode()
    assert "count" in msg or "coeffs" in msg


def test_rejected_flags():
    good = _coeffs_struct(3, [9, 2, 17])
    for flag in (native.SVS_READBACK, native.SVS_KEEP_COLOUR, 0x400, 0x1000, native.SVS_READBACK | native.SVS_NEAREST):
        assert _select_calls(good, flag, flag) == (INVALID,) * 4, hex(flag)
    # SVS_NEAREST: an embed flag - the extract calls refuse it, the embed calls get past the flag check (and then stop at the
    # NULL pointers, also before any device work)
    rc = _select_calls(good, native.SVS_NEAREST, native.SVS_NEAREST)
    assert rc[2:] == (INVALID, INVALID)
    lib = native.load()
    planes = native.Planes.contiguous(0, 8, 8)           # an empty batch: every accepted flag combination returns SVS_OK
    done = C.c_uint64(7)
    for flags in (0, 1, 2, 3, native.SVS_NEAREST, native.SVS_NEAREST | 1):
        assert lib.svs_embed_select_dev(None, None, C.byref(planes), None, C.byref(good), 8.0, None, 0, 8, flags, C.byref(done),
                                        None) == 0 and done.value == 0
        assert lib.svs_embed_select(None, None, C.byref(planes), None, C.byref(good), 8.0, None, 0, 8, flags, C.byref(done)) == 0
    for flags in (0, 1, 2, 3):
        assert lib.svs_extract_select_dev(None, C.byref(planes), None, C.byref(good), 8.0, None, 0, flags, C.byref(done), None) == 0
        assert lib.svs_extract_select(None, C.byref(planes), None, C.byref(good), 8.0, None, 0, flags, C.byref(done)) == 0
    # ... and the embed-only flags stay refused on extract for an empty batch too
    for flag in (native.SVS_READBACK, native.SVS_NEAREST):
        assert lib.svs_extract_select_dev(None, C.byref(planes), None, C.byref(good), 8.0, None, 0, flag, C.byref(done), None) == INVALID


def test_header_binding_and_exports_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "svsdct.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(svs_[a-z0-9_]+)\s*\(", text))
    new = {"svs_coeffs_scan", "svs_embed_select_dev", "svs_extract_select_dev", "svs_embed_select", "svs_extract_select"}
    assert new <= declared and new <= set(native.SIGNATURES)
    lib = native.load()
    for name in new:
        assert hasattr(lib, name)
    assert "#define SVS_ABI_VERSION 4" in text and "#define SVS_SCAN_ZIGZAG 1" in text and "#define SVS_SCAN_ROW_MAJOR 0" in text
    assert C.sizeof(native.Coeffs) == 64
    assert re.search(r"typedef struct svs_coeffs \{\s*uint8_t count;[^}]*uint8_t index\[63\];", text)
    assert len(native.SIGNATURES["svs_embed_select_dev"][1]) == 12 and len(native.SIGNATURES["svs_extract_select_dev"][1]) == 10


# ---- the Python layer -----------------------------------------------------------------------------------------------------
def test_spec_parsing():
    assert coeffs.selection(None, 5) is None
    assert coeffs.selection("rowmajor", 4) == (1, 2, 3, 4) and coeffs.is_prefix(coeffs.selection("rowmajor", 4))
    assert list(coeffs.selection("zigzag", 10)) == cs.ZIGZAG[1:11]
    assert list(coeffs.selection("zigzag:6", 3)) == cs.ZIGZAG[6:9]
    assert list(coeffs.selection(" zigzag : 6 ", 3)) == cs.ZIGZAG[6:9]
    assert list(coeffs.selection("zigzag", 100)) == cs.ZIGZAG[1:]      # n_ac clamps to 63 as everywhere
    assert coeffs.selection("zigzag", 0) == () == coeffs.selection("zigzag", -3)
    assert coeffs.selection([9, 2, 17], 3) == (9, 2, 17) == coeffs.selection(np.array([9, 2, 17]), 3)
    for spec, n in (("zigzag:0", 3), ("zigzag:62", 3), ("zigzag:x", 3), ("spiral", 3), ([9, 2], 3), ([0, 1, 2], 3),
                    ([64, 1, 2], 3), ([5, 5, 6], 3)):
        with pytest.raises(ValueError):
            coeffs.selection(spec, n)
    with pytest.raises(TypeError):
        coeffs.selection([1.5, 2, 3], 3)
    with pytest.raises(TypeError):
        coeffs.check("123")
    c = coeffs.native_coeffs((9, 2, 17))
    assert c.count == 3 and list(c.index) == [9, 2, 17] + [0] * 60


def test_from_env():
    assert coeffs.from_env(3, {}) is None and coeffs.from_env(3, {"SVS_COEFFS": "  "}) is None
    assert list(coeffs.from_env(3, {"SVS_COEFFS": "zigzag"})) == cs.ZIGZAG[1:4]
    assert list(coeffs.from_env(3, {"SVS_COEFFS": "zigzag:6"})) == cs.ZIGZAG[6:9]
    assert coeffs.from_env(3, {"SVS_COEFFS": "9, 2,0x11"}) == (9, 2, 17)
    assert coeffs.from_env(2, {"SVS_COEFFS": "rowmajor"}) == (1, 2)
    for value in ("9,2", "9,2,2", "0,1,2", "nope", "9,x,3"):
        with pytest.raises(ValueError):
            coeffs.from_env(3, {"SVS_COEFFS": value})


def test_value_errors_come_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(native, "load", no_library)
    frames = np.zeros((1, 8, 8), np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_frames(frames, 8, 3, np.zeros(3, np.uint8), coeffs="zigzag", readback=True)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_device(0, 0, planes, 8, 3, 0, 0, 3, coeffs="zigzag", readback=True)
    with pytest.raises(ValueError, match="n_ac"):
        batch.embed_frames(frames, 8, 3, np.zeros(3, np.uint8), coeffs=[9, 2])
    with pytest.raises(ValueError, match="n_ac"):
        batch.extract_frames(frames, 8, 4, coeffs=[9, 2, 17])
    with pytest.raises(ValueError):
        batch.extract_device(0, planes, 8, 3, 0, 0, coeffs=[9, 2, 2])
    with pytest.raises(ValueError, match="colour"):
        batch.embed_bgr_frames(np.zeros((1, 8, 8, 3), np.uint8), 8, 3, np.zeros(3, np.uint8), coeffs="zigzag")
    with pytest.raises(ValueError, match="colour"):
        batch.embed_bgr_device(0, 0, 0, planes, 8, 3, 0, 0, 3, coeffs="zigzag")
    with pytest.raises(ValueError, match="colour"):
        batch.extract_bgr_device(0, planes, 8, 3, 0, 0, coeffs=[9, 2, 17])
    import inspect
    for name in ("embed_frames", "extract_frames", "embed_device", "extract_device"):
        assert inspect.signature(getattr(batch, name)).parameters["coeffs"].default is None
    assert inspect.signature(pipeline.FramePipeline.__init__).parameters["coeffs"].default is None


def test_pipeline_refuses_readback_with_a_selection():
    with pytest.raises(ValueError, match="read-back"):
        pipeline.FramePipeline(8, 8, 1, 8, 3, coeffs="zigzag", readback=True)
    with pytest.raises(ValueError):
        pipeline.FramePipeline(8, 8, 1, 8, 3, coeffs=[1, 2])


def test_drop_in_refusals(monkeypatch, capsys):
    import embed_process as emb
    import extract_process as ext
    for switch in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
        monkeypatch.setenv("SVS_COEFFS", "zigzag")
        for other in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
            monkeypatch.setattr(emb, other, other == switch)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        out = capsys.readouterr().out
        assert "Error: SVS_COEFFS tidak dapat dipakai bersama" in out and "SVS_" + switch in out
    for other in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
        monkeypatch.setattr(emb, other, False)
    for value in ("spiral", "9,2", "zigzag:60"):         # n_ac = 10: two indices are too few, position 60 + 10 > 64
        monkeypatch.setenv("SVS_COEFFS", value)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        assert "Error: SVS_COEFFS tidak valid" in capsys.readouterr().out
        assert ext.ekstraksi_gambar_video_final("stego.avi", "out.png", 20, 10, None) is False
        assert "Error: SVS_COEFFS tidak valid" in capsys.readouterr().out
