"""CPU tier of matrix embedding (include/svsdct.h, svs_matrix_embed* / svs_matrix_extract*; GPU tier: test_matrix_gpu.py): the
header, the binding and the exports; the refusals (they need no GPU); the route; the host build of the matrix block bodies
(tests/hostemu/matrix_emu.cpp) against the independent NumPy sender and receiver of tests/matrix_lib.py, byte for byte; the k = 1
identity against the stepped bodies; the pair search's verdicts; and the PSNR table the README quotes."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import dither_lib as dl
import matrix_lib as mx
import minmove_lib as ml
import stepped_lib as st
from svsdct import batch, matrix, native, steps
from svsdct.pipeline import FramePipeline

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("svs_matrix_capacity_bits", "svs_matrix_embed_dev", "svs_matrix_embed", "svs_matrix_extract_dev", "svs_matrix_extract")
SHAPES = st.SHAPES          # (1, 8, 8), (3, 48, 272), (3, 40, 200)


@pytest.fixture(scope="module", autouse=True)
def emu(tmp_path_factory):
    return mx.emu(tmp_path_factory.mktemp("matrix_emu"))


# ---- 1. the header, the binding and the exports --------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_exports_agree():
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    declared = set(re.findall(r"\b(svs_matrix_\w+)\s*\(", header))
    assert declared == set(NAMES)
    assert {n for n in native.SIGNATURES if n.startswith("svs_matrix_")} == set(NAMES)
    lib = native.load()
    for name in NAMES:
        assert getattr(lib, name) is not None
    body = re.search(r"typedef struct svs_matrix \{(.*?)\} svs_matrix;", header, re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+)", body) == ["k", "search", "reserved"] and "reserved[2]" in body
    assert C.sizeof(native.Matrix) == 16 and [f[0] for f in native.Matrix._fields_] == ["k", "search", "reserved"]
    # the argument lists are the stepped calls' with the matrix behind the table
    for verb in ("embed_dev", "embed", "extract_dev", "extract"):
        want = list(native.SIGNATURES[f"svs_stepped_{verb}"][1])
        at = want.index(native._QS) + 1
        want.insert(at, native._MX)
        assert native.SIGNATURES[f"svs_matrix_{verb}"][1] == want, verb


def test_capacity():
    lib = native.load()
    planes = native.Planes.contiguous(3, 40, 200)
    for k in range(1, 7):
        m = matrix.matrix_struct(k)
        assert lib.svs_matrix_capacity_bits(C.byref(planes), C.byref(m)) == 3 * 5 * 25 * k == matrix.capacity_bits(3, 40, 200, k)
    for k in (0, 7):
        assert lib.svs_matrix_capacity_bits(C.byref(planes), C.byref(native.Matrix(k, 0))) == 0 == matrix.capacity_bits(3, 40, 200, k)
    assert lib.svs_matrix_capacity_bits(C.byref(planes), None) == 0
    assert lib.svs_matrix_capacity_bits(None, C.byref(matrix.matrix_struct(3))) == 0


# ---- 2. refusals (no GPU: every one comes before any device work) -----------------------------------------------------------------
INVALID = native.SVS_ERR_INVALID_ARG
FORMS = [(v, d) for v in ("embed", "extract") for d in (True, False)]
NO_TABLE = object()


def _call(verb, dev, m, n_ac=7, coeffs=None, table=None, flags=0, planes=None):
    lib = native.load()
    done = C.c_uint64(12345)
    planes = planes or native.Planes.contiguous(2, 16, 24)
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    tab = None if table is NO_TABLE else steps.steps_struct(st.uniform(20)) if table is None else table
    head = [64, 128, C.byref(planes)] if verb == "embed" else [64, C.byref(planes)]
    tail = [256, 0, 100, flags, C.byref(done)] if verb == "embed" else [128, 1 << 20, flags, C.byref(done)]
    rc = getattr(lib, f"svs_matrix_{verb}" + ("_dev" if dev else ""))(*head, None, ref(coeffs), None, ref(tab), ref(m), n_ac, *tail,
                                                                      *([None] if dev else []))
    return rc, lib.svs_last_error().decode(), int(done.value)


def _flags(*names):
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    return [int(re.search(rf"#define\s+{n}\s+(\S+)", header).group(1).rstrip("u"), 0) for n in names]


@pytest.mark.parametrize("verb,dev", FORMS)
def test_refusals_of_the_matrix_calls(verb, dev):
    good = matrix.matrix_struct(3)
    rc, msg, done = _call(verb, dev, None)
    assert rc == INVALID and "matrix is NULL" in msg and done == 12345
    rc, msg, done = _call(verb, dev, good, table=NO_TABLE)
    assert rc == INVALID and "steps is NULL" in msg and done == 12345
    for k in (0, 7, 64):
        rc, msg, done = _call(verb, dev, native.Matrix(k, 0), n_ac=(1 << min(k, 6)) - 1)
        assert rc == INVALID and "svs_matrix.k" in msg and done == 12345, (k, msg)
    rc, msg, done = _call(verb, dev, native.Matrix(3, 2))
    assert rc == INVALID and "svs_matrix.search" in msg and done == 12345
    for r in ((1, 0), (0, 1)):
        rc, msg, done = _call(verb, dev, native.Matrix(3, 0, (C.c_uint32 * 2)(*r)))
        assert rc == INVALID and "svs_matrix.reserved" in msg and done == 12345
    # the pair search is limited to k <= 5 (its wave tile of 2^k - 1 floats a lane must fit a launch's LDS)
    rc, msg, done = _call(verb, dev, native.Matrix(6, 1), n_ac=63)
    assert rc == INVALID and "k <= 5" in msg and done == 12345
    # a selection or n_ac of a size other than 2^k - 1
    for n_ac in (0, 3, 6, 8, 63, -1, 70):
        rc, msg, done = _call(verb, dev, good, n_ac=n_ac)
        assert rc == INVALID and "exactly 7 coefficients" in msg and done == 12345, (n_ac, msg)
    six = native.Coeffs(6, (C.c_uint8 * 63)(1, 8, 16, 9, 2, 3))
    rc, msg, done = _call(verb, dev, good, n_ac=7, coeffs=six)
    assert rc == INVALID and "exactly 7 coefficients" in msg and done == 12345
    # flags: SVS_READBACK, SVS_KEEP_COLOUR, unknown bits; an extract also SVS_NEAREST and SVS_MINMOVE
    readback, keep, nearest, minmove = _flags("SVS_READBACK", "SVS_KEEP_COLOUR", "SVS_NEAREST", "SVS_MINMOVE")
    for flags in [readback, keep, 1 << 30] + ([nearest, minmove] if verb == "extract" else []):
        rc, msg, done = _call(verb, dev, good, flags=flags)
        assert rc == INVALID and f"a matrix {verb} takes" in msg and done == 12345, (hex(flags), msg)
    # a bad table entry, as the stepped calls
    bad = steps.steps_struct(st.uniform(20))
    bad.delta[5] = 0
    rc, msg, done = _call(verb, dev, good, table=bad)
    assert rc == INVALID and "delta[5] = 0" in msg and done == 12345
    # what passes every check reaches the plane checks; an empty batch is no error and touches nothing
    rc, msg, _ = _call(verb, dev, good, planes=native.Planes(2, 16, 20, 0, 24, 16 * 24))
    assert rc == INVALID and "multiples of 8" in msg
    seven = native.Coeffs(7, (C.c_uint8 * 63)(*mx.zigzag(3)))
    for m, n_ac, coeffs in ((good, 7, None), (good, 99, seven), (native.Matrix(5, 1), 31, None), (native.Matrix(6, 0), 63, None)):
        rc, msg, done = _call(verb, dev, m, n_ac=n_ac, coeffs=coeffs, planes=native.Planes.contiguous(0, 16, 24))
        assert rc == 0 and done == 0, msg


def test_python_refusals_come_before_any_call():
    frames = np.zeros((1, 8, 8), np.uint8)
    table = st.uniform(20)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_frames(frames, 1.0, 7, "0101", matrix=3)
    with pytest.raises(ValueError, match="needs steps"):
        batch.extract_frames(frames, 1.0, 7, matrix=3)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_device(0, 0, native.Planes.contiguous(1, 8, 8), 1.0, 7, 0, 0, 4, matrix=(3, "pair"))
    with pytest.raises(ValueError, match="needs steps"):
        batch.extract_device(0, native.Planes.contiguous(1, 8, 8), 1.0, 7, 0, 64, matrix=3)
    with pytest.raises(ValueError, match="needs steps"):
        FramePipeline(8, 8, 1, 1.0, 7, matrix=3)
    for switch in (dict(readback=True), dict(readback_keyed=True), dict(readback_stepped=True), dict(readback_margin=64)):
        with pytest.raises(ValueError):
            batch.embed_frames(frames, 1.0, 7, "0101", steps=table, matrix=3, **switch)
        with pytest.raises(ValueError):
            batch.embed_device(0, 0, native.Planes.contiguous(1, 8, 8), 1.0, 7, 0, 0, 4, steps=table, matrix=3, **switch)
        with pytest.raises(ValueError):
            FramePipeline(8, 8, 1, 1.0, 7, steps=table, matrix=3, **switch)
    for bad in (0, 7, True, 2.0, (6, "pair"), (3, "triple"), (3,), "3"):
        with pytest.raises(ValueError):
            batch.embed_frames(frames, 1.0, 7, "0101", steps=table, matrix=bad)
    for call in (lambda: batch.extract_soft_frames(frames, 1.0, 7, steps=table, matrix=3),
                 lambda: batch.extract_vote_frames(frames, 1.0, 7, 8, steps=table, matrix=3),
                 lambda: batch.extract_histogram_frames(frames, 1.0, 7, steps=table, matrix=3),
                 lambda: batch.embed_frames_str(frames, 1.0, 7, "0101", matrix=3),
                 lambda: batch.extract_frames_str(frames, 1.0, 7, matrix=3),
                 lambda: batch.embed_bgr_frames(np.zeros((1, 8, 8, 3), np.uint8), 1.0, 7, "0101", matrix=3),
                 lambda: batch.extract_bgr_frames(np.zeros((1, 8, 8, 3), np.uint8), 1.0, 7, matrix=3)):
        with pytest.raises(ValueError, match="matrix embedding has no"):
            call()


def test_the_environment_switch():
    assert matrix.from_env({}) is None and matrix.from_env({"SVS_MATRIX": " "}) is None
    assert matrix.from_env({"SVS_MATRIX": "3"}) == 3 and matrix.from_env({"SVS_MATRIX": "4:pair"}) == (4, "pair")
    assert matrix.as_pair(3) == (3, 0) and matrix.as_pair((4, "pair")) == (4, 1) and matrix.slots(4) == 15
    for bad in ("0", "7", "6:pair", "3:both", "x", "3:"):
        if bad == "3:":
            assert matrix.from_env({"SVS_MATRIX": bad}) == 3
            continue
        with pytest.raises(ValueError):
            matrix.from_env({"SVS_MATRIX": bad})


EXACT_EMBED, EXACT_EXTRACT = 2, 1     # svs_route.hpp EmbedPath / ExtractPath


# ---- 3. the route ------------------------------------------------------------------------------------------------------------
def test_a_matrix_call_plans_the_stepped_holders_with_k_stream_bits_and_a_table_of_2_k_minus_1_slots():
    total = 600
    for k, search in itertools.product(range(1, 7), (0, 1)):
        if search and k == 6:
            continue
        word = 1 | ((k | (8 if search else 0)) << 16)
        for extra in (0, 8, 16, 32, 8 | 16 | 32):
            for index in (None, list(range(1, mx.slots(k) + 1)), list(mx.zigzag(k))):
                pe = mx.host_plan(True, k, search, total, total * k - 5, extra, index)
                assert (pe["path"], pe["rows"], pe["qm"], pe["n_ac"]) == (EXACT_EMBED, 8, ml.QM_DOUBLE, k), pe
                assert pe["steps_on"] == word and pe["table_count"] == mx.slots(k) and pe["use"] == total * k - 5, pe
                assert pe["keyed"] == int(bool(extra & 32)) and pe["tile_floats"] == 64 * mx.slots(k) * (2 if search else 1), pe
                px = mx.host_plan(False, k, search, total, 0, extra & 48, index)
                assert (px["path"], px["rows"], px["qm"], px["n_ac"]) == (EXACT_EXTRACT, 8, ml.QM_POW2, k), px
                assert (px["steps_on"], px["table_count"]) == (word, mx.slots(k)), px
    # the largest tiles a launch requests, four waves each: 64 x 2 x 31 floats with the search, 64 x 63 without
    assert 4 * 4 * mx.host_plan(True, 5, 1, total, 100)["tile_floats"] <= 64 * 1024
    assert 4 * 4 * mx.host_plan(True, 6, 0, total, 100)["tile_floats"] <= 64 * 1024


# ---- 4. the host build is the NumPy sender and receiver (search 0) -----------------------------------------------------------------
def _rotation():
    """(table, k, rule) -> an option set, rotated so that every option meets every k, rule and table"""
    names = list(mx.OPTIONS)
    cases = list(itertools.product(mx.TABLES, mx.KS, st.RULES))
    return [(t, k, r, names[(i + i // len(names)) % len(names)]) for i, (t, k, r) in enumerate(cases)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_host_build_is_the_numpy_sender_and_receiver(shape):
    """tables uniform(20), uniform(16), uniform(7), matched(75, 2) x k = 1, 2, 3, 4, 6 x the three rules, with and without a dither,
    a keyed order and a zig-zag selection (rotated); clipping noise; the payload ends inside a block and inside the last frame"""
    frames = st.content("full", SHAPES[shape])
    seen = set()
    for table, k, rule, option in _rotation():
        order_key, zz, key = mx.OPTIONS[option]
        index = mx.selection(k, zz)
        payload = mx.payload_for(SHAPES[shape], k)
        assert k == 1 or payload.size % k != 0
        assert payload.size < mx.capacity(SHAPES[shape], k) or mx.capacity(SHAPES[shape], k) == 1   # one block at k = 1 holds one bit
        want, used = mx.model_batch_embed(frames, st.TABLES[table], payload, k, index, rule, key, mx.FIRST_FRAME, order_key)
        got, host_used = mx.host_batch_embed(frames, st.TABLES[table], payload, k, index, 0, rule, key, mx.FIRST_FRAME, order_key)
        where = (shape, table, k, rule, option)
        assert used == host_used == payload.size, where
        assert np.array_equal(got, want), (where, int((got != want).sum()))
        bits = mx.host_batch_extract(got, st.TABLES[table], k, index, key, mx.FIRST_FRAME, order_key)
        assert np.array_equal(bits, mx.model_batch_extract(got, st.TABLES[table], k, index, key, mx.FIRST_FRAME, order_key)), where
        assert bits.size == mx.capacity(SHAPES[shape], k)
        seen.add(option)
    assert seen == set(mx.OPTIONS)


def test_blocks_past_the_budget_are_the_covers_and_a_cut_block_reads_zeros_past_it():
    frames = st.content("mid", SHAPES["odd"])
    k, index, table = 4, mx.zigzag(4), st.uniform(20)
    payload = mx.payload_for(SHAPES["odd"], k)
    got, used = mx.host_batch_embed(frames, table, payload, k, index, 1, "minmove")
    touched = -(-payload.size // k)
    per_frame = mx.n_blocks_of(frames[0])
    last = got[-1].reshape(5, 8, 25, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    cover = frames[-1].reshape(5, 8, 25, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    first_free = touched - 2 * per_frame
    assert 0 < first_free < per_frame and np.array_equal(last[first_free:], cover[first_free:])
    bits = mx.host_batch_extract(got, table, k, index)
    assert np.array_equal(bits[:payload.size], payload) and not bits[payload.size:touched * k].any()


# ---- 5. the k = 1 identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", (0, 1))
def test_k_1_is_the_stepped_call_on_the_host_build(search):
    for kind in ("full", "mid", "flat"):
        frames = st.content(kind, SHAPES["odd"])
        payload = mx.payload_for(SHAPES["odd"], 1)
        for table, rule, key, coeff in itertools.product(("u20", "u16", "u7", "m75x2"), st.RULES, (None, mx.DITHER_KEY), (1, 10, 63)):
            tab = st.TABLES[table]
            pos = 0
            for f, plane in enumerate(frames):
                part = payload[pos:pos + mx.n_blocks_of(plane)]
                got, used = mx.host_embed(plane, tab, part, 1, (coeff,), search, rule, key, f)
                want = st.host_embed(plane, tab, part, rule=rule, index=(coeff,), key=key, t=f)
                assert np.array_equal(got, want), (kind, table, rule, key, coeff, f)
                assert np.array_equal(mx.host_extract(got, tab, 1, (coeff,), key, f), st.host_extract(got, tab, index=(coeff,), key=key, t=f))
                pos += used


# ---- 6. the pair search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", st.RULES)
@pytest.mark.parametrize("k", (2, 3, 4, 5))
def test_the_pair_search_on_the_host_build(k, rule):
    """every block decodes to its message with the NumPy receiver; at most two parities of a block differ from the cover's; the
    chosen set's summed e is <= the single flip's, e recomputed in NumPy float32; and the set is a pair on a non-zero share of the
    blocks (a search 0 body would pass the rest)"""
    shape = SHAPES["odd"]
    frames = st.content("mid", shape)
    for option in ("plain", "all"):
        order_key, zz, key = mx.OPTIONS[option]
        index = mx.selection(k, zz)
        table = st.TABLES["m75x2" if option == "all" else "u20"]
        payload = mx.payload_for(shape, k)
        got, used = mx.host_batch_embed(frames, table, payload, k, index, 1, rule, key, mx.FIRST_FRAME, order_key)
        assert used == payload.size
        bits = mx.model_batch_extract(got, table, k, index, key, mx.FIRST_FRAME, order_key)
        assert np.array_equal(bits[:payload.size], payload), (k, rule, option, int((bits[:payload.size] != payload).sum()))
        pairs = singles = 0
        pos = 0
        for f in range(shape[0]):
            perm = dl._perm(order_key, mx.FIRST_FRAME + f, mx.n_blocks_of(frames[f]))
            p0, e = mx.flip_costs(frames[f], table, k, index, rule, key, mx.FIRST_FRAME + f, perm)
            p1 = mx.parities(got[f], table, k, index, key, mx.FIRST_FRAME + f, perm).astype(np.int64)
            left = min(payload.size - pos, p0.shape[0] * k)
            touched = -(-left // k)
            flipped = p0 ^ p1
            assert not flipped[touched:].any()
            count = flipped[:touched].sum(axis=1)
            assert count.max() <= 2, (k, rule, option, f, int(count.max()))
            j = mx.syndrome(p0[:touched]) ^ mx.messages(payload[pos:pos + left], k, touched)
            assert np.array_equal(count == 0, j == 0)
            for b in np.nonzero(count)[0]:
                chosen = np.nonzero(flipped[b])[0]
                assert np.bitwise_xor.reduce(chosen + 1) == j[b]
                cost = np.float32(e[b, chosen[0]] + e[b, chosen[1]]) if chosen.size == 2 else e[b, chosen[0]]
                assert cost <= e[b, j[b] - 1], (k, rule, option, f, b)
                if chosen.size == 2:
                    assert cost < e[b, j[b] - 1]
            pairs += int((count == 2).sum())
            singles += int((count == 1).sum())
            pos += left
        print(f"k = {k}, {rule}, {option}: {singles} single flips, {pairs} pairs")
        assert pairs > 0 and singles > 0


# ---- 7. the PSNR table --------------------------------------------------------------------------------------------------------
def _cell(cover, d, k, rule):
    table = st.uniform(d)
    message = np.random.default_rng(3).integers(0, 2, 4800 * k).astype(np.uint8)
    zz = mx.zigzag(k)
    plain, used = st.model_embed(cover, table, message, rule=rule, index=zz[:k])
    assert used == message.size
    errors = [int((st.model_extract(plain, table, index=zz[:k]) != message).sum())]
    values = [mx.psnr(plain, cover)]
    for search in (0, 1):
        stego, used = mx.host_embed(cover, table, message, k, zz, search, rule)
        assert used == message.size
        errors.append(int((mx.model_extract(stego, table, k, zz) != message).sum()))
        values.append(mx.psnr(stego, cover))
    return values, errors


def test_the_psnr_table():
    """one 480 x 640 frame of noise in [16, 240) (seed 1), message rng(3), k bits in each of the 4 800 blocks, a uniform table,
    SVS_MINMOVE: the plain stepped embed of the same bits on zig-zag 1..k against the matrix forms on zig-zag 1..2^k - 1.  0 bit
    errors in every cell, matrix > plain and pair >= single in every cell; under SVS_NEAREST at k = 4 the matrix forms are BELOW
    plain: the limit, pinned.  The README quotes the printed values."""
    cover = dl.noise((480, 640))
    print("| delta, k (n) | plain | single flip | cheapest of one flip or a pair |")
    for d in (12, 20, 40):
        for k in (2, 3, 4):
            (plain, single, pair), errors = _cell(cover, d, k, "minmove")
            print(f"| {d}, {k} ({mx.slots(k)}) | {plain:.2f} | {single:.2f} | {pair:.2f} |")
            assert errors == [0, 0, 0], (d, k, errors)
            assert single > plain and pair >= single, (d, k, plain, single, pair)
    for d in (12, 20, 40):
        (plain, single, pair), errors = _cell(cover, d, 4, "nearest")
        print(f"nearest: | {d}, 4 (15) | {plain:.2f} | {single:.2f} | {pair:.2f} |")
        assert errors == [0, 0, 0], (d, errors)
        assert single < plain and pair < plain, (d, plain, single, pair)


# ---- 8. the drop-in loops' refusals ------------------------------------------------------------------------------------------
def test_the_drop_in_loops_refuse_before_they_open_anything(monkeypatch, capsys):
    import embed_process as emb
    import extract_process as ext
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY", "SVS_STEPS"):
        monkeypatch.delenv(name, raising=False)
    for switch in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR", "READBACK_KEYED", "READBACK_STEPPED"):
        monkeypatch.setattr(emb, switch, False)
    monkeypatch.setattr(emb, "READBACK_MARGIN", "")
    monkeypatch.setenv("SVS_MATRIX", "3")
    assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 7, b"") == (False, None, None)
    assert "SVS_MATRIX memerlukan SVS_STEPS" in capsys.readouterr().out
    assert ext.ekstraksi_gambar_video_final("in.avi", "out.png", 20, 7, None) is False
    assert "SVS_MATRIX memerlukan SVS_STEPS" in capsys.readouterr().out
    monkeypatch.setenv("SVS_STEPS", ",".join(["20"] * 64))
    for value in ("0", "7", "6:pair", "3:both", "k"):
        monkeypatch.setenv("SVS_MATRIX", value)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 7, b"") == (False, None, None)
        assert "SVS_MATRIX tidak valid" in capsys.readouterr().out
        assert ext.ekstraksi_gambar_video_final("in.avi", "out.png", 20, 7, None) is False
        assert "SVS_MATRIX tidak valid" in capsys.readouterr().out
    monkeypatch.setenv("SVS_MATRIX", "3:pair")
    monkeypatch.setattr(emb, "READBACK_STEPPED", True)
    assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 7, b"") == (False, None, None)
    assert "SVS_MATRIX tidak dapat dipakai bersama" in capsys.readouterr().out
