"""CPU tier of the per-coefficient QIM steps (include/svsdct.h, svs_stepped_embed* / svs_stepped_extract*; GPU tier:
test_stepped_gpu.py): the NumPy model of the format against the existing models under a uniform table, the host build of the
stepped block bodies against the model, the fixed-point property that makes a matched table survive its codec, svs_matched_steps
against svsdct/steps.py, the stepped route, the refusals (they need no GPU), and the survival table of the README."""
import ctypes as C

import numpy as np
import pytest

import channel_lib as cl
import coeff_select_lib as cs
import dither_lib as dl
import minmove_lib as ml
import stepped_lib as st
import tie_lib as tl
from oracle.qim_dct_oracle import frame_embed, frame_extract_bits
from svsdct import channel, native, steps

KEY = st.DITHER_KEY


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return st.emu(tmp_path_factory.mktemp("stepped_emu"))


def frames_of(kind, shape=(2, 32, 48)):
    return cl.content(kind, shape)


# ---- 1. the model, under a uniform table, is the existing models --------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 16, 7))
def test_the_model_with_a_uniform_table_is_the_existing_models(d):
    table = st.uniform(d)
    for kind in ("full", "mid", "flat"):
        frames = frames_of(kind)
        for gray in frames:
            cap = (gray.shape[0] // 8) * (gray.shape[1] // 8) * 10
            bits = dl.payload(cap - 13, seed=d)
            # reference rule: the oracle itself
            assert np.array_equal(st.model_embed(gray, table, bits, 10)[0], frame_embed(gray, d, bits, 10)[1]), (kind, d)
            assert np.array_equal(st.model_extract(gray, table, 10), frame_extract_bits(gray, d, 10)), (kind, d)
            # nearest and minimum-move, with a selection: minmove_lib.model_embed
            for rule in ("nearest", "minmove"):
                want = ml.model_embed(gray, d, bits, 10, minmove=rule == "minmove", index=st.SELECTION)[1]
                assert np.array_equal(st.model_embed(gray, table, bits, rule=rule, index=st.SELECTION)[0], want), (kind, d, rule)
            assert np.array_equal(st.model_embed(gray, table, bits, index=st.SELECTION)[0],
                                  cs.select_embed(gray, d, bits, st.SELECTION)[1]), (kind, d)
            # the dither model, every rule, prefix and selection
            for rule in st.RULES:
                for index in (None, st.SELECTION):
                    got = st.model_embed(gray, table, bits, 10, rule, index, KEY, 3)[0]
                    want = dl.model_embed(gray, d, bits, 10, rule, index, KEY, 3)[0]
                    assert np.array_equal(got, want), (kind, d, rule, index)
                    assert np.array_equal(st.model_extract(want, table, 10, index, KEY, 3), dl.model_extract(want, d, 10, index, KEY, 3))


# ---- 2. the host build of the stepped block bodies is the model ----------------------------------------------------------------
def _emu_against_model(gray, table, bits, n_ac, index, stats, t=0):
    for rule in st.RULES:
        for key in (None, KEY):
            want, _ = st.model_embed(gray, table, bits, n_ac, rule, index, key, t, stats=stats)
            got = st.host_embed(gray, table, bits, n_ac, rule, index, key, t)
            assert np.array_equal(got, want), (rule, key, int((got != want).sum()))
    for key in (None, KEY):
        assert np.array_equal(st.host_extract(gray, table, n_ac, index, key, t), st.model_extract(gray, table, n_ac, index, key, t, stats=stats))


def test_the_host_build_of_the_stepped_bodies_is_the_model(emu):
    """embed_block_stepped under each rule with and without a dither, and extract_block_stepped, byte for byte on clipping noise,
    mid noise and flat blocks under every table of the GPU test, and on the tie corpus under the uniform table of its integer
    deltas.  The inputs reach quantiser inputs exactly on a half-integer and coefficients exactly 0: both are counted."""
    stats = {}
    for name, table in st.TABLES.items():
        for kind in ("full", "mid", "flat"):
            for gray in frames_of(kind):
                cap = (gray.shape[0] // 8) * (gray.shape[1] // 8) * 10
                bits = dl.payload(cap - 7, seed=len(name))
                _emu_against_model(gray, table, bits, 10, None, stats)
                _emu_against_model(gray, table, bits, 10, st.SELECTION, stats)
    zero = stats["zero"]
    assert zero > 0                                    # flat blocks: every AC coefficient is exactly 0 (the c == c0 branch)
    for d in (8, 20):                                  # the corpus's integer deltas, as uniform tables
        for n in (10, 63):
            frames, _ = tl.frames_for(n, d, 136)
            for f, gray in enumerate(frames):
                cap = (gray.shape[0] // 8) * (gray.shape[1] // 8) * n
                _emu_against_model(gray, st.uniform(d), dl.payload(cap, seed=d + n), n, None, stats, t=tl.FIRST_FRAME + f)
    print("quantiser inputs exactly on a half-integer:", stats["half"], " payload coefficients exactly 0:", stats["zero"])
    assert stats["half"] > 0 and stats["zero"] > 0


def test_the_tie_corpus_under_the_corpus_key_is_the_dithered_model(emu):
    """the corpus's dither ties are ties under ITS key and clip frames: the uniform table of delta = 20 against the dithered model"""
    stats = {}
    frames, _ = tl.frames_for(10, 20, 136)
    for f, gray in enumerate(frames):
        bits = dl.payload((gray.shape[0] // 8) * (gray.shape[1] // 8) * 10, seed=f)
        t = tl.FIRST_FRAME + f
        for rule in st.RULES:
            want = dl.model_embed(gray, 20, bits, 10, rule, None, tl.KEY, t)[0]
            assert np.array_equal(st.host_embed(gray, st.uniform(20), bits, 10, rule, None, tl.KEY, t), want), (f, rule)
        assert np.array_equal(st.host_extract(gray, st.uniform(20), 10, None, tl.KEY, t), dl.model_extract(gray, 20, 10, None, tl.KEY, t))
        st.model_extract(gray, st.uniform(20), 10, None, tl.KEY, t, stats=stats)
    assert stats["half"] > 0


# ---- 3. the fixed-point property --------------------------------------------------------------------------------------------
def test_a_lattice_point_of_a_matched_step_is_a_fixed_point_of_the_requantiser():
    """rintf(c / s_k) * s_k == c for c = q * m * s_k: every codec step 1..255 (every k of every table), m = 1..16 and q over
    +-2040 / delta_k, in the channel's float32 arithmetic"""
    for s in range(1, 256):
        sf = np.float32(s)
        for m in range(1, 17):
            dk = s * m
            if dk > 4095:
                break
            qmax = 2040 // dk
            c = (np.arange(-qmax, qmax + 1, dtype=np.int64) * dk).astype(np.float32)
            back = np.rint(c / sf) * sf
            assert back.dtype == np.float32 and np.array_equal(back, c), (s, m)


# ---- 4. svs_matched_steps ---------------------------------------------------------------------------------------------------
def test_matched_steps_agree_with_the_python_restatement():
    lib = native.load()
    for q in range(1, 101):
        codec = channel.steps_struct(q)
        for multiple in (1, 2, 3, 4):
            for floor in (0, 16):
                out = native.QimSteps()
                assert lib.svs_matched_steps(C.byref(out), C.byref(codec), multiple, floor) == 0, (q, multiple, floor)
                want = steps.matched(q, multiple, floor)
                assert np.array_equal(np.array(out.delta[:], np.uint16), want), (q, multiple, floor)
                assert np.array_equal(want, st.matched(q, multiple, floor))
    assert list(steps.matched(75, 2)[1:11]) == [12, 10, 16, 24, 40, 52, 62, 12, 12, 14]
    assert np.array_equal(steps.uniform(20), st.uniform(20))


def test_matched_steps_refusals():
    lib = native.load()
    codec = channel.steps_struct(50)
    out = native.QimSteps()
    for k in range(64):
        out.delta[k] = 7
    INVALID = lib.svs_matched_steps(None, C.byref(codec), 2, 0)
    assert INVALID != 0 and b"out is NULL" in lib.svs_last_error()
    assert lib.svs_matched_steps(C.byref(out), None, 2, 0) == INVALID and b"codec is NULL" in lib.svs_last_error()
    for multiple in (0, 17, -1):
        assert lib.svs_matched_steps(C.byref(out), C.byref(codec), multiple, 0) == INVALID and b"multiple" in lib.svs_last_error()
    for floor in (-1, 4096):
        assert lib.svs_matched_steps(C.byref(out), C.byref(codec), 2, floor) == INVALID and b"floor" in lib.svs_last_error()
    bad = channel.steps_struct(50)
    bad.step[9] = 0
    assert lib.svs_matched_steps(C.byref(out), C.byref(bad), 2, 0) == INVALID and b"step[9]" in lib.svs_last_error()
    bad.step[9] = 256
    assert lib.svs_matched_steps(C.byref(out), C.byref(bad), 2, 0) == INVALID and b"step[9]" in lib.svs_last_error()
    big = channel.steps_struct(np.full(64, 255, np.uint16))
    assert lib.svs_matched_steps(C.byref(out), C.byref(big), 16, 0) == 0          # 4080
    assert lib.svs_matched_steps(C.byref(out), C.byref(big), 1, 4095) == INVALID and b"delta[1]" in lib.svs_last_error()   # 4335
    for k in range(64):
        out.delta[k] = 7
    assert lib.svs_matched_steps(C.byref(out), C.byref(big), 1, 4095) == INVALID
    assert all(v == 7 for v in out.delta)              # a refusal leaves *out as it was
    with pytest.raises(ValueError, match=r"delta\[1\]"):
        steps.matched(np.full(64, 255, np.uint16), 1, 4095)
    for args in ((50, 0), (50, 17), (50, 2, -1), (50, 2, 4096), (0, 2), (101, 2)):
        with pytest.raises(ValueError):
            steps.matched(*args)


def test_step_tables_from_python():
    with pytest.raises(ValueError, match=r"delta\[5\]"):
        steps.as_table([0] + [3] * 4 + [0] + [3] * 58)
    with pytest.raises(ValueError, match=r"delta\[63\]"):
        steps.as_table([1] * 63 + [4096])
    with pytest.raises(ValueError):
        steps.as_table([1] * 63)
    with pytest.raises(ValueError):
        steps.uniform(0)
    with pytest.raises(ValueError):
        steps.uniform(4096)
    assert steps.from_env({}) is None and steps.from_env({"SVS_STEPS": " "}) is None
    assert np.array_equal(steps.from_env({"SVS_STEPS": "q75x2"}), st.matched(75, 2))
    assert np.array_equal(steps.from_env({"SVS_STEPS": "q95x2f16"}), st.matched(95, 2, 16))
    assert np.array_equal(steps.from_env({"SVS_STEPS": ",".join(str(int(v)) for v in st.odd_steps())}), st.odd_steps())
    for spec in ("q75", "75x2", "q75x2f", "1,2,3", "q0x2", "q75x17"):
        with pytest.raises(ValueError):
            steps.parse(spec)
    s = steps.steps_struct(st.matched(50, 3))
    assert list(s.delta) == [int(v) for v in st.matched(50, 3)]


# ---- 5. routing -------------------------------------------------------------------------------------------------------------
EXACT_EMBED, COPY, ROUND_TRIP, EXACT_EXTRACT = 2, 0, 1, 1     # svs_route.hpp EmbedPath / ExtractPath
QM_DOUBLE, QM_POW2 = ml.QM_DOUBLE, ml.QM_POW2


@pytest.mark.parametrize("mode", (0, 1, 2), ids=("fast", "pocketfft", "guarded"))
@pytest.mark.parametrize("n_ac", (3, 10, 20, 63))
def test_a_stepped_call_plans_the_exact_kernels_that_hold_the_stepped_side(emu, mode, n_ac):
    """EXACT, rows = 8 and the holder's quantiser mode - QM_DOUBLE for an embed, QM_POW2 for an extract - in every mode, with and
    without a rule, a dither, an order, a selection and a PREFIX selection (which plans as no selection and brings the prefix
    table); never streaming, never FAST"""
    total = 600
    prefix = list(range(1, n_ac + 1))
    scattered = cs.scattered(min(n_ac, 40))
    for extra in (0, 4, 8, 16, 32, 4 | 16 | 32):
        for index in (None, prefix, scattered):
            count = n_ac if index is None else len(index)
            pe = st.host_plan(True, n_ac, total, total * count - 5, mode | extra, index)
            assert (pe["path"], pe["rows"], pe["qm"], pe["stepped"], pe["steps_on"]) == (EXACT_EMBED, 8, QM_DOUBLE, 1, 1), pe
            assert pe["table_count"] == count and pe["selected"] == int(index is scattered), pe
            assert pe["dithered"] == int(bool(extra & 16)) and pe["keyed"] == int(bool(extra & 32)) and pe["use"] == total * count - 5
            px = st.host_plan(False, n_ac, total, 0, mode | (extra & 48), index)
            assert (px["path"], px["rows"], px["qm"], px["stepped"], px["steps_on"]) == (EXACT_EXTRACT, 8, QM_POW2, 1, 1), px
            assert px["table_count"] == count and px["selected"] == int(index is scattered), px


def test_a_stepped_call_with_nothing_to_embed_copies_or_round_trips(emu):
    p = st.host_plan(True, 10, 600, 0)
    assert (p["path"], p["stepped"], p["steps_on"], p["use"]) == (COPY, 0, 0, 0), p
    p = st.host_plan(True, 0, 600, 77)
    assert (p["path"], p["rows"], p["stepped"], p["steps_on"], p["use"]) == (ROUND_TRIP, 8, 0, 0, 0), p


# ---- 6. refusals (no GPU: every one comes before any device work) ---------------------------------------------------------------
INVALID = native.SVS_ERR_INVALID_ARG


def _args(verb, dev, planes, order, coeffs, dither, table, flags, done, n_ac=10, gray=64, out=128, bits=256):
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    head = [gray, out, C.byref(planes)] if verb == "embed" else [gray, C.byref(planes)]
    tail = [bits, 0, 100, flags, C.byref(done)] if verb == "embed" else [out, 1 << 20, flags, C.byref(done)]
    return [*head, ref(order), ref(coeffs), ref(dither), ref(table), n_ac, *tail, *([None] if dev else [])]


def _call(verb, dev, **kw):
    lib = native.load()
    done = C.c_uint64(12345)
    planes = kw.pop("planes", native.Planes.contiguous(2, 16, 24))
    rc = getattr(lib, f"svs_stepped_{verb}" + ("_dev" if dev else ""))(
        *_args(verb, dev, planes, kw.get("order"), kw.get("coeffs"), kw.get("dither"), kw.get("table"), kw.get("flags", 0), done,
               kw.get("n_ac", 10)))
    return rc, lib.svs_last_error().decode(), int(done.value)


FORMS = [(v, d) for v in ("embed", "extract") for d in (True, False)]


def _table(values=None):
    return steps.steps_struct(st.uniform(20) if values is None else values)


def _raw_table(mutate):
    t = _table()
    mutate(t)
    return t


@pytest.mark.parametrize("verb,dev", FORMS)
def test_refusals_of_the_stepped_calls(verb, dev):
    # steps: NULL, an entry of 0, an entry above 4095; entry 0 (DC) is not read
    rc, msg, done = _call(verb, dev)
    assert rc == INVALID and "steps is NULL" in msg and done == 12345
    for k, v in ((1, 0), (37, 0), (63, 4096), (12, 65535)):
        rc, msg, done = _call(verb, dev, table=_raw_table(lambda t: t.delta.__setitem__(k, v)))
        assert rc == INVALID and f"delta[{k}] = {v}" in msg and done == 12345, msg
    # dither, coeffs, flags, each on its own
    bad_dither = native.Dither(5, 0, 1)
    rc, msg, done = _call(verb, dev, table=_table(), dither=bad_dither)
    assert rc == INVALID and "svs_dither.reserved" in msg and done == 12345
    rc, msg, done = _call(verb, dev, table=_table(), dither=native.Dither(5, 3, 0), order=native.BlockOrder(9, 4, 0))
    assert rc == INVALID and "first_frame" in msg and done == 12345
    bad_coeffs = native.Coeffs(2, (C.c_uint8 * 63)(5, 5))
    rc, msg, done = _call(verb, dev, table=_table(), coeffs=bad_coeffs)
    assert rc == INVALID and "svs_coeffs.index" in msg and done == 12345
    rc, msg, done = _call(verb, dev, table=_table(), coeffs=native.Coeffs(0, (C.c_uint8 * 63)(0, 7)))
    assert rc == INVALID and "behind count" in msg and done == 12345
    refused = _flag_values(verb)
    for flags in refused:
        rc, msg, done = _call(verb, dev, table=_table(), flags=flags)
        assert rc == INVALID and f"a stepped {verb} takes" in msg and done == 12345, (hex(flags), msg)
    # the order of the checks, in pairs: steps before dither before coeffs before flags
    bad_flags = refused[0]
    rc, msg, _ = _call(verb, dev, dither=bad_dither, coeffs=bad_coeffs, flags=bad_flags)
    assert "steps is NULL" in msg
    rc, msg, _ = _call(verb, dev, table=_raw_table(lambda t: t.delta.__setitem__(2, 0)), dither=bad_dither)
    assert "delta[2]" in msg
    rc, msg, _ = _call(verb, dev, table=_table(), dither=bad_dither, coeffs=bad_coeffs)
    assert "svs_dither.reserved" in msg
    rc, msg, _ = _call(verb, dev, table=_table(), coeffs=bad_coeffs, flags=bad_flags)
    assert "svs_coeffs.index" in msg
    rc, msg, _ = _call(verb, dev, table=_table(), dither=bad_dither, flags=bad_flags)
    assert "svs_dither.reserved" in msg
    # then what every gray call checks: the planes, the order
    rc, msg, _ = _call(verb, dev, table=_table(), planes=native.Planes(2, 16, 20, 0, 24, 16 * 24))
    assert rc == INVALID and "multiples of 8" in msg
    rc, msg, done = _call(verb, dev, table=_table(), order=native.BlockOrder(9, 0, 1))
    assert rc == INVALID and "svs_block_order.reserved" in msg and done == 0        # as the ordered calls: the count is cleared first
    # an empty batch is no error and touches nothing
    rc, msg, done = _call(verb, dev, table=_table(), planes=native.Planes.contiguous(0, 16, 24))
    assert rc == 0 and done == 0


def _flag_values(verb):
    """the flags a stepped call refuses: SVS_READBACK, SVS_KEEP_COLOUR and unknown bits; an extract also SVS_NEAREST / SVS_MINMOVE"""
    import re
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svsdct.h")).read()
    value = {}
    for name in ("SVS_READBACK", "SVS_KEEP_COLOUR", "SVS_NEAREST", "SVS_MINMOVE", "SVS_EXACT_POCKETFFT", "SVS_EXACT_GUARDED"):
        m = re.search(r"#define\s+" + name + r"\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\s*(?:<<\s*(\d+))?", header)
        assert m, name
        value[name] = int(m.group(1), 0) << int(m.group(2) or 0)
    out = [value["SVS_READBACK"], value["SVS_KEEP_COLOUR"], 1 << 30, value["SVS_READBACK"] | value["SVS_EXACT_POCKETFFT"]]
    if verb == "extract":
        out += [value["SVS_NEAREST"], value["SVS_MINMOVE"]]
    return out


def test_python_refuses_what_has_no_stepped_form():
    from svsdct import batch
    frames = np.zeros((1, 8, 8), np.uint8)
    for kw in (dict(readback=True), dict(readback_keyed=True)):
        with pytest.raises(ValueError, match="read-back"):
            batch.embed_frames(frames, 20, 3, np.zeros(3, np.uint8), steps=st.uniform(20), **kw)
        with pytest.raises(ValueError, match="read-back"):
            batch.embed_device(64, 64, native.Planes.contiguous(1, 8, 8), 20, 3, 128, 0, 3, steps=st.uniform(20), **kw)
    with pytest.raises(ValueError, match=r"delta\[1\]"):
        batch.extract_frames(frames, 20, 3, steps=np.zeros(64, np.uint16))


# ---- 7. the survival table -----------------------------------------------------------------------------------------------------
def test_the_survival_table():
    """the README's table, from the model: what matched steps buy at equal survival.  The uniform rows are the README's rows of
    the requantisation channel (channel_lib.survival gives the same counts)."""
    rows = st.survival_table()
    print("\n" + st.format_survival(rows))
    by = {label: (p, e) for label, _, p, e in rows}
    steps_of = {label: s for label, s, _, _ in rows}
    zero = [0, 0, 0]

    def errors(label):
        return [by[label][1][q] for q in cl.QUALITIES]

    # the uniform rows reproduce the channel's table (README, requantisation channel)
    assert errors("1..10; uniform 20; reference") == [zero, zero, zero, [143, 136, 131], [481, 453, 455]]
    assert cl.survival(20, 10, None, "reference", 75)["single"] == [143, 136, 131]
    assert errors("1..10; uniform 40; reference") == [zero, zero, zero, zero, [141, 145, 133]]
    # the row-major matched row: integers, and PSNR to 0.01 dB
    assert steps_of["1..10; matched; reference"] == [12, 10, 16, 24, 40, 52, 62, 12, 12, 14]
    assert errors("1..10; matched; reference") == [zero, zero, zero, zero, [0, 0, 1]]
    assert round(by["1..10; matched; reference"][0], 2) == 28.81
    # the two zig-zag reference-rule rows the feature was proposed with - steps 12,14,12,10,16,14,14,14,18,18, 32.51 and 35.23 dB:
    # those steps and figures are the ones of scan positions 2..11 (k = 8, 16, 9, 2, 3, 10, 17, 24, 32, 25) ...
    assert st.ZZ_2_11 == (8, 16, 9, 2, 3, 10, 17, 24, 32, 25)
    assert steps_of["zig-zag 2..11; matched; reference"] == [12, 14, 12, 10, 16, 14, 14, 14, 18, 18]
    assert errors("zig-zag 2..11; uniform 20; reference") == [zero] * 5
    assert round(by["zig-zag 2..11; uniform 20; reference"][0], 2) == 32.51
    assert errors("zig-zag 2..11; matched; reference") == [zero] * 5
    assert round(by["zig-zag 2..11; matched; reference"][0], 2) == 35.23
    # ... and the same two rows on scan positions 1..10 proper (k = 1, 8, 16, 9, 2, 3, 10, 17, 24, 32): the model's numbers
    assert st.ZZ_1_10 == (1, 8, 16, 9, 2, 3, 10, 17, 24, 32)
    assert steps_of["zig-zag 1..10; matched; reference"] == [12, 12, 14, 12, 10, 16, 14, 14, 14, 18]
    assert errors("zig-zag 1..10; uniform 20; reference") == [zero] * 5
    assert round(by["zig-zag 1..10; uniform 20; reference"][0], 2) == 32.47
    assert errors("zig-zag 1..10; matched; reference") == [zero] * 5
    assert round(by["zig-zag 1..10; matched; reference"][0], 2) == 35.69
    assert errors("zig-zag 6..15; uniform 20; reference")[-1] == [139, 145, 145]
    assert errors("zig-zag 6..15; matched; reference") == [zero, zero, zero, zero, [1, 0, 1]]


def test_a_table_matched_to_a_fine_codec_table_needs_a_floor():
    """twice the quality-95 table has steps of 2 - 4 on the low frequencies, below the embed's own truncation disturbance of up
    to 4.0: it fails at quality 95 itself; with floor = 16 the per-quality tables are error-free"""
    _, e = st.survival(st.matched(95, 2), st.ROW_1_10, "reference", qualities=(95,))
    print("x2 of the quality-95 table at quality 95:", e[95])
    assert min(e[95]) > 50
    _, e = st.survival(st.matched(95, 2, 16), st.ROW_1_10, "reference", qualities=(95,))
    assert e[95] == [0, 0, 0]


# ---- 8. the drop-in loops -----------------------------------------------------------------------------------------------------
def test_drop_in_refusals(monkeypatch, capsys):
    """SVS_STEPS is refused with the switches that have no stepped form, as SVS_COEFFS is, and an invalid value before any work"""
    import embed_process as emb
    import extract_process as ext
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY"):
        monkeypatch.delenv(name, raising=False)
    switches = ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR", "READBACK_KEYED")
    monkeypatch.setenv("SVS_STEPS", "q75x2")
    for switch in switches:
        for other in switches:
            monkeypatch.setattr(emb, other, other == switch)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        out = capsys.readouterr().out
        assert "Error: SVS_STEPS tidak dapat dipakai bersama" in out and "SVS_" + switch in out
    for other in switches:
        monkeypatch.setattr(emb, other, False)
    for value in ("q75", "q75x0", "1,2,3", "q101x2"):
        monkeypatch.setenv("SVS_STEPS", value)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        assert "Error: SVS_STEPS tidak valid" in capsys.readouterr().out
        assert ext.ekstraksi_gambar_video_final("stego.avi", "out.png", 20, 10, None) is False
        assert "Error: SVS_STEPS tidak valid" in capsys.readouterr().out
