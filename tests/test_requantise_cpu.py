"""The requantisation channel without a GPU (include/svsdct.h, svs_quality_steps / svs_requantise*): the quality tables of the
library against svsdct/channel.py and the standard, every refusal of the two calls through the real library, the properties of
the host model (tests/channel_lib.py), what the inputs of tests/test_requantise_gpu.py exercise, and the survival table the
README quotes."""
import ctypes as C
import os

import numpy as np
import pytest

import channel_lib as cl
from testlib import build_emu
from svsdct import channel, native
from svsdct.native import Planes, Steps

PKG = os.path.dirname(os.path.dirname(os.path.abspath(native.__file__)))
INVALID = native.SVS_ERR_INVALID_ARG
FAKE_IN, FAKE_OUT = 0x7F0000001000, 0x7F0000101000     # 8-byte aligned, far apart, never dereferenced: every case is refused


@pytest.fixture(scope="module")
def lib():
    return native.load()


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_three_calls(lib):
    for name in ("svs_quality_steps", "svs_requantise_dev", "svs_requantise"):
        assert name in native.SIGNATURES and getattr(lib, name)
    assert C.sizeof(Steps) == 128


def test_quality_steps_of_the_library_are_the_python_ones(lib):
    for quality in range(1, 101):
        out = Steps()
        assert lib.svs_quality_steps(C.byref(out), quality) == native.SVS_OK
        got = np.array(out.step[:], np.uint16)
        want = channel.quality_steps(quality)
        assert want.dtype == np.uint16 and want.shape == (64,)
        assert np.array_equal(got, want), quality
        assert np.array_equal(np.array(channel.steps_struct(quality).step[:]), want)
    assert np.array_equal(channel.quality_steps(50), channel.ANNEX_K_LUMA)
    assert channel.ANNEX_K_LUMA[0] == 16 and channel.ANNEX_K_LUMA[63] == 99 and int(channel.ANNEX_K_LUMA.sum()) == 3688
    assert (channel.quality_steps(100) == 1).all()
    assert (channel.quality_steps(1) == 255).all()                    # 16 * 5000 / 100 = 800 and up: every entry clamps
    assert channel.quality_steps(25)[0] == 32 and channel.quality_steps(75)[0] == 8


@pytest.mark.parametrize("quality", (0, 101, -3, 1000))
def test_quality_outside_1_100_is_refused(lib, quality):
    out = Steps(*[(C.c_uint16 * 64)(*([0xABCD] * 64))])
    assert lib.svs_quality_steps(C.byref(out), quality) == INVALID
    assert str(quality) in lib.svs_last_error().decode()
    assert all(v == 0xABCD for v in out.step)
    with pytest.raises(ValueError):
        channel.quality_steps(quality)
    assert lib.svs_quality_steps(None, 50) == INVALID


def test_python_tables_are_checked():
    for bad, k in ((np.zeros(64, np.int64), 0), (np.where(np.arange(64) == 17, 256, 3), 17)):
        with pytest.raises(ValueError, match=rf"step\[{k}\]"):
            channel.as_steps(bad)
    with pytest.raises(ValueError):
        channel.as_steps(np.ones(63, np.int64))
    with pytest.raises(ValueError):
        channel.as_steps(np.ones(64))
    assert np.array_equal(channel.as_steps(np.full((8, 8), 7)), np.full(64, 7, np.uint16))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------
GOOD_PLANES = (2, 16, 24, 0, 24, 16 * 24)


def _call(lib, host, planes=GOOD_PLANES, steps="ones", flags=0, d_in=FAKE_IN, d_out=FAKE_OUT):
    """one call with fake pointers -> (return code, message)"""
    p = None if planes is None else Planes(*planes)
    s = None if steps is None else Steps((C.c_uint16 * 64)(*(int(v) for v in (cl.TABLES["ones"] if isinstance(steps, str) else steps))))
    args = [d_in, d_out, C.byref(p) if p is not None else None, C.byref(s) if s is not None else None, flags]
    rc = lib.svs_requantise(*args) if host else lib.svs_requantise_dev(*args, None)
    return rc, lib.svs_last_error().decode()


def _with(k, v):
    t = np.ones(64, np.int64)
    t[k] = v
    return t


REFUSALS = [
    ("steps NULL", dict(steps=None), "steps is NULL"),
    ("a step of 0 at DC", dict(steps=_with(0, 0)), "step[0] = 0"),
    ("a step of 0 at 37", dict(steps=_with(37, 0)), "step[37] = 0"),
    ("a step of 256 at 63", dict(steps=_with(63, 256)), "step[63] = 256"),
    ("a step of 65535 at 5", dict(steps=_with(5, 65535)), "step[5] = 65535"),
    ("flags 1", dict(flags=native.SVS_EXACT_POCKETFFT), "flags 0x1"),
    ("flags SVS_NEAREST", dict(flags=native.SVS_NEAREST), "flags 0x800"),
    ("planes NULL", dict(planes=None), "planes is NULL"),
    ("planes reserved", dict(planes=(2, 16, 24, 1, 24, 384)), "reserved"),
    ("height 12", dict(planes=(2, 12, 24, 0, 24, 288)), "multiples of 8"),
    ("width 0", dict(planes=(2, 16, 0, 0, 24, 384)), "geometry"),
    ("negative frame count", dict(planes=(-1, 16, 24, 0, 24, 384)), "geometry"),
    ("row pitch below the width", dict(planes=(2, 16, 24, 0, 16, 384)), "row_pitch"),
    ("row pitch 28", dict(planes=(2, 16, 24, 0, 28, 28 * 16)), "row_pitch"),
    ("frame pitch below a frame", dict(planes=(2, 16, 24, 0, 24, 376)), "frame_pitch"),
    ("frame pitch 388", dict(planes=(2, 16, 24, 0, 24, 388)), "frame_pitch"),
    ("in NULL", dict(d_in=None), "NULL"),
    ("out NULL", dict(d_out=None), "NULL"),
    ("partial overlap", dict(d_out=FAKE_IN + 64), "overlap"),
]
DEVICE_ONLY = [
    ("in misaligned", dict(d_in=FAKE_IN + 4), "8-byte aligned"),
    ("out misaligned", dict(d_out=FAKE_OUT + 2), "8-byte aligned"),
]


@pytest.mark.parametrize("host", (False, True), ids=("dev", "host"))
@pytest.mark.parametrize("name,changes,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_work(lib, host, name, changes, message):
    """fake pointers and n_frames > 0: a call that got past its checks would not return SVS_ERR_INVALID_ARG"""
    rc, text = _call(lib, host, **changes)
    assert rc == INVALID, (name, rc, text)
    assert message in text, (name, text)


@pytest.mark.parametrize("name,changes,message", DEVICE_ONLY, ids=[r[0] for r in DEVICE_ONLY])
def test_device_pointers_must_be_aligned(lib, name, changes, message):
    """the device form alone: the host form stages through buffers of its own"""
    rc, text = _call(lib, False, **changes)
    assert rc == INVALID and message in text, (name, rc, text)


@pytest.mark.parametrize("host", (False, True), ids=("dev", "host"))
def test_the_first_fault_in_the_documented_order_is_reported(lib, host):
    """steps, then flags, then planes, then pointers"""
    rc, text = _call(lib, host, steps=_with(9, 0), flags=4, planes=None, d_in=None)
    assert rc == INVALID and "step[9] = 0" in text
    rc, text = _call(lib, host, flags=4, planes=None, d_in=None)
    assert rc == INVALID and "flags 0x4" in text
    rc, text = _call(lib, host, planes=None, d_in=None)
    assert rc == INVALID and "planes is NULL" in text


@pytest.mark.parametrize("host", (False, True), ids=("dev", "host"))
def test_the_empty_call_is_ok_and_looks_at_no_pointer(lib, host):
    rc, text = _call(lib, host, planes=(0, 16, 24, 0, 24, 384), d_in=None, d_out=None)
    assert rc == native.SVS_OK, text
    rc, _ = _call(lib, host, planes=(0, 16, 24, 0, 24, 384), steps=_with(1, 0), d_in=None, d_out=None)
    assert rc == INVALID                  # a faulty table is refused even then


# ---- 3. the model ----------------------------------------------------------------------------------------------------------
def test_a_second_pass_through_the_coarsest_table_changes_nothing():
    """all 255: the first pass leaves every coefficient on a multiple of 255 up to the store's rounding of at most 1/2 a pixel -
    at most 4 in a coefficient, far from the decision boundary at 127.5 - so the second pass finds the same indices"""
    frames = np.random.default_rng(3).integers(0, 256, (2, 48, 64)).astype(np.uint8)
    once = cl.model_requantise(frames, cl.TABLES["all255"])
    assert not np.array_equal(once, frames)
    assert np.array_equal(cl.model_requantise(once, cl.TABLES["all255"]), once)


def test_the_all_ones_table_only_rounds():
    frames = np.random.default_rng(8).integers(16, 240, (2, 64, 96)).astype(np.uint8)
    out = cl.model_requantise(frames, cl.TABLES["ones"])
    diff = np.abs(out.astype(np.int64) - frames)
    print(f"all ones on noise in [16, 240): {int((diff != 0).sum())} of {diff.size} pixels move, by at most {int(diff.max())}")
    assert diff.max() <= 1
    plane = cl.model_requantise(frames[0], cl.TABLES["ones"])           # one plane in, one plane out
    assert plane.shape == frames[0].shape and np.array_equal(plane, out[0])


def test_flat_frames_and_dc_steps():
    """a flat block has one non-zero coefficient, DC = 8 v: with the level shift a DC step s maps v to
    128 + rint((8 v - 1024) / s) s / 8 - 128 itself is a fixed point of every table"""
    for name, table in cl.TABLES.items():
        out = cl.model_requantise(np.full((8, 8), 128, np.uint8), table)
        assert (out == 128).all(), name
    out = cl.model_requantise(np.full((8, 8), 255, np.uint8), cl.TABLES["dc200"])
    assert (out == 253).all()             # 8 * 127 / 200 = 5.08 -> 5 * 200 / 8 = 125


# ---- 4. what the GPU test's inputs exercise ---------------------------------------------------------------------------------
def test_the_gpu_tests_inputs_meet_ties_and_saturate():
    """Over the frames and tables of tests/test_requantise_gpu.py (channel_lib.gpu_cases x channel_lib.TABLES, content seed 11)
    the model meets quantiser inputs exactly on k + 1/2, inverse outputs exactly on k + 1/2 and pixels beyond either end of
    [0, 255] - on the noise and stego frames alone as well as with the flat ones (whose rows tie in every pixel)."""
    total = dict(q_ties=0, p_ties=0, low=0, high=0)
    textured = dict(total)
    print("| table | quantiser ties | pixel ties | below 0 | above 255 |  (flat frames left out)")
    for name, table in cl.TABLES.items():
        row = dict.fromkeys(total, 0)
        for _, kind, frames in cl.gpu_cases():
            counts = {}
            cl.model_requantise(frames, table, counts)
            for k, v in counts.items():
                total[k] += v
                if kind != "flat":
                    textured[k] += v
                    row[k] += v
        print(f"| {name} | {row['q_ties']} | {row['p_ties']} | {row['low']} | {row['high']} |")
    print("all:", total, " without the flat frames:", textured)
    for counts in (total, textured):
        assert counts["q_ties"] >= 50 and counts["p_ties"] >= 3, counts
        assert counts["low"] >= 10 and counts["high"] >= 10, counts


def test_the_host_build_of_the_block_body_is_the_model(tmp_path):
    """csrc/svs_block.hpp requantise_block_exact - what a lane of the kernel runs - compiled for the host, on every frame and
    table of the GPU test: the model's bytes, ties and saturation included"""
    emu = build_emu("channel_emu.cpp", {"channel_emu_blocks": (None, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])}, tmp_path,
                    ("-ffp-contract=off",)).channel_emu_blocks
    for _, kind, frames in cl.gpu_cases():
        f, h, w = frames.shape
        blocks = np.ascontiguousarray(frames.reshape(f, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4))
        for name, table in cl.TABLES.items():
            out = np.empty_like(blocks)
            steps = np.ascontiguousarray(table, np.uint16)
            emu(blocks.ctypes.data, out.ctypes.data, blocks.size // 64, steps.ctypes.data)
            got = out.transpose(0, 1, 3, 2, 4).reshape(f, h, w)
            assert np.array_equal(got, cl.model_requantise(frames, table)), (frames.shape, kind, name)


# ---- 5. the README's table --------------------------------------------------------------------------------------------------
def test_survival_table():
    """Fixed seeds (channel_lib.survival).  The asserted row is delta = 20, n = 10, reference rule: no error down to quality 85,
    and at 75 the copies fail together - the hard majority is no better than a copy alone - while the soft vote removes more
    than half of the errors.  The others are printed for the README's table."""
    rows = {}
    for label, delta, n, index in cl.SETTINGS:
        print(f"\ndelta, n = {label}: errors of each copy alone, hard majority, soft vote (of {12 * 20 * n} bits)")
        print("| rule | " + " | ".join(f"Q = {q}" for q in cl.QUALITIES) + " |")
        print("|---|" + "---|" * len(cl.QUALITIES))
        for rule in cl.RULES:
            cells = []
            for quality in cl.QUALITIES:
                r = rows[(label, rule, quality)] = cl.survival(delta, n, index, rule, quality)
                cells.append(f"{' / '.join(str(e) for e in r['single'])}, {r['majority']}, {r['soft']}")
            print(f"| {rule} | " + " | ".join(cells) + " |")
    r100 = cl.survival(20, 10, None, "reference", 100)
    assert r100["single"] == [0, 0, 0] and all(s == 1.0 for s in r100["share"])
    for quality in (95, 90, 85):
        assert rows[("20, 10", "reference", quality)]["single"] == [0, 0, 0], quality
    r = rows[("20, 10", "reference", 75)]
    assert min(r["single"]) > 100
    assert r["majority"] >= min(r["single"])
    assert 2 * r["soft"] < min(r["single"]), r
    assert max(r["share"]) < 0.9
