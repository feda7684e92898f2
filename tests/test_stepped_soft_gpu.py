"""Soft bytes, the fused vote and the fused histograms under per-coefficient steps on the GPU (svs_stepped_soft_*,
include/svsdct.h): the device output against the NumPy model of the byte (tests/stepped_soft_lib.py) byte for byte - no tolerance:
the model is pocketfft and the exact kernels are pocketfft-identical -, uniform tables against the existing soft, vote and
histogram calls of the same build, the vote across the periods at which its tail takes another path, the histogram across the
frame split and the workgroup edge, the host forms across staging chunk sizes, one round trip through the channel, and the
refusals through the C ABI."""
import ctypes as C
import functools

import numpy as np
import pytest

import soft_histogram_lib as hl
import stepped_lib as st
import stepped_soft_lib as ss
from test_gpu_parity import _Dev
from testlib import experiments_library, using_library
from svsdct import batch, native, soft, steps
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

PAD = 0xAB
GUARD = 64
TABLES = ("u20", "u16", "u7", "m75x2", "odd")
LAYOUTS = [(s, False) for s in st.SHAPES] + [(st.PITCHED, True)]
LAYOUT_IDS = [s + ("_pitched" if p else "") for s, p in LAYOUTS]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    if kind == "stego":          # stepped stego: mid noise with a payload under matched(75, 2), plain options
        cover = st.content("mid", st.SHAPES[shape])
        frames = st.model_batch_embed(cover, st.TABLES["m75x2"], st.payload_for(st.SHAPES[shape]), st.N_AC, "nearest")[0]
    else:
        frames = st.content(kind, st.SHAPES[shape])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def model_of(shape, kind, table, option, n_ac=st.N_AC):
    order_key, index, key = st.OPTIONS[option]
    out = ss.model_batch_soft(frames_of(shape, kind), st.TABLES[table], n_ac, index, key, st.FIRST_FRAME, order_key)
    out.setflags(write=False)
    return out


def geometry(frames, pitched):
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    return Planes(f, h, w, 0, row_pitch, frame_pitch)


def planted(frames, planes):
    host = np.full(planes.n_frames * planes.frame_pitch, PAD, np.uint8)
    np.lib.stride_tricks.as_strided(host, (planes.n_frames, planes.height, planes.width), (planes.frame_pitch, planes.row_pitch, 1))[...] = frames
    return host


def on_device(frames, pitched=False):
    planes = geometry(frames, pitched)
    d = _Dev(planes.n_frames * planes.frame_pitch)
    d.put(planted(frames, planes))
    return d, planes


def keywords(option, table=None, histogram=False):
    order_key, index, key = st.OPTIONS[option]
    kw = dict(coeffs=list(index) if index is not None else None, dither_key=key, first_frame=st.FIRST_FRAME)
    if not histogram:
        kw["order"] = batch.block_order(order_key, st.FIRST_FRAME) if order_key is not None else None
    if table is not None:
        kw["steps"] = table
    return kw


def sync():
    native.check(native.load().svs_stream_synchronize(None), "sync")


def capacity(frames, n_ac=st.N_AC):
    return frames.shape[0] * (frames.shape[1] // 8) * (frames.shape[2] // 8) * n_ac


def device_soft(frames, delta, pitched=False, n_ac=st.N_AC, **kw):
    """one extract_soft_device call -> the bytes; exactly the capacity is written, the guard behind it is untouched"""
    d_in, planes = on_device(frames, pitched)
    cap = capacity(frames, n_ac)
    size = cap + (-cap) % 4 + GUARD
    d_out = _Dev(size)
    d_out.put(np.full(size, PAD, np.uint8))
    got = batch.extract_soft_device(d_in.ptr.value, planes, delta, n_ac, d_out.ptr.value, cap + (-cap) % 4, **kw)
    sync()
    out = d_out.get()
    assert got == cap
    assert (out[cap:] == PAD).all(), "the soft call wrote past its capacity"
    return out[:cap]


def device_vote(frames, delta, period, stream_bit0=0, pitched=False, n_ac=st.N_AC, d_tally=None, **kw):
    """one extract_vote_device call into a zeroed tally (or d_tally) with a guard entry behind it -> (tally, the device buffer)"""
    d_in, planes = on_device(frames, pitched)
    if d_tally is None:
        d_tally = _Dev(4 * (period + 4))
        d_tally.put(np.concatenate([np.zeros(period, np.int32), np.full(4, 0x5A5A5A5A, np.int32)]))
    got = batch.extract_vote_device(d_in.ptr.value, planes, delta, n_ac, d_tally.ptr.value, period, stream_bit0, **kw)
    sync()
    out = d_tally.get(dtype=np.int32)
    assert got == capacity(frames, n_ac)
    assert (out[period:] == 0x5A5A5A5A).all(), "the vote wrote past its tally"
    return out[:period].copy(), d_tally


def device_hist(frames, delta, pitched=False, n_ac=st.N_AC, start=None, **kw):
    d_in, planes = on_device(frames, pitched)
    f = frames.shape[0]
    d_hist = _Dev(1024 * f + 16)
    first = np.zeros((f, 256), np.uint32) if start is None else start
    d_hist.put(np.concatenate([first.reshape(-1), np.full(4, 0x5A5A5A5A, np.uint32)]))
    got = batch.extract_histogram_device(d_in.ptr.value, planes, delta, n_ac, d_hist.ptr.value, **kw)
    sync()
    out = d_hist.get(dtype=np.uint32)
    assert got == capacity(frames, n_ac)
    assert (out[256 * f:] == 0x5A5A5A5A).all(), "the histogram wrote past its rows"
    return out[: 256 * f].reshape(f, 256).copy()


def first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return "no difference" if not len(bad) else f"{len(bad)} of {want.size} differ, first at {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"


# ---- 1. the device is the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", st.CONTENTS + ("stego",))
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_the_device_is_the_model(shape, pitched, kind):
    """svs_stepped_soft_extract_dev under the uniform tables 20, 16 and 7, matched(75, 2) and the odd-step table x plain, order,
    select, dither, all at n_ac = 10: exactly the capacity in bytes, each the model's"""
    frames = frames_of(shape, kind)
    for table in TABLES:
        for option in st.OPTIONS:
            want = model_of(shape, kind, table, option)
            got = device_soft(frames, 1.0, pitched, **keywords(option, st.TABLES[table]))
            assert np.array_equal(got, want), (shape, pitched, kind, table, option, first_difference(got, want))


def test_the_device_is_the_model_at_63_coefficients():
    frames = frames_of("odd", "full")
    for option in ("plain", "dither"):
        order_key, index, key = st.OPTIONS[option]
        want = ss.model_batch_soft(frames, st.TABLES["odd"], 63, None, key, st.FIRST_FRAME, order_key)
        got = device_soft(frames, 1.0, n_ac=63, **keywords(option, st.TABLES["odd"]))
        assert np.array_equal(got, want), (option, first_difference(got, want))


# ---- 2. the uniform identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(st.UNIFORM))
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_a_uniform_table_is_the_existing_call(shape, pitched, name):
    """every delta[k] = D against delta = D: bytes, tally entries and counts equal exactly.  D = 16 runs the same instantiation
    on both sides (the existing call multiplies by 1 / 16 where the stepped side divides)."""
    d = st.UNIFORM[name]
    table = st.TABLES[name]
    for kind in ("full", "flat"):
        frames = frames_of(shape, kind)
        cap = capacity(frames)
        for option in ("plain", "all"):
            where = (shape, pitched, name, kind, option)
            got = device_soft(frames, 1.0, pitched, **keywords(option, table))
            want = device_soft(frames, d, pitched, **keywords(option))
            assert np.array_equal(got, want), (where, first_difference(got, want))
            period = max(1, cap // 3)
            got_t, _ = device_vote(frames, 1.0, period, 5, pitched, **keywords(option, table))
            want_t, _ = device_vote(frames, d, period, 5, pitched, **keywords(option))
            assert np.array_equal(got_t, want_t), (where, first_difference(got_t, want_t))
            got_h = device_hist(frames, 1.0, pitched, **keywords(option, table, histogram=True))
            want_h = device_hist(frames, d, pitched, **keywords(option, histogram=True))
            assert np.array_equal(got_h, want_h), (where, first_difference(got_h, want_h))


# ---- 3. the vote --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["plain", "order", "all"])
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=LAYOUT_IDS)
def test_the_vote_is_the_tally_of_the_model_bytes(shape, pitched, option):
    """n_ac = 10: a wave's run is 640 bytes.  Periods 1, 7, 65, 641, capacity / 3 and capacity + 5 cover the per-entry sums of the
    keyed tail (period <= 64) and of the raster tail (below 640) and both their complements; stream_bit0 0 and not 0"""
    frames = frames_of(shape, "full")
    table = st.TABLES["m75x2"]
    want_bytes = model_of(shape, "full", "m75x2", option)
    cap = want_bytes.size
    for period in sorted({1, 7, 65, 641, max(1, cap // 3), cap + 5}):
        for bit0 in (0, 12_345):
            want = ss.model_tally(want_bytes, period, bit0)
            got, _ = device_vote(frames, 1.0, period, bit0, pitched, **keywords(option, table))
            assert np.array_equal(got, want), (shape, pitched, option, period, bit0, first_difference(got, want))


def test_a_clip_voted_in_two_batches_is_the_clip_voted_in_one():
    frames = frames_of("even", "stego")
    table = st.TABLES["m75x2"]
    per_frame = capacity(frames[:1])
    period = capacity(frames) // 3 - 7
    for option in ("plain", "all"):
        kw = keywords(option, table)
        whole, _ = device_vote(frames, 1.0, period, 0, **kw)
        _, d_tally = device_vote(frames[:1], 1.0, period, 0, **kw)
        later = dict(kw, first_frame=st.FIRST_FRAME + 1)
        if kw["order"] is not None:
            later["order"] = batch.block_order(st.OPTIONS[option][0], st.FIRST_FRAME + 1)
        both, _ = device_vote(frames[1:], 1.0, period, per_frame, d_tally=d_tally, **later)
        assert np.array_equal(both, whole), (option, first_difference(both, whole))
        want_bits, _ = soft.combine(np.asarray(model_of("even", "stego", "m75x2", option)), period)
        assert np.array_equal(soft.tally_bits(whole), want_bits), option


# ---- 4. the histogram -----------------------------------------------------------------------------------------------------------
HIST_SHAPES = [("stepped", s) for s in st.SHAPES] + [("hist", "straddle"), ("hist", "past_workgroup_edge")]


@pytest.mark.parametrize("family,shape", HIST_SHAPES, ids=[s for _, s in HIST_SHAPES])
def test_the_histogram_is_the_byte_histogram_of_the_soft_bytes(family, shape):
    """the rows equal soft.byte_histogram of the soft call's bytes and of the model's, each row sums to its frame's capacity, and a
    call into non-zero rows adds.  (5, 64, 120): frames split inside a workgroup; (3, 8, 2056): 257 blocks a frame."""
    dims = st.SHAPES[shape] if family == "stepped" else hl.SHAPES[shape]
    frames = np.random.default_rng(len(shape)).integers(0, 256, dims).astype(np.uint8)
    f = dims[0]
    for table, option in (("m75x2", "plain"), ("odd", "select"), ("m75x2", "dither")):
        kw = keywords(option, st.TABLES[table], histogram=True)
        order_key, index, key = st.OPTIONS[option]
        want = ss.model_hist(ss.model_batch_soft(frames, st.TABLES[table], st.N_AC, index, key, st.FIRST_FRAME), f)
        soft_kw = dict(kw, order=None)
        assert np.array_equal(soft.byte_histogram(device_soft(frames, 1.0, **soft_kw), f), want), (shape, table, option)
        got = device_hist(frames, 1.0, **kw)
        assert np.array_equal(got, want), (shape, table, option, first_difference(got, want))
        assert (got.sum(axis=1) == capacity(frames[:1])).all()
        start = np.arange(f * 256, dtype=np.uint32).reshape(f, 256) * 3 + 1
        again = device_hist(frames, 1.0, start=start, **kw)
        assert np.array_equal(again, want + start), (shape, table, option)


def test_a_frame_embedded_under_an_order_reads_the_same_rows():
    cover = st.content("mid", st.SHAPES["odd"])
    table = st.TABLES["m75x2"]
    payload = st.payload_for(st.SHAPES["odd"])
    plain = st.model_batch_embed(cover, table, payload, st.N_AC, "reference", None, st.DITHER_KEY, st.FIRST_FRAME, None)[0]
    ordered = st.model_batch_embed(cover, table, payload, st.N_AC, "reference", None, st.DITHER_KEY, st.FIRST_FRAME, st.ORDER_KEY)[0]
    kw = dict(dither_key=st.DITHER_KEY, first_frame=st.FIRST_FRAME, steps=table)
    rows = device_hist(ordered, 1.0, **kw)
    under_order = ss.model_batch_soft(ordered, table, st.N_AC, None, st.DITHER_KEY, st.FIRST_FRAME, st.ORDER_KEY)
    assert np.array_equal(rows, soft.byte_histogram(under_order, cover.shape[0]))
    assert soft.lattice_share(rows).min() > 0.9 and soft.lattice_share(device_hist(plain, 1.0, **kw)).min() > 0.9


# ---- 5. the host forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_kb", [8, 32, 4096])
@pytest.mark.parametrize("option", ["plain", "all"])
def test_the_host_forms_equal_the_device_forms_across_staging_chunks(option, chunk_kb, monkeypatch):
    exp = experiments_library()
    monkeypatch.setenv("SVS_STAGE_CHUNK_KB", str(chunk_kb))
    f, h, w = 5, 64, 136
    frames = np.random.default_rng(chunk_kb).integers(0, 256, (f, h, w)).astype(np.uint8)
    order_key, index, key = st.OPTIONS[option]
    table = st.TABLES["m75x2"]
    want = ss.model_batch_soft(frames, table, st.N_AC, index, key, st.FIRST_FRAME, order_key)
    period = want.size // 3 + 1
    kw = dict(first_frame=st.FIRST_FRAME, coeffs=list(index) if index else None, dither_key=key, steps=table)
    with using_library(exp):
        got, n = batch.extract_soft_frames(frames, 1.0, st.N_AC, block_key=order_key, **kw)
        bits, tally = batch.extract_vote_frames(frames, 1.0, st.N_AC, period, 9, block_key=order_key, **kw)
        hist, counted = batch.extract_histogram_frames(frames, 1.0, st.N_AC, **kw)
    assert n == counted == want.size and np.array_equal(got, want), first_difference(got, want)
    assert np.array_equal(tally, ss.model_tally(want, period, 9)) and np.array_equal(bits, soft.tally_bits(tally))
    raster = ss.model_batch_soft(frames, table, st.N_AC, index, key, st.FIRST_FRAME)
    assert np.array_equal(hist, ss.model_hist(raster, f))
    assert np.array_equal(device_soft(frames, 1.0, **keywords(option, table)), got)
    assert np.array_equal(device_vote(frames, 1.0, period, 9, **keywords(option, table))[0], tally)
    assert np.array_equal(device_hist(frames, 1.0, **keywords(option, table, histogram=True)), hist)


# ---- 6. embed, channel, vote: the number of the model -------------------------------------------------------------------------
def test_round_trip_through_the_channel_on_the_device():
    """embed_repeated_frames(steps=matched(75, 2)) -> requantise_frames at quality 40 -> extract_vote_frames(steps=...) on three
    96 x 160 frames: the vote's error count is the CPU model's for the same seeds, exactly (71, README.md)"""
    index = st.ROW_1_10
    table = st.matched(75, 2)
    cover, payload = ss.survival_clip(index)
    want = ss.survival(table, index, "reference", qualities=(40,))[40]
    stego, used, period = batch.embed_repeated_frames(cover, 1.0, 10, payload, coeffs=list(index), steps=table)
    assert used == 3 * payload.size and period == payload.size
    through = batch.requantise_frames(stego, 40)
    bits, tally = batch.extract_vote_frames(through, 1.0, 10, period, coeffs=list(index), steps=table)
    errors = int((bits != payload).sum())
    got_soft, _ = batch.extract_soft_frames(through, 1.0, 10, coeffs=list(index), steps=table)
    single = [int((b != payload).sum()) for b in (np.asarray(got_soft) >> 7).reshape(3, -1)]
    print("per copy", single, "soft vote", errors, "model", want)
    assert single == want[0] and errors == want[2]


# ---- 7. refusals through the C ABI, each leaving the outputs untouched ------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    lib = native.load()
    frames = frames_of("odd", "full")
    d_in, planes = on_device(frames)
    cap = capacity(frames)
    d_out = _Dev(cap + 64)
    fill = np.full(cap + 64, PAD, np.uint8)
    d_out.put(fill)
    table = steps.steps_struct(st.uniform(20))
    INVALID = native.SVS_ERR_INVALID_ARG

    def calls(names, steps_ptr, flags=0, period=7, out_offset=0, out_capacity=cap + 64):
        """-> [(name, return code, *n_bits_out after the call)] of the named device calls, each with its own n_bits_out of 12345"""
        out = d_out.ptr.value + out_offset
        made = []
        for name in names:
            done = C.c_uint64(12345)
            if name == "extract":
                rc = lib.svs_stepped_soft_extract_dev(d_in.ptr, C.byref(planes), None, None, None, steps_ptr, 10, out, out_capacity, flags,
                                                      C.byref(done), None)
            elif name == "vote":
                rc = lib.svs_stepped_soft_vote_dev(d_in.ptr, C.byref(planes), None, None, None, steps_ptr, 10, period, 0, out, flags,
                                                   C.byref(done), None)
            else:
                rc = lib.svs_stepped_soft_histogram_dev(d_in.ptr, C.byref(planes), None, None, steps_ptr, 10, out, flags, C.byref(done), None)
            made.append((name, rc, lib.svs_last_error().decode(), int(done.value)))
        return made

    def refused(what, names=("extract", "vote", "histogram"), message=None, late=False, code=INVALID, **kw):
        """late: a refusal behind the geometry.  There svs_soft_extract_dev has cleared *n_bits_out already, and so has the stepped
        call (include/svsdct.h: a refusal leaves *n_bits_out as it was WHERE THE EXISTING CALL DOES); a tally or a histogram call
        never touches it before it succeeds."""
        for name, rc, msg, done in calls(names, **kw):
            assert rc == code and done == (0 if late and name == "extract" else 12345), (what, name, rc, msg, done)
            if message:
                assert message in msg, (what, name, msg)
        sync()
        assert np.array_equal(d_out.get(), fill), (what, "a refused call wrote to its output")

    refused("NULL steps", steps_ptr=None, message="steps is NULL")
    for k, v in ((1, 0), (63, 4096)):
        bad = steps.steps_struct(st.uniform(20))
        bad.delta[k] = v
        refused(f"entry {v}", steps_ptr=C.byref(bad), message=f"delta[{k}] = {v}")
    refused("an embed flag", steps_ptr=C.byref(table), flags=batch.embed_flags(None, nearest=True) & ~batch.mode_flags(None) or 4,
            message="mode bits only")
    refused("period 0", ("vote",), steps_ptr=C.byref(table), period=0, message="period is 0")
    refused("an unaligned output", steps_ptr=C.byref(table), out_offset=2, message="4-byte aligned", late=True)
    refused("a capacity above the output's", ("extract",), steps_ptr=C.byref(table), out_capacity=cap - 1, late=True,
            code=native.SVS_ERR_CAPACITY, message=f"needs {cap} bytes")
    # the existing soft call at the same arguments: the same return code and the same *n_bits_out
    for out, out_capacity, code in ((d_out.ptr.value + 2, cap + 64, INVALID), (d_out.ptr.value, cap - 1, native.SVS_ERR_CAPACITY)):
        done = C.c_uint64(12345)
        rc = lib.svs_soft_extract_dev(d_in.ptr, C.byref(planes), None, None, None, 20.0, 10, out, out_capacity, 0, C.byref(done), None)
        assert rc == code and done.value == 0
    # and the accepted call still runs: the mode bits change nothing
    for name, rc, msg, done in calls(("extract", "vote", "histogram"), C.byref(table), flags=batch.mode_flags("exact")):
        assert rc == 0 and done == cap, (name, rc, msg)
    sync()
