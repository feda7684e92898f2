"""The fused soft vote on the GPU (svs_soft_vote_dev / svs_soft_vote, include/svsdct.h): the tally of the device call, on the
shapes, frames and forms of tests/test_soft_extract_gpu.py, against soft.tally of the NumPy model's bytes and of
svs_soft_extract_dev's own bytes - exact integer equality at every period at which the vote tail takes another path -; the
stream offset, batches that add into one tally, a pre-filled tally, the host call, what a vote call leaves behind, and the
round trip of a tiled payload under pixel noise."""
import ctypes as C

import numpy as np
import pytest

import soft_lib as sl
import soft_vote_lib as vl
import test_soft_extract_gpu as se
from test_gpu_parity import _Dev
from svsdct import batch, native
from svsdct import soft as sv
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

SHAPES, FORMS = se.SHAPES, se.FORMS
DELTAS = (8, 20, 12.5, 0.1)
N_ACS = (1, 3, 10, 63, 70, 0)          # 70 clamps, 0 is a capacity of 0
GUARD = 16                             # sentinel int32 values before and behind the tally
SENTINEL = 0x5A5A5A5A
MAX_PERIOD = 100_000


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


class Planted:
    """the frames of a stack on the device, tight or pitched with 0xAB in the padding, and one tally buffer with sentinels"""

    def __init__(self, frames, pitched=False):
        self.frames = frames
        f, h, w = frames.shape
        row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
        self.planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
        self.host = np.full(f * frame_pitch, 0xAB, np.uint8)
        np.lib.stride_tricks.as_strided(self.host, (f, h, w), (frame_pitch, row_pitch, 1))[...] = frames
        self.d = _Dev(self.host.size)
        self.d.put(self.host)
        self.d_tally = _Dev(4 * (MAX_PERIOD + 2 * GUARD))

    def sub(self, f0, f1):
        """(device address, planes) of frames f0 .. f1 - 1"""
        p = self.planes
        return self.d.ptr.value + f0 * p.frame_pitch, Planes(f1 - f0, p.height, p.width, 0, p.row_pitch, p.frame_pitch)

    def start(self, period, fill=None):
        buf = np.full(period + 2 * GUARD, SENTINEL, np.int32)
        buf[GUARD: GUARD + period] = 0 if fill is None else fill
        self.d_tally.put(buf)

    def vote(self, delta, n, period, stream_bit0=0, index=None, key=None, order_key=None, first_frame=0, frames=None):
        """one svs_soft_vote_dev into the tally as it stands -> the capacity the call reports"""
        lib = native.load()
        ptr, planes = (self.d.ptr.value, self.planes) if frames is None else self.sub(*frames)
        order = batch.block_order(order_key, first_frame)
        dith = None if key is None else native.Dither(key, first_frame, 0)
        sel = None if index is None else native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
        ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
        got = C.c_uint64(0xDEAD)
        native.check(lib.svs_soft_vote_dev(ptr, C.byref(planes), ref(order), ref(sel), ref(dith), float(delta), n, period, stream_bit0,
                                           self.d_tally.ptr.value + 4 * GUARD, 0, C.byref(got), None), "svs_soft_vote_dev")
        return int(got.value)

    def finish(self, period):
        """-> the tally; the sentinels around it must have survived"""
        native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
        buf = self.d_tally.get(4 * (period + 2 * GUARD), np.int32)
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + period:] == SENTINEL).all(), "the call wrote outside the tally"
        return buf[GUARD: GUARD + period]

    def planes_unchanged(self):
        return np.array_equal(self.d.get(), self.host)


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "no difference" if not bad.size else f"{bad.size} of {want.size} entries differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 1. equality with the model and with the soft call ------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_tally_is_the_models_and_that_of_the_soft_calls_bytes(shape, form):
    f, h, w = SHAPES[shape]
    for delta in DELTAS:
        frames = se.frames_of(shape, delta)
        planted = Planted(frames, pitched=shape == "pitched")
        for n in N_ACS:
            model_kw, batch_kw = se.form_args(form, n)
            count = max(0, min(n, 63))
            model = sl.model_batch_soft(frames, delta, n, **model_kw)
            soft = se.dev_soft(frames, delta, n, pitched=shape == "pitched", **model_kw)
            assert np.array_equal(soft, model)
            if count == 0:
                # a capacity of 0: SVS_OK, nothing voted, the tally as it was
                pattern = np.arange(7, dtype=np.int32) - 3
                planted.start(7, pattern)
                assert planted.vote(delta, n, 7, **model_kw) == 0
                assert np.array_equal(planted.finish(7), pattern)
                continue
            for period in vl.landmark_periods(f, h, w, count):
                what = (shape, form, delta, n, period)
                want = sv.tally(model, period)
                planted.start(period)
                assert planted.vote(delta, n, period, **model_kw) == model.size, what
                got = planted.finish(period)
                assert np.array_equal(got, want), (what, first_difference(got, want))
                assert np.array_equal(got, sv.tally(soft, period)), what
                if period <= model.size:
                    assert np.array_equal(sv.tally_bits(got), sv.combine(model, period)[0]), what
            assert planted.planes_unchanged(), (shape, form, delta, n, "the call wrote to its planes")


def test_the_periods_of_the_largest_shape_are_the_landmarks():
    """(5, 64, 120) at n = 10: a capacity of 6 000, a wave's run of 640 bytes, a frame of 1 200"""
    want = {1, 7, 10, 639, 640, 641, 1200, 1201, 2399, 5999, 6000, 6001, 100_000}
    assert want <= set(vl.landmark_periods(5, 64, 120, 10))
    assert max(vl.landmark_periods(5, 64, 120, 63)) <= MAX_PERIOD


@pytest.mark.parametrize("form", FORMS)
def test_the_host_call_returns_the_same_tally_and_combines_bits(form):
    frames = se.frames_of("three_workgroups", 20)
    for n in (3, 10, 63):
        model_kw, batch_kw = se.form_args(form, n)
        model = sl.model_batch_soft(frames, 20, n, **model_kw)
        for period in (1, 7, 64 * n - 1, 2399, model.size, model.size + 1):
            bits, tally = batch.extract_vote_frames(frames, 20, n, period, **batch_kw)
            assert tally.dtype == np.int32 and tally.shape == (period,) and bits.dtype == np.uint8
            assert np.array_equal(tally, sv.tally(model, period)), (form, n, period)
            assert np.array_equal(bits, sv.tally_bits(tally))
            if period <= model.size:
                assert np.array_equal(bits, sv.combine(model, period)[0]), (form, n, period)
        # the staging context's tally is zeroed at the start of every call: the same call again gives the same tally
        again = batch.extract_vote_frames(frames, 20, n, 7, stream_bit0=3, **batch_kw)[1]
        assert np.array_equal(again, sv.tally(model, 7, 3))
    bits, tally = batch.extract_vote_frames(frames, 20, 0, 5)        # a capacity of 0: the host form writes zeros
    assert not tally.any() and tally.shape == (5,) and not bits.any()


# ---- 2. the stream offset -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_stream_bit0(form):
    frames = se.frames_of("three_workgroups", 20)
    planted = Planted(frames)
    for n in (10, 63):
        model_kw, _ = se.form_args(form, n)
        model = sl.model_batch_soft(frames, 20, n, **model_kw)
        for period in (1, 7, 64, 65, 64 * n - 1, 64 * n + 1, 2399, model.size, MAX_PERIOD):
            for s in (5, period - 1, (1 << 32) + 3):
                planted.start(period)
                assert planted.vote(20, n, period, s, **model_kw) == model.size
                got, want = planted.finish(period), sv.tally(model, period, s)
                assert np.array_equal(got, want), (form, n, period, s, first_difference(got, want))


# ---- 3. batches, 4. adds and does not overwrite ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_batches_add_into_one_tally_on_top_of_what_is_there(form):
    frames = se.frames_of("three_workgroups", 20)
    planted = Planted(frames)
    for n in (3, 10):
        model_kw, _ = se.form_args(form, n)
        model = sl.model_batch_soft(frames, 20, n, **model_kw)
        cap2 = batch.capacity_bits(2, frames.shape[1], frames.shape[2], n)
        later = dict(model_kw, first_frame=model_kw["first_frame"] + (2 if form != "plain" and form != "zigzag" else 0))
        for period in (1, 7, 64 * n - 1, 1201, 2399, model.size // 3, model.size):
            pattern = (np.arange(period, dtype=np.int64) * 2654435761 % 2001 - 1000).astype(np.int32)
            planted.start(period, pattern)
            assert planted.vote(20, n, period, 0, frames=(0, 2), **model_kw) == cap2
            assert planted.vote(20, n, period, cap2, frames=(2, 5), **later) == model.size - cap2
            got = planted.finish(period)
            assert np.array_equal(got - pattern, sv.tally(model, period)), (form, n, period)
            planted.start(period)
            assert planted.vote(20, n, period, **model_kw) == model.size          # the one-call tally of all five frames
            assert np.array_equal(planted.finish(period), got - pattern), (form, n, period)
    assert planted.planes_unchanged()


# ---- 5. nothing left behind --------------------------------------------------------------------------------------------------
def test_a_vote_call_leaves_nothing_behind_for_the_hard_and_soft_calls():
    """the same stream: hard call, vote call, hard call again - for every hard entry the second hard result is the first, byte
    for byte - and a soft call after a vote call gives the model's bytes"""
    lib = native.load()
    frames = se.frames_of("three_workgroups", 20)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in = _Dev(frames.nbytes)
    d_in.put(frames)
    d_tally = _Dev(4 * 2400)
    for entry in sorted(se.HARD_CALLS):
        for n in (3, 10, 63):
            hard_kw, soft_kw = se.HARD_CALLS[entry](n)
            cap = batch.capacity_bits(f, h, w, n)
            nbytes = (cap + 7) // 8
            d_hard, d_soft = _Dev(nbytes + 8), _Dev(cap + 8)
            kw = dict(coeffs=soft_kw.get("index"), dither_key=soft_kw.get("key"), order=hard_kw.get("order"),
                      first_frame=soft_kw.get("first_frame"))
            results = []
            for k in range(2):
                d_hard.put(np.full(nbytes + 8, 0x5A, np.uint8))
                assert batch.extract_device(d_in.ptr.value, planes, 20, n, d_hard.ptr.value, nbytes, **hard_kw) == cap
                if k == 0:
                    d_tally.put(np.zeros(2400, np.int32))
                    assert batch.extract_vote_device(d_in.ptr.value, planes, 20, n, d_tally.ptr.value, 2400, **kw) == cap
                native.check(lib.svs_stream_synchronize(None), "sync")
                results.append(d_hard.get())
            assert np.array_equal(results[0], results[1]), (entry, n)
            assert batch.extract_soft_device(d_in.ptr.value, planes, 20, n, d_soft.ptr.value, cap, **kw) == cap
            native.check(lib.svs_stream_synchronize(None), "sync")
            soft = d_soft.get()[:cap]
            assert np.array_equal(soft, sl.model_batch_soft(frames, 20, n, **soft_kw)), (entry, n)
            assert np.array_equal(d_tally.get(dtype=np.int32), sv.tally(soft, 2400)), (entry, n)


# ---- 6. round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("plain", "all"))
def test_round_trip_of_three_copies_under_pixel_noise(form):
    rng = np.random.default_rng(17)
    cover = rng.integers(64, 192, (3, 96, 160)).astype(np.uint8)
    payload = rng.integers(0, 2, 2400).astype(np.uint8)
    _, kw = se.form_args(form, 10)
    stego, used, period = batch.embed_repeated_frames(cover, 20, 10, payload, copies=3, **kw)
    assert (used, period) == (7200, 2400)
    noisy = np.clip(stego.astype(np.int64) + rng.integers(-8, 9, stego.shape), 0, 255).astype(np.uint8)
    bits, tally = batch.extract_vote_frames(noisy, 20, 10, period, **kw)
    soft, n_bits = batch.extract_soft_frames(noisy, 20, 10, **kw)
    assert n_bits == 7200
    assert np.array_equal(bits, sv.combine(soft[:used], period)[0])
    assert np.array_equal(tally, sv.tally(soft[:used], period))
    clean = batch.extract_vote_frames(stego, 20, 10, period, **kw)[0]
    print(f"{form}: payload bit errors of the fused vote: {int((clean != payload).sum())} undisturbed, {int((bits != payload).sum())} at +-8")
    # copies=None fills the capacity; two copies and a half in a stack that holds 7 200 bits at a period of 2 880
    stego, used, period = batch.embed_repeated_frames(cover, 20, 10, rng.integers(0, 2, 2880).astype(np.uint8), **kw)
    assert (used, period) == (7200, 2880)
