"""The fused per-frame soft histograms on the GPU (svs_soft_histogram_dev / svs_soft_histogram, include/svsdct.h): the rows of
the device call against soft.byte_histogram of the NumPy model's bytes and of svs_soft_extract_dev's own bytes - exact integer
equality, no tolerance - on the smallest shapes at which the split of a workgroup's blocks into frames can go wrong; that the
rows do not depend on a keyed order; batches that add into rows on top of what is there; the host call; what a histogram call
leaves behind; and the use: which frames of a clip carry a payload."""
import ctypes as C

import numpy as np
import pytest

import dither_lib as dl
import soft_histogram_lib as hl
import soft_lib as sl
import test_soft_extract_gpu as se
from test_gpu_parity import _Dev
from svsdct import batch, native
from svsdct import soft as sv
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

KEY, ORDER_KEY, FIRST = se.KEY, se.ORDER_KEY, se.FIRST
SHAPES = hl.SHAPES
FORMS = ("plain", "zigzag", "dither", "zigzag_dither")
DELTAS = (8, 20, 12.5, 0.1)
N_ACS = (1, 3, 10, 63, 70, 0)          # 70 clamps, 0 is a capacity of 0
GUARD = 16                             # sentinel uint32 values before and behind the rows
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def form_args(form, n):
    """-> (soft_lib / Planted keywords, batch keywords) of a form at n coefficients"""
    n = max(0, min(n, 63))
    index = sl.zigzag(n) if form.startswith("zigzag") and n else None
    key = KEY if form.endswith("dither") else None
    first = FIRST if key is not None else 0
    return dict(index=index, key=key, first_frame=first), dict(coeffs=index, dither_key=key, first_frame=first)


_inputs = {}


def frames_of(shape, delta):
    """as test_soft_extract_gpu.frames_of: a SVS_MINMOVE stego (n_ac = 10, the library's own embed call) whose budget ends
    inside a frame and inside a block, over noise in [0, 256).  One per shape and delta, shared and never written to."""
    if (shape, delta) not in _inputs:
        f, h, w = SHAPES[shape]
        cover = dl.noise((f, h, w), 0, 256, seed=len(shape))
        cap = batch.capacity_bits(f, h, w, 10)
        stego, used = batch.embed_frames(cover, delta, 10, dl.payload(cap - cap // (2 * f) - 3, seed=1), minmove=True)
        assert used == cap - cap // (2 * f) - 3
        stego = np.array(stego)
        stego.setflags(write=False)
        _inputs[(shape, delta)] = stego
    return _inputs[(shape, delta)]


class Planted:
    """the frames of a stack on the device, tight or pitched with 0xAB in the padding, and rows of counts between sentinels"""

    def __init__(self, frames, pitched=False):
        self.frames = frames
        f, h, w = frames.shape
        row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
        self.planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
        self.host = np.full(f * frame_pitch, 0xAB, np.uint8)
        np.lib.stride_tricks.as_strided(self.host, (f, h, w), (frame_pitch, row_pitch, 1))[...] = frames
        self.d = _Dev(self.host.size)
        self.d.put(self.host)
        self.size = 256 * f
        self.d_hist = _Dev(4 * (self.size + 2 * GUARD))

    def sub(self, f0, f1):
        """(device address, planes) of frames f0 .. f1 - 1"""
        p = self.planes
        return self.d.ptr.value + f0 * p.frame_pitch, Planes(f1 - f0, p.height, p.width, 0, p.row_pitch, p.frame_pitch)

    def start(self, fill=None):
        buf = np.full(self.size + 2 * GUARD, SENTINEL, np.uint32)
        buf[GUARD: GUARD + self.size] = 0 if fill is None else fill
        self.d_hist.put(buf)

    def count(self, delta, n, index=None, key=None, first_frame=0, frames=None, flags=0):
        """one svs_soft_histogram_dev into the rows as they stand -> the capacity the call reports"""
        lib = native.load()
        f0 = 0 if frames is None else frames[0]
        ptr, planes = (self.d.ptr.value, self.planes) if frames is None else self.sub(*frames)
        dith = None if key is None else native.Dither(key, first_frame, 0)
        sel = None if index is None else native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
        ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
        got = C.c_uint64(0xDEAD)
        native.check(lib.svs_soft_histogram_dev(ptr, C.byref(planes), ref(sel), ref(dith), float(delta), n,
                                                self.d_hist.ptr.value + 4 * (GUARD + 256 * f0), flags, C.byref(got), None),
                     "svs_soft_histogram_dev")
        return int(got.value)

    def finish(self):
        """-> the rows [n_frames, 256]; the sentinels around them must have survived"""
        native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
        buf = self.d_hist.get(4 * (self.size + 2 * GUARD), np.uint32)
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + self.size:] == SENTINEL).all(), "the call wrote outside the rows"
        return buf[GUARD: GUARD + self.size].reshape(-1, 256)

    def planes_unchanged(self):
        return np.array_equal(self.d.get(), self.host)


def first_difference(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if not bad.size:
        return "no difference"
    f, v = bad[0]
    return f"{len(bad)} entries differ, first at frame {f}, byte {v}: {got[f, v]} != {want[f, v]}"


def test_the_shapes_are_the_issues():
    blocks = {k: (h // 8) * (w // 8) for k, (f, h, w) in SHAPES.items()}
    assert blocks == dict(one_block=1, one_block_frames=1, tight=6, pitched=6, straddle=120, wave_edge=64, workgroup_edge=256,
                          past_workgroup_edge=257)
    assert SHAPES["one_block_frames"][0] == 70 and SHAPES["straddle"][0] * 120 % 256 == 88      # 64 + 6 frames; a ragged tail


# ---- 1. equality with the model and with the soft call ------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_rows_are_the_models_and_those_of_the_soft_calls_bytes(shape, form):
    f, h, w = SHAPES[shape]
    pitched = shape == "pitched"
    for delta in DELTAS:
        frames = frames_of(shape, delta)
        planted = Planted(frames, pitched)
        for n in N_ACS:
            model_kw, _ = form_args(form, n)
            what = (shape, form, delta, n)
            count = max(0, min(n, 63))
            if count == 0:
                # a capacity of 0: SVS_OK, nothing counted, the rows as they were
                pattern = (np.arange(planted.size, dtype=np.uint32) * 7 + 3)
                planted.start(pattern)
                assert planted.count(delta, n, **model_kw) == 0, what
                assert np.array_equal(planted.finish().ravel(), pattern), what
                continue
            model = sl.model_batch_soft(frames, delta, n, **model_kw)
            soft = se.dev_soft(frames, delta, n, pitched=pitched, **model_kw)
            assert np.array_equal(soft, model), what
            want = sv.byte_histogram(model, f)
            planted.start()
            assert planted.count(delta, n, **model_kw) == model.size == f * (h // 8) * (w // 8) * count, what
            got = planted.finish()
            assert np.array_equal(got, want), (what, first_difference(got, want))
            assert np.array_equal(got, sv.byte_histogram(soft, f)), what
            assert (got.sum(1) == model.size // f).all()
            assert np.array_equal(sv.margins(got), sv.margin_histogram(model, f)), what
        assert planted.planes_unchanged(), (shape, form, delta, "the call wrote to its planes")


def test_the_mode_bits_change_nothing():
    frames = frames_of("straddle", 20)
    planted = Planted(frames)
    want = sv.byte_histogram(sl.model_batch_soft(frames, 20, 10), 5)
    for flags in (native.SVS_EXACT_POCKETFFT, native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED):
        planted.start()
        assert planted.count(20, 10, flags=flags) == 6000
        assert np.array_equal(planted.finish(), want), flags


# ---- 2. the rows do not depend on a keyed order -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("straddle", "past_workgroup_edge", "one_block_frames"))
def test_a_clip_read_under_a_keyed_order_has_the_same_rows(shape):
    f = SHAPES[shape][0]
    frames = frames_of(shape, 20)
    planted = Planted(frames)
    for n in (3, 10, 63):
        for key in (None, KEY):
            ordered = se.dev_soft(frames, 20, n, key=key, order_key=ORDER_KEY, first_frame=FIRST)      # svs_soft_extract_dev
            raster = se.dev_soft(frames, 20, n, key=key, first_frame=FIRST)
            assert shape == "one_block_frames" or not np.array_equal(ordered, raster)                   # the order does permute
            planted.start()
            assert planted.count(20, n, key=key, first_frame=FIRST) == ordered.size
            got = planted.finish()
            assert np.array_equal(got, sv.byte_histogram(ordered, f)), (shape, n, key, first_difference(got, sv.byte_histogram(ordered, f)))


# ---- 3. adds on top -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_batches_add_into_the_rows_on_top_of_what_is_there(form):
    frames = frames_of("straddle", 20)
    planted = Planted(frames)
    for n in (3, 10):
        model_kw, _ = form_args(form, n)
        want = sv.byte_histogram(sl.model_batch_soft(frames, 20, n, **model_kw), 5)
        later = dict(model_kw, first_frame=model_kw["first_frame"] + (2 if model_kw["key"] is not None else 0))
        pattern = (np.arange(planted.size, dtype=np.int64) * 2654435761 % 2001).astype(np.uint32)
        planted.start(pattern)
        cap2 = batch.capacity_bits(2, 64, 120, n)
        assert planted.count(20, n, frames=(0, 2), **model_kw) == cap2
        assert planted.count(20, n, frames=(2, 5), **later) == want.sum() - cap2
        got = planted.finish()
        assert np.array_equal(got - pattern.reshape(5, 256), want), (form, n)
        planted.start()
        assert planted.count(20, n, **model_kw) == want.sum()               # the one-call rows of all five frames
        assert planted.count(20, n, **model_kw) == want.sum()               # and once more on top
        assert np.array_equal(planted.finish(), 2 * want), (form, n)
    assert planted.planes_unchanged()


# ---- 4. the host form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_host_call_returns_the_device_calls_rows(shape):
    f = SHAPES[shape][0]
    frames = frames_of(shape, 20)
    planted = Planted(frames, shape == "pitched")
    for form in FORMS:
        for n in (3, 10, 63):
            model_kw, batch_kw = form_args(form, n)
            planted.start()
            cap = planted.count(20, n, **model_kw)
            want = planted.finish()
            hist, n_bits = batch.extract_histogram_frames(np.array(frames), 20, n, **batch_kw)
            assert hist.dtype == np.uint32 and hist.shape == (f, 256) and n_bits == cap
            assert np.array_equal(hist, want), (shape, form, n, first_difference(hist, want))
            # the staging context's rows are zeroed at the start of every call: the same call again gives the same counts
            assert np.array_equal(batch.extract_histogram_frames(np.array(frames), 20, n, **batch_kw)[0], want)
    hist, n_bits = batch.extract_histogram_frames(np.array(frames), 20, 0)        # a capacity of 0: the host form writes zeros
    assert n_bits == 0 and hist.shape == (f, 256) and not hist.any()


def test_the_host_call_on_a_stack_of_several_staging_chunks():
    """40 x 480 x 640 = 12.3 MB: above twice the smallest staging chunk of 4 MB (csrc/svs_stage.hpp), so the embed calls cut it
    into chunks; the histogram call stages whole frames - against numpy.bincount of svs_soft_extract's bytes"""
    f, h, w, n = 40, 480, 640, 10
    assert f * h * w > 2 * (4 << 20)
    frames = dl.noise((f, h, w), 16, 240, seed=40)
    hist, n_bits = batch.extract_histogram_frames(frames, 20, n, dither_key=KEY, first_frame=FIRST)
    soft, n_soft = batch.extract_soft_frames(frames, 20, n, dither_key=KEY, first_frame=FIRST)
    per = (h // 8) * (w // 8) * n
    assert n_bits == n_soft == f * per
    want = np.stack([np.bincount(soft[k * per: (k + 1) * per], minlength=256) for k in range(f)])
    assert np.array_equal(hist, want), first_difference(hist, want)
    assert np.array_equal(batch.extract_histogram_frames(frames, 20, n, dither_key=KEY, first_frame=FIRST)[0], want)


# ---- 5. nothing left behind --------------------------------------------------------------------------------------------------
def test_a_histogram_call_leaves_nothing_behind_for_the_hard_soft_and_vote_calls():
    """the same stream: hard call, histogram call, hard call again - for every hard entry the second hard result is the first,
    byte for byte - and a soft call and a vote call after a histogram call give the model's bytes and soft.tally of them"""
    lib = native.load()
    frames = np.array(frames_of("straddle", 20))
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in = _Dev(frames.nbytes)
    d_in.put(frames)
    d_tally, d_hist = _Dev(4 * 2400), _Dev(1024 * f)
    for entry in sorted(se.HARD_CALLS):
        for n in (3, 10, 63):
            hard_kw, soft_kw = se.HARD_CALLS[entry](n)
            cap = batch.capacity_bits(f, h, w, n)
            nbytes = (cap + 7) // 8
            d_hard, d_soft = _Dev(nbytes + 8), _Dev(cap + 8)
            kw = dict(coeffs=soft_kw.get("index"), dither_key=soft_kw.get("key"), first_frame=soft_kw.get("first_frame"))
            results = []
            for k in range(2):
                d_hard.put(np.full(nbytes + 8, 0x5A, np.uint8))
                assert batch.extract_device(d_in.ptr.value, planes, 20, n, d_hard.ptr.value, nbytes, **hard_kw) == cap
                if k == 0:
                    d_hist.put(np.zeros(256 * f, np.uint32))
                    assert batch.extract_histogram_device(d_in.ptr.value, planes, 20, n, d_hist.ptr.value, **kw) == cap
                native.check(lib.svs_stream_synchronize(None), "sync")
                results.append(d_hard.get())
            assert np.array_equal(results[0], results[1]), (entry, n)
            kw["order"] = hard_kw.get("order")
            assert batch.extract_soft_device(d_in.ptr.value, planes, 20, n, d_soft.ptr.value, cap, **kw) == cap
            d_tally.put(np.zeros(2400, np.int32))
            assert batch.extract_vote_device(d_in.ptr.value, planes, 20, n, d_tally.ptr.value, 2400, **kw) == cap
            native.check(lib.svs_stream_synchronize(None), "sync")
            soft = d_soft.get()[:cap]
            assert np.array_equal(soft, sl.model_batch_soft(frames, 20, n, **soft_kw)), (entry, n)
            assert np.array_equal(d_tally.get(dtype=np.int32), sv.tally(soft, 2400)), (entry, n)
            assert np.array_equal(d_hist.get(dtype=np.uint32).reshape(f, 256), sv.byte_histogram(soft, f)), (entry, n)


# ---- 6. the use -------------------------------------------------------------------------------------------------------------
def test_the_frames_that_carry_a_payload_stand_out_with_the_key_only():
    """examples/find_payload_frames.py as an assertion, on the frames tests/test_soft_histogram_cpu.py holds the model to: with
    the key the share of m >= 64 is 1.0 on frames 2..4 and within 0.45 .. 0.55 elsewhere; without it within 0.45 .. 0.55 on all
    eight (the README's 0.492 / 0.500 with room for 12 000 bytes a frame: 0.05 is eleven standard deviations)"""
    s = hl.SCENARIO
    clip = hl.scenario_cover()
    lo, hi = s["first"], s["last"] + 1
    stego, used = batch.embed_frames(clip[lo:hi], s["delta"], s["n_ac"], hl.scenario_payload(), dither_key=s["key"], first_frame=lo)
    assert used == hl.scenario_payload().size
    clip[lo:hi] = stego
    assert np.array_equal(clip, hl.scenario_stego_model())                      # the frames the CPU tier checked
    keyed, n_bits = batch.extract_histogram_frames(clip, s["delta"], s["n_ac"], dither_key=s["key"])
    keyless, _ = batch.extract_histogram_frames(clip, s["delta"], s["n_ac"])
    assert n_bits == batch.capacity_bits(s["frames"], s["height"], s["width"], s["n_ac"])
    with_key, without = sv.lattice_share(keyed), sv.lattice_share(keyless)
    print("lattice share with the key:", np.round(with_key, 3).tolist(), "without:", np.round(without, 3).tolist())
    hl.assert_scenario(with_key, without)
