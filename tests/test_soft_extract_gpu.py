"""Soft-decision extraction on the GPU (svs_soft_extract_dev / svs_soft_extract, include/svsdct.h): the device call on tight and
pitched planes and the host call against the NumPy model of soft_lib.py byte for byte, on the smallest shapes at which the
block -> (frame, slot) arithmetic and the wave tile of the soft side can go wrong; the identity of the hard bits with every hard
extract call; and that a soft call leaves nothing behind that a hard call reads."""
import ctypes as C

import numpy as np
import pytest

import dither_lib as dl
import soft_lib as sl
import tie_lib as tl
from test_gpu_parity import _Dev
from svsdct import batch, native
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

KEY = 0x0123456789ABCDEF
ORDER_KEY = 0xC0FFEE1234
FIRST = 5
# one block; two frames; three workgroups of 256 blocks with a ragged tail of 88 and waves that straddle frames (120 blocks per
# frame); row and frame padding
SHAPES = {"one_block": (1, 8, 8), "two_frames": (2, 16, 24), "three_workgroups": (5, 64, 120), "pitched": (2, 16, 24)}
N_ACS = (1, 3, 10, 63, 0, 70)          # 0 and 70 clamp
DELTAS = (8, 20, 12.5, 0.1, -1)
FORMS = ("plain", "zigzag", "dither", "order", "all")


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def form_args(form, n):
    """-> (model / soft_lib keywords, batch keywords) of a form at n coefficients"""
    n = max(0, min(n, 63))
    index = sl.zigzag(n) if form in ("zigzag", "all") and n else None
    key = KEY if form in ("dither", "all") else None
    okey = ORDER_KEY if form in ("order", "all") else None
    first = FIRST if key is not None or okey is not None else 0
    return (dict(index=index, key=key, order_key=okey, first_frame=first),
            dict(coeffs=index, dither_key=key, block_key=okey, first_frame=first))


_inputs = {}


def frames_of(shape, delta):
    """A SVS_MINMOVE stego (n_ac = 10, made by the library's own embed call) whose budget ends inside a frame and inside a
    block, over noise in [0, 256): the blocks past the budget are the raw noise.  One per shape and delta, shared."""
    if (shape, delta) not in _inputs:
        f, h, w = SHAPES[shape]
        cover = dl.noise((f, h, w), 0, 256, seed=len(shape))
        cap = batch.capacity_bits(f, h, w, 10)
        stego, used = batch.embed_frames(cover, delta, 10, dl.payload(cap - cap // (2 * f) - 3, seed=1), minmove=True)
        assert used == (cap - cap // (2 * f) - 3 if delta > 0 else 0)
        _inputs[(shape, delta)] = np.array(stego)
    return _inputs[(shape, delta)]


def dev_soft(frames, delta, n, pitched=False, mode=None, index=None, key=None, order_key=None, first_frame=0):
    """svs_soft_extract_dev on tight or pitched planes with sentinels in the padding of the planes and behind the capacity
    -> the soft bytes"""
    lib = native.load()
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    planes = Planes(f, h, w, 0, row_pitch, frame_pitch)
    host = np.full(f * frame_pitch, 0xAB, np.uint8)
    view = lambda a: np.lib.stride_tricks.as_strided(a, (f, h, w), (frame_pitch, row_pitch, 1))   # noqa: E731
    view(host)[...] = frames
    d = _Dev(host.size)
    d.put(host)
    count = max(0, min(n, 63)) if index is None else len(index)
    cap = batch.capacity_bits(f, h, w, count)
    d_out = _Dev(cap + 16)
    d_out.put(np.full(cap + 16, 0x5A, np.uint8))
    order = batch.block_order(order_key, first_frame)
    dith = None if key is None else native.Dither(key, first_frame, 0)
    sel = None if index is None else native.Coeffs(len(index), (C.c_uint8 * 63)(*index))
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    got = C.c_uint64(0xDEAD)
    native.check(lib.svs_soft_extract_dev(d.ptr, C.byref(planes), ref(order), ref(sel), ref(dith), float(delta), n, d_out.ptr, cap,
                                          batch.mode_flags(mode), C.byref(got), None), "svs_soft_extract_dev")
    native.check(lib.svs_stream_synchronize(None), "svs_stream_synchronize")
    res = d_out.get()
    assert got.value == cap, (got.value, cap)
    assert (res[cap:] == 0x5A).all(), "bytes behind the capacity were written"
    assert np.array_equal(d.get(), host), "the call wrote to its planes"
    return res[:cap]


def first_difference(got, want, n):
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return "no difference"
    return f"{bad.size} of {want.size} bytes differ, first at byte {bad[0]} (block slot {bad[0] // max(n, 1)}): {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_call_forms_against_the_model(shape, form):
    for delta in DELTAS:
        frames = frames_of(shape, delta)
        for n in N_ACS:
            model_kw, batch_kw = form_args(form, n)
            want = sl.model_batch_soft(frames, delta, n, **model_kw)
            count = max(0, min(n, 63))
            what = (shape, form, delta, n)
            got = dev_soft(frames, delta, n, pitched=shape == "pitched", **model_kw)
            assert got.size == want.size and np.array_equal(got, want), (what, "svs_soft_extract_dev", first_difference(got, want, count))
            if delta <= 0:
                assert not got.any()
            got, n_bits = batch.extract_soft_frames(frames, delta, n, **batch_kw)                      # svs_soft_extract
            assert n_bits == want.size and np.array_equal(got, want), (what, "svs_soft_extract", first_difference(got, want, count))


def dev_hard(frames, delta, n, **kw):
    """svs_extract*_dev (the entry batch.extract_device routes **kw to) -> the packed bytes"""
    f, h, w = frames.shape
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    d_in, d_out = _Dev(frames.nbytes), _Dev(nbytes + 8)
    d_in.put(frames)
    d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
    got = batch.extract_device(d_in.ptr.value, Planes.contiguous(f, h, w), delta, n, d_out.ptr.value, nbytes, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    assert got == cap
    return d_out.get()[:nbytes]


HARD_CALLS = {   # the hard entry -> (batch.extract_device keywords, dev_soft keywords) at n coefficients
    "svs_extract_dev": lambda n: ({}, {}),
    "svs_extract_ordered_dev": lambda n: (dict(order=batch.block_order(ORDER_KEY, FIRST)), dict(order_key=ORDER_KEY, first_frame=FIRST)),
    "svs_extract_select_dev": lambda n: (dict(coeffs=sl.zigzag(n)), dict(index=sl.zigzag(n))),
    "svs_extract_dithered_dev": lambda n: (dict(dither_key=KEY, first_frame=FIRST), dict(key=KEY, first_frame=FIRST)),
}


def identity_inputs():
    """the stego-and-noise frames of the largest shape, and the tie corpus (the ties are in its frames) at its own deltas"""
    out = [("three_workgroups", d, frames_of("three_workgroups", d), None) for d in (8, 20, 12.5, 0.1)]
    for family, n, delta in tl.one_setting_per_family_and_mode():
        out.append((f"ties-{family}", delta, np.array(tl.frames_for(n, delta, tl.WIDTHS[n % 2])[0]), n))
    return out


@pytest.mark.parametrize("entry", sorted(HARD_CALLS))
def test_hard_bits_are_those_of_the_hard_call(entry):
    for name, delta, frames, only_n in identity_inputs():
        for n in ((only_n,) if only_n else (1, 10, 63)):
            hard_kw, soft_kw = HARD_CALLS[entry](n)
            if entry == "svs_extract_dithered_dev" and only_n:
                hard_kw, soft_kw = (dict(dither_key=tl.KEY, first_frame=tl.FIRST_FRAME), dict(key=tl.KEY, first_frame=tl.FIRST_FRAME))
            soft = dev_soft(frames, delta, n, **soft_kw)
            for mode in (None, "exact"):
                hard = dev_hard(frames, delta, n, mode=mode, **hard_kw)
                assert np.array_equal(sl.packed_hard(soft), hard), (entry, name, delta, n, mode)


def test_a_soft_call_leaves_nothing_behind_for_the_hard_calls():
    """the same stream, the same output buffer: hard call, soft call, hard call again - for every hard entry, the second
    hard result is the first, byte for byte (no state, no LDS setting, no stale output survives the soft launch)"""
    lib = native.load()
    frames = frames_of("three_workgroups", 20)
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    d_in = _Dev(frames.nbytes)
    d_in.put(frames)
    for entry in sorted(HARD_CALLS):
        for n in (3, 10, 63):
            hard_kw, soft_kw = HARD_CALLS[entry](n)
            cap = batch.capacity_bits(f, h, w, n)
            nbytes = (cap + 7) // 8
            d_hard, d_soft = _Dev(nbytes + 8), _Dev(cap + 8)
            results = []
            for k in range(2):
                d_hard.put(np.full(nbytes + 8, 0x5A, np.uint8))
                assert batch.extract_device(d_in.ptr.value, planes, 20, n, d_hard.ptr.value, nbytes, **hard_kw) == cap
                if k == 0:
                    index, key = soft_kw.get("index"), soft_kw.get("key")
                    assert batch.extract_soft_device(d_in.ptr.value, planes, 20, n, d_soft.ptr.value, cap, coeffs=index, dither_key=key,
                                                     order=hard_kw.get("order"), first_frame=soft_kw.get("first_frame")) == cap
                native.check(lib.svs_stream_synchronize(None), "sync")
                results.append(d_hard.get())
            assert np.array_equal(results[0], results[1]), (entry, n)
            assert np.array_equal(sl.packed_hard(d_soft.get()[:cap]), results[0][:nbytes]), (entry, n)
