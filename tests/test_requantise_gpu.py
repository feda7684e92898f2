"""The requantisation channel on the GPU (svs_requantise_dev / svs_requantise, include/svsdct.h): the device output against the
NumPy model of the format (tests/channel_lib.py model_requantise) byte for byte - no tolerance: the model is pocketfft and the
exact kernels are pocketfft-identical - on the shapes, tables and contents of channel_lib (tests/test_requantise_cpu.py checks
that they meet rounding ties and saturate); pitched planes whose padding must survive, in place against out of place, the host
call over several staging chunks, the round trip embed - channel - fused vote against the model, and the embed calls that
share the channel's kernel instantiation."""
import ctypes as C
import functools

import numpy as np
import pytest

import channel_lib as cl
from oracle import qim_dct_oracle as orc
from test_gpu_parity import _Dev
from testlib import experiments_library
from svsdct import batch, channel, native
from svsdct import soft as sv
from svsdct.native import Planes, Steps

pytestmark = pytest.mark.gpu

PAD = 0xAB


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


@functools.lru_cache(maxsize=None)
def frames_of(shape, kind):
    frames = cl.content(kind, cl.SHAPES[shape])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def model_of(shape, kind, table):
    out = cl.model_requantise(frames_of(shape, kind), cl.TABLES[table])
    out.setflags(write=False)
    return out


def geometry(frames, pitched):
    f, h, w = frames.shape
    row_pitch, frame_pitch = (w + 24, (w + 24) * h + 64) if pitched else (w, w * h)
    return Planes(f, h, w, 0, row_pitch, frame_pitch)


def planted(frames, planes, fill=PAD):
    """the frames in a host buffer of the planes' geometry, `fill` in the padding"""
    host = np.full(planes.n_frames * planes.frame_pitch, fill, np.uint8)
    view(host, planes)[...] = frames
    return host


def view(host, planes):
    return np.lib.stride_tricks.as_strided(host, (planes.n_frames, planes.height, planes.width), (planes.frame_pitch, planes.row_pitch, 1))


def padding_of(host, planes):
    mask = np.ones(host.size, bool)
    view(mask, planes)[...] = False
    return host[mask]


def run(frames, table, pitched=False, in_place=False):
    """one svs_requantise_dev -> (output frames, the output buffer's padding bytes, the input buffer after the call)"""
    planes = geometry(frames, pitched)
    host = planted(frames, planes)
    d_in = _Dev(host.size)
    d_in.put(host)
    d_out = d_in if in_place else _Dev(host.size)
    if not in_place:
        d_out.put(np.full(host.size, PAD, np.uint8))
    batch.requantise_device(d_in.ptr.value, d_out.ptr.value, planes, table)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    out = d_out.get()
    return view(out, planes).copy(), padding_of(out, planes), d_in.get()


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else f"{len(bad)} of {want.size} pixels differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---- 1. equality with the model ----------------------------------------------------------------------------------------------
LAYOUTS = [(s, False) for s in cl.SHAPES] + [(cl.PITCHED, True)]


@pytest.mark.parametrize("kind", cl.CONTENTS)
@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=[s + ("_pitched" if p else "") for s, p in LAYOUTS])
def test_the_device_output_is_the_models(shape, pitched, kind):
    frames = frames_of(shape, kind)
    for table in cl.TABLES:
        want = model_of(shape, kind, table)
        got, padding, source = run(frames, cl.TABLES[table], pitched)
        assert np.array_equal(got, want), (shape, pitched, kind, table, first_difference(got, want))
        assert (padding == PAD).all(), (shape, kind, table, "the call wrote into the padding")
        assert np.array_equal(source, planted(frames, geometry(frames, pitched))), "the call wrote to its input"


@pytest.mark.parametrize("shape,pitched", LAYOUTS, ids=[s + ("_pitched" if p else "") for s, p in LAYOUTS])
def test_in_place_equals_out_of_place_and_leaves_the_padding_alone(shape, pitched):
    for kind in ("full", "stego"):
        frames = frames_of(shape, kind)
        for table in ("q75", "odd", "ones"):
            got, padding, _ = run(frames, cl.TABLES[table], pitched, in_place=True)
            want = model_of(shape, kind, table)
            assert np.array_equal(got, want), (shape, kind, table, first_difference(got, want))
            assert (padding == PAD).all(), (shape, kind, table)


def test_a_quality_is_its_table_and_the_host_call_returns_a_new_array():
    frames = frames_of("odd", "mid")
    got = batch.requantise_frames(frames, 75)
    assert got is not frames and got.dtype == np.uint8 and got.shape == frames.shape
    assert np.array_equal(got, model_of("odd", "mid", "q75"))
    assert np.array_equal(batch.requantise_frames(frames, channel.quality_steps(75)), got)
    assert np.array_equal(batch.requantise_frames(frames[0], cl.TABLES["odd"])[0], model_of("odd", "mid", "odd")[0])


# ---- 2. the host call over several staging chunks -----------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_kb", [8, 32, 4096])
def test_the_host_call_in_chunks_equals_the_device_call(chunk_kb, monkeypatch):
    """As tests/test_gpu_parity.py forces it for svs_embed: with the experiments library's SVS_STAGE_CHUNK_KB the chunks of a
    pitched five-frame clip with an odd block count per row are bands of 32 rows (8 KB), groups of three frames (32 KB) or the
    whole batch (4 MB).  Padding of the caller's output stays untouched; in place works on the host too."""
    exp = experiments_library()
    monkeypatch.setenv("SVS_STAGE_CHUNK_KB", str(chunk_kb))
    f, h, w = 5, 64, 136
    planes = Planes(f, h, w, 0, 144, 64 * 144 + 64)
    frames = np.random.default_rng(chunk_kb).integers(0, 256, (f, h, w)).astype(np.uint8)
    src = planted(frames, planes, 0x11)
    for table in ("q50", "odd"):
        steps = channel.steps_struct(cl.TABLES[table])
        want = cl.model_requantise(frames, cl.TABLES[table])
        device, _, _ = run(frames, cl.TABLES[table], pitched=True)
        assert np.array_equal(device, want), (table, first_difference(device, want))
        dst = np.full(src.size, 0xA5, np.uint8)
        rc = exp.svs_requantise(src.ctypes.data, dst.ctypes.data, C.byref(planes), C.byref(steps), 0)
        assert rc == 0, exp.svs_last_error()
        assert np.array_equal(view(dst, planes), device), (chunk_kb, table, first_difference(view(dst, planes), device))
        assert (padding_of(dst, planes) == 0xA5).all(), (chunk_kb, table)
        assert np.array_equal(src, planted(frames, planes, 0x11))
        both = src.copy()
        rc = exp.svs_requantise(both.ctypes.data, both.ctypes.data, C.byref(planes), C.byref(steps), 0)
        assert rc == 0, exp.svs_last_error()
        assert np.array_equal(view(both, planes), device) and (padding_of(both, planes) == 0x11).all(), (chunk_kb, table)


def test_refusals_and_the_empty_call_leave_the_output_untouched():
    lib = native.load()
    frames = frames_of("one_block", "full")
    planes = geometry(frames, False)
    d_in, d_out = _Dev(frames.size), _Dev(frames.size)
    d_in.put(frames)
    d_out.put(np.full(frames.size, PAD, np.uint8))
    bad = Steps((C.c_uint16 * 64)(*([1] * 63 + [256])))
    good = channel.steps_struct(50)
    empty = Planes(0, 8, 8, 0, 8, 64)
    assert lib.svs_requantise_dev(d_in.ptr, d_out.ptr, C.byref(planes), C.byref(bad), 0, None) == native.SVS_ERR_INVALID_ARG
    assert b"step[63] = 256" in lib.svs_last_error()
    assert lib.svs_requantise_dev(d_in.ptr, d_out.ptr, C.byref(planes), C.byref(good), 2, None) == native.SVS_ERR_INVALID_ARG
    assert lib.svs_requantise_dev(d_in.ptr, d_out.ptr, C.byref(planes), None, 0, None) == native.SVS_ERR_INVALID_ARG
    assert lib.svs_requantise_dev(d_in.ptr, d_out.ptr, C.byref(empty), C.byref(good), 0, None) == native.SVS_OK
    native.check(lib.svs_stream_synchronize(None), "sync")
    assert (d_out.get() == PAD).all()


# ---- 3. embed, channel, fused vote: the numbers of the model ------------------------------------------------------------------
@pytest.mark.parametrize("quality", (85, 75))
def test_round_trip_numbers_are_the_models(quality):
    """the example's small shape: three frames of noise in [64, 192), one 2 400-bit payload copy per frame, delta = 20, n = 10"""
    lib = native.load()
    delta, n = 20, 10
    rng = np.random.default_rng(cl.SURVIVAL_SEED)
    f, h, w = cl.SURVIVAL_SHAPE
    cover = rng.integers(64, 192, cl.SURVIVAL_SHAPE).astype(np.uint8)
    payload = rng.integers(0, 2, (h // 8) * (w // 8) * n).astype(np.uint8)
    stego, used, period = batch.embed_repeated_frames(cover, delta, n, payload, mode="exact")
    assert (used, period) == (3 * payload.size, payload.size)
    assert np.array_equal(stego, cl.model_stego(cover, delta, n, payload))
    want = cl.read_copies(cl.model_requantise(stego, channel.quality_steps(quality)), delta, n, payload)

    planes = Planes.contiguous(f, h, w)
    d = _Dev(stego.size)
    d.put(stego)
    batch.requantise_device(d.ptr.value, d.ptr.value, planes, quality)
    d_tally, d_hist = _Dev(4 * period), _Dev(1024 * f)
    d_tally.put(np.zeros(period, np.int32))
    d_hist.put(np.zeros(256 * f, np.uint32))
    assert batch.extract_vote_device(d.ptr.value, planes, delta, n, d_tally.ptr.value, period) == used
    assert batch.extract_histogram_device(d.ptr.value, planes, delta, n, d_hist.ptr.value) == used
    native.check(lib.svs_stream_synchronize(None), "sync")
    bits = sv.tally_bits(d_tally.get(dtype=np.int32))
    hist = d_hist.get(dtype=np.uint32).reshape(f, 256)
    soft, _ = batch.extract_soft_frames(d.get().reshape(f, h, w), delta, n)
    single = [int((b != payload).sum()) for b in (soft >> 7).reshape(f, -1)]
    got = dict(single=single, soft=int((bits != payload).sum()), share=[float(s) for s in sv.lattice_share(hist)])
    print(f"quality {quality}: {got}")
    assert got["single"] == want["single"] and got["soft"] == want["soft"] and got["share"] == want["share"], (got, want)
    if quality == 75:
        assert got["soft"] > 0        # the channel is felt: not the numbers of an undisturbed clip


# ---- 4. the embed calls that share the channel's instantiation ----------------------------------------------------------------
@pytest.mark.parametrize("n", (40, 63))
def test_the_exact_embed_at_a_delta_that_is_no_float32_is_still_the_oracles(n):
    """delta = 7.3 with sixteen and more coefficients runs embed_exact_kernel<QM_DOUBLE, 8>, which now also holds the channel
    body - before and after a channel launch on the same stream"""
    frames = frames_of("odd", "full")
    f, h, w = frames.shape
    payload = np.random.default_rng(n).integers(0, 2, batch.capacity_bits(f, h, w, n) - 5 * n - 3).astype(np.uint8)
    want, want_used = orc.batch_embed(frames, 7.3, payload, n)
    for _ in range(2):
        stego, used = batch.embed_frames(frames, 7.3, n, payload, mode="exact")
        assert used == want_used == payload.size
        assert np.array_equal(stego, want), first_difference(stego, want)
        assert np.array_equal(batch.requantise_frames(frames, 90), model_of("odd", "full", "q90"))
