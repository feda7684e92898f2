"""The Viterbi decoder on the GPU (svs_fec_decode_soft_dev / svs_fec_decode_weights_dev, include/svsfec.h) against the NumPy
model of tests/fec_lib.py, bit for bit and without a tolerance, at the lengths at which the kernel takes another path (one step
past the tail, a window clamped at both ends, exactly one segment, a second segment of one step, a last segment shorter than the
overlap, several workgroups with a ragged last one), both rates, both input kinds; what a call leaves behind; a second stream;
and the round trips of batch.embed_coded_frames / extract_coded_frames through the requantisation channel.  No case passes an
out-of-range argument: those are refused on the host (tests/test_fec_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import fec_lib as fl
from test_gpu_parity import _Dev
from svsdct import batch, fec, native
from svsdct import soft as sv
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

GUARD = 64                              # sentinel bytes before and behind the output
SENTINEL = 0xA5
LEAD = {np.dtype(np.uint8): 1, np.dtype(np.int32): 8}     # the input starts inside its buffer: soft bytes at an odd address


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    fec.load()


def device_decode(values, n_info, rate, stream=None):
    """one decoder call on `values` (uint8 soft bytes or int32 weights) -> the decoded bits; checks what the call leaves behind"""
    lib = native.load()
    lead = LEAD[values.dtype]
    host_in = np.concatenate([np.full(lead, 0x3C, np.uint8), values.view(np.uint8), np.full(16, 0x3C, np.uint8)])
    d_in = _Dev(host_in.size)
    d_in.put(host_in)
    out_bytes = (n_info + 7) // 8
    d_out = _Dev(out_bytes + 2 * GUARD)
    d_out.put(np.full(out_bytes + 2 * GUARD, SENTINEL, np.uint8))
    call = fec.decode_soft_device if values.dtype == np.uint8 else fec.decode_weights_device
    call(d_in.ptr.value + lead, n_info, rate, d_out.ptr.value + GUARD, out_bytes, stream or 0)
    native.check(lib.svs_stream_synchronize(stream), "svs_stream_synchronize")
    got = d_out.get()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + out_bytes:] == SENTINEL).all(), "the call wrote outside its output"
    packed = got[GUARD: GUARD + out_bytes]
    if n_info % 8:
        assert packed[-1] & (0xFF >> (n_info % 8)) == 0, "the pad bits of the last byte are not 0"
    assert np.array_equal(d_in.get(), host_in), "the call wrote to its input"
    return np.unpackbits(packed, count=n_info)


@pytest.mark.parametrize("rate", fl.RATES)
@pytest.mark.parametrize("kind", fl.SOFT_KINDS + fl.INT32_KINDS)
def test_the_device_is_the_model_bit_for_bit(kind, rate):
    for n_info in fl.N_INFOS:
        values, info, want = fl.case(kind, n_info, rate)
        got = device_decode(values, n_info, rate)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (kind, rate, n_info, f"{bad.size} bits differ, first at {bad[0]}")


def test_int32_weights_at_the_ends_of_the_range():
    """INT32_MIN, INT32_MAX and 0 alone, and each in every position of a step"""
    for rate in fl.RATES:
        for n_info in (59, 571):
            nc = fl.coded_bits(n_info, rate)
            for pattern in ([fl.I32_MIN], [fl.I32_MAX], [0], [fl.I32_MIN, fl.I32_MAX, 0, 0, fl.I32_MAX, fl.I32_MIN, 1, -1]):
                values = np.resize(np.array(pattern, np.int64), nc).astype(np.int32)
                assert np.array_equal(device_decode(values, n_info, rate), fl.decode_int32(values, n_info, rate)), (rate, n_info, pattern)


def test_a_second_stream_gives_the_same_bits():
    lib = native.load()
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for kind, rate, n_info in (("flipped", 2, 2045), ("random", 3, 4 * 512 * 9 + 77), ("tally", 3, 571)):
            values, _, want = fl.case(kind, n_info, rate)
            assert np.array_equal(device_decode(values, n_info, rate, stream), want), (kind, rate, n_info)
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def test_the_staged_call_and_an_empty_payload():
    values, _, want = fl.case("flipped", 1019, 2)
    assert np.array_equal(fec.decode_soft(values, 1019, 2), want)
    values, _, want = fl.case("tally", 507, 3)
    assert np.array_equal(fec.decode_weights(values, 507, 3), want)
    assert fec.decode_soft(np.zeros(12, np.uint8), 0, 2).size == 0
    fec.decode_soft_device(0, 0, 3, 0, 0)                    # n_info = 0: SVS_OK, no pointer is looked at, nothing is launched


def _requantise_on_device(frames, quality):
    f, h, w = frames.shape
    d = _Dev(frames.size)
    d.put(frames)
    batch.requantise_device(d.ptr.value, d.ptr.value, Planes.contiguous(f, h, w), quality)
    native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
    return d.get().reshape(frames.shape)


@pytest.mark.parametrize("rate", fl.RATES)
def test_round_trip_through_the_channel_at_q75(rate):
    """the CPU test's cell on the device: delta = 20, n = 10, reference rule, the channel at Q = 75 - 0 wrong payload bits, where
    three copies and the soft vote leave 51"""
    cover, info = fl.coded_clip(rate)
    stego, used, n_info = batch.embed_coded_frames(cover, 20, 10, info, rate=rate)
    assert n_info == info.size == fec.info_bits(7200, rate) and used == fec.coded_bits(n_info, rate)
    received = _requantise_on_device(stego, 75)
    soft, _ = batch.extract_soft_frames(received, 20, 10)
    assert 300 < int(((soft[:used] >> 7) != fec.encode(info, rate)).sum()) < 700          # the channel did damage: 456 / 459 on the CPU
    got = batch.extract_coded_frames(received, 20, 10, n_info, rate=rate)
    assert int((got != info).sum()) == 0
    assert np.array_equal(got, fl.decode_soft(soft[:used], n_info, rate))


def test_round_trip_of_two_copies_through_the_tally():
    """rate 1/3, 1 194 payload bits: two copies of the 3 600 coded bits fill the 7 200 capacity bits; the channel at Q = 60 leaves
    errors, and the device's bits are the model's on soft.tally of the device's own soft bytes"""
    rate, n_info = 3, 1194
    cover, info = fl.coded_clip(rate, n_info=n_info)
    n_coded = fec.coded_bits(n_info, rate)
    stego, used, _ = batch.embed_coded_frames(cover, 20, 10, info, rate=rate, copies=2, dither_key=77, block_key=5)
    assert used == 2 * n_coded == 7200
    received = _requantise_on_device(stego, 60)
    soft, _ = batch.extract_soft_frames(received, 20, 10, dither_key=77, block_key=5)
    tally = sv.tally(soft, n_coded)
    want = fl.decode_int32(tally, n_info, rate)
    got = batch.extract_coded_frames(received, 20, 10, n_info, rate=rate, copies=2, dither_key=77, block_key=5)
    assert np.array_equal(got, want)
    print(f"two copies at rate 1/3 through Q = 60: {int((got != info).sum())} wrong payload bits of {n_info}, "
          f"{int((sv.tally_bits(tally) != fec.encode(info, rate)).sum())} wrong coded bits in the tally")
    assert np.array_equal(batch.extract_coded_frames(stego, 20, 10, n_info, rate=rate, copies=None, dither_key=77, block_key=5), info)
