"""The punctured codes on the GPU (svs_fec_decode_soft_dev / svs_fec_decode_weights_dev at rate 23, 34, 56, 78;
include/svsfec.h "Punctured codes") against the NumPy model of tests/fec_punctured_lib.py, bit for bit and without a tolerance:
tests/fec_lib.py's lengths (at least three segments, windows that start at steps 448 and 960, so every ws mod P occurs and is
not 0 at P = 7; a ragged last workgroup) and 1 019 .. 1 025, where the cut last period takes every length; against the rate-2
call that already exists, on the model's depunctured weights; what a call leaves behind, soft bytes at every byte alignment,
a second stream; and the round trips of batch.embed_coded_frames / extract_coded_frames through the requantisation channel.
No case passes an out-of-range argument: those are refused on the host (tests/test_fec_punctured_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import fec_lib as fl
import fec_punctured_lib as pl
from test_gpu_parity import _Dev
from svsdct import batch, fec, native
from svsdct import soft as sv
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

GUARD = 64                              # sentinel bytes before and behind the output
SENTINEL = 0xA5
FILL = 0x3C                             # around the input: the hard bit 0 at margin 60, and no weight the streams hold


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    fec.load()


def device_decode(values, n_info, rate, stream=None, lead=None):
    """one decoder call on `values` (uint8 soft bytes or int32 weights), which start `lead` bytes inside their buffer -> the
    decoded bits; checks what the call leaves behind"""
    lib = native.load()
    lead = (1 if values.dtype == np.uint8 else 8) if lead is None else lead
    host_in = np.concatenate([np.full(lead, FILL, np.uint8), values.view(np.uint8), np.full(16, FILL, np.uint8)])
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


def _same(got, want, *what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (*what, f"{bad.size} bits differ, first at {bad[0]}")


@pytest.mark.parametrize("code", pl.CODES)
@pytest.mark.parametrize("kind", pl.KINDS)
def test_the_device_is_the_model_bit_for_bit(kind, code):
    for n_info in pl.lengths(kind):
        values, _, want, _ = pl.case(kind, n_info, code)
        assert values.size == fec.coded_bits(n_info, code)
        _same(device_decode(values, n_info, code), want, kind, code, n_info)


@pytest.mark.parametrize("code", pl.CODES)
@pytest.mark.parametrize("kind", pl.KINDS)
def test_the_rate_2_call_on_depunctured_weights_gives_the_same_bits(kind, code):
    """the call that exists today, svs_fec_decode_weights_dev at rate 2, on the model's depunctured int32 weights (zeros at the
    unsent bits) against the punctured soft call and the punctured weights call on the n_sent values themselves"""
    for n_info in pl.lengths(kind):
        values, _, want, mother = pl.case(kind, n_info, code)
        assert mother.size == 2 * (n_info + 6) and (mother == 0).sum() >= mother.size - values.size
        old = device_decode(mother, n_info, 2)
        _same(old, want, "rate 2 on depunctured weights", kind, code, n_info)
        weights = values if values.dtype == np.int32 else fl.weights_of_soft(values).astype(np.int32)
        _same(device_decode(weights, n_info, code), old, "punctured weights call", kind, code, n_info)
        if values.dtype == np.uint8:
            _same(device_decode(values, n_info, code), old, "punctured soft call", kind, code, n_info)


def test_soft_bytes_at_every_byte_alignment():
    """the run of sent values [S(ws), S(we)) starts wherever it starts: the input pointer at odd and even byte offsets"""
    for code in pl.CODES:
        for lead in (1, 2, 3, 4):
            for n_info in (571, 1023):
                values, _, want, _ = pl.case("flipped", n_info, code)
                _same(device_decode(values, n_info, code, lead=lead), want, code, lead, n_info)


def test_a_second_stream_gives_the_same_bits():
    lib = native.load()
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for kind, code, n_info in (("flipped", 23, 2045), ("random", 78, pl.LARGEST), ("tally", 56, 1021), ("all80", 34, 571)):
            values, _, want, _ = pl.case(kind, n_info, code)
            _same(device_decode(values, n_info, code, stream), want, kind, code, n_info)
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def test_the_staged_call_and_an_empty_payload():
    values, _, want, _ = pl.case("flipped", 1019, 34)
    assert np.array_equal(fec.decode_soft(values, 1019, 34), want)
    values, _, want, _ = pl.case("tally", 507, 78)
    assert np.array_equal(fec.decode_weights(values, 507, 78), want)
    assert fec.decode_soft(np.zeros(fec.coded_bits(0, 56), np.uint8), 0, 56).size == 0
    fec.decode_soft_device(0, 0, 23, 0, 0)                   # n_info = 0: SVS_OK, no pointer is looked at, nothing is launched


def _requantise_on_device(frames, quality):
    f, h, w = frames.shape
    d = _Dev(frames.size)
    d.put(frames)
    batch.requantise_device(d.ptr.value, d.ptr.value, Planes.contiguous(f, h, w), quality)
    native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
    return d.get().reshape(frames.shape)


# (code, quality of the channel, the wrong coded bits the channel must leave).  Rate 3/4 at Q = 75: the CPU model has 483.
# Rate 5/6 at Q = 80: the CPU model has 82, and the bounds are its half and its double
@pytest.mark.parametrize("code,quality,low,high", [(34, 75, 300, 700), (56, 80, 41, 164)])
def test_round_trip_through_the_channel(code, quality, low, high):
    """the CPU test's zero cells on the device: delta = 20, n = 10, reference rule - 0 wrong payload bits of 5 394 at rate 3/4
    behind Q = 75 and of 5 994 at rate 5/6 behind Q = 80"""
    cover, info = pl.coded_clip(code)
    stego, used, n_info = batch.embed_coded_frames(cover, 20, 10, info, rate=code)
    assert n_info == info.size == fec.info_bits(7200, code) and used == fec.coded_bits(n_info, code) <= 7200
    received = _requantise_on_device(stego, quality)
    soft, _ = batch.extract_soft_frames(received, 20, 10)
    coded_wrong = int(((soft[:used] >> 7) != fec.encode(info, code)).sum())
    got = batch.extract_coded_frames(received, 20, 10, n_info, rate=code)
    print(f"code {code} through Q = {quality}: {coded_wrong} wrong coded bits of {used}, {int((got != info).sum())} wrong payload bits of {n_info}")
    assert low < coded_wrong < high                           # the channel did damage
    assert np.array_equal(got, pl.decode_soft(soft[:used], n_info, code))
    assert int((got != info).sum()) == 0


def test_round_trip_of_two_copies_through_the_tally():
    """rate 2/3, 2 394 payload bits: two copies of the 3 600 sent bits fill the 7 200 capacity bits; the tally's period is
    n_sent, and the device's bits are the model's on soft.tally of the device's own soft bytes"""
    code = 23
    n_info = fec.info_bits(7200 // 2, code)
    n_sent = fec.coded_bits(n_info, code)
    assert (n_info, n_sent) == (2394, 3600)
    cover, info = pl.coded_clip(code, n_info=n_info)
    stego, used, _ = batch.embed_coded_frames(cover, 20, 10, info, rate=code, copies=2, dither_key=77, block_key=5)
    assert used == 2 * n_sent == 7200
    received = _requantise_on_device(stego, 75)
    soft, _ = batch.extract_soft_frames(received, 20, 10, dither_key=77, block_key=5)
    tally = sv.tally(soft, n_sent)
    want = pl.decode_int32(tally, n_info, code)
    got = batch.extract_coded_frames(received, 20, 10, n_info, rate=code, copies=2, dither_key=77, block_key=5)
    assert np.array_equal(got, want)
    print(f"two copies at rate 2/3 through Q = 75: {int((got != info).sum())} wrong payload bits of {n_info}, "
          f"{int((sv.tally_bits(tally) != fec.encode(info, code)).sum())} wrong sent bits in the tally")
    assert np.array_equal(batch.extract_coded_frames(stego, 20, 10, n_info, rate=code, copies=None, dither_key=77, block_key=5), info)
