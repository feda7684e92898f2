"""The device encoders on the GPU (svs_rs_encode_dev, svs_fec_encode_dev, svs_bits_tile_dev, include/svsenc.h) against the host
encoders - byte for byte, without a tolerance - at the lengths of tests/enc_lib.py (the CPU tier runs the host build of the
kernels' arithmetic on the same ones): what a call leaves round its output and of its input, inputs at every byte alignment,
Reed-Solomon in place and out of place at odd addresses, a second stream, the staged forms, the empty calls; then the public
path: batch.embed_coded_frames(encoder="device") against encoder="host", batch.embed_coded_device on a payload that lies on the
device, and one round trip through the requantisation channel.  No case passes an out-of-range argument: those are refused on
the host (tests/test_enc_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import enc_lib as el
import fec_punctured_lib as pl
from test_gpu_parity import _Dev
from svsdct import batch, enc, fec, native, rs, soft
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

GUARD = 64                              # sentinel bytes before and behind an output
SENTINEL = 0xA5
IN_LEAD = 8                             # room before an input, so that it can start at any byte alignment


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    enc.load()


def _sync(stream=None):
    native.check(native.load().svs_stream_synchronize(stream), "svs_stream_synchronize")


def run(call, src, align, out_bytes, out_lead=GUARD, stream=None):
    """one device call: src at byte alignment `align`, out_bytes of output behind out_lead sentinel bytes.  call(d_in, d_out).
    Checks that the input and the sentinels round the output stay; returns the output bytes"""
    host_in = np.full(IN_LEAD + src.size + GUARD, SENTINEL, np.uint8)
    host_in[align: align + src.size] = src
    d_in, d_out = _Dev(host_in.size), _Dev(out_lead + out_bytes + GUARD)
    d_in.put(host_in)
    d_out.put(np.full(out_lead + out_bytes + GUARD, SENTINEL, np.uint8))
    assert d_in.ptr.value % 4 == 0 and d_out.ptr.value % 4 == 0
    call(d_in.ptr.value + align, d_out.ptr.value + out_lead)
    _sync(stream)
    got = d_out.get()
    assert np.array_equal(d_in.get(), host_in), "the call wrote its input"
    assert (got[:out_lead] == SENTINEL).all() and (got[out_lead + out_bytes:] == SENTINEL).all(), "the call wrote outside its output"
    return got[out_lead: out_lead + out_bytes]


def host_coded(n_info, rate):
    """svs_fec_encode's bytes"""
    return np.packbits(fec.encode(el.info(n_info), rate))


def device_coded(n_info, rate, align, stream=None):
    nbytes = (fec.coded_bits(n_info, rate) + 7) // 8
    return run(lambda d_in, d_out: enc.fec_encode_device(d_in, n_info, rate, d_out, nbytes, stream or 0), el.packed_info(n_info), align,
               nbytes, stream=stream)


def device_stream(k, in_place, lead, stream=None):
    """svs_rs_encode_dev out of place (the data at an odd address, the stream behind `lead` sentinel bytes) or in place"""
    total = rs.coded_bytes(k)
    if not in_place:
        return run(lambda d_in, d_out: enc.rs_encode_device(d_in, k, d_out, total, stream or 0), el.data(k), 3, total, out_lead=lead,
                   stream=stream)
    host = np.full(lead + total + GUARD, SENTINEL, np.uint8)
    host[lead: lead + k] = el.data(k)
    d = _Dev(host.size)
    d.put(host)
    enc.rs_encode_device(d.ptr.value + lead, k, d.ptr.value + lead, total, stream or 0)
    _sync(stream)
    got = d.get()
    assert (got[:lead] == SENTINEL).all() and (got[lead + total:] == SENTINEL).all(), "the call wrote outside the stream"
    return got[lead: lead + total]


def device_tiled(period, n_out, align, stream=None):
    nbytes = (n_out + 7) // 8
    return run(lambda d_in, d_out: enc.tile_device(d_in, period, d_out, n_out, nbytes, stream or 0), el.packed_tile_bits(period), align,
               nbytes, stream=stream)


# ---- the three calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", el.RATES)
def test_the_convolutional_encoder_is_the_hosts_byte_for_byte(rate):
    assert max(el.N_INFOS) == 4 * 512 * 9 + 77
    for i, n_info in enumerate(el.N_INFOS):
        want = host_coded(n_info, rate)
        aligns = range(4) if n_info in (1, 9, 33, 1019, el.LARGEST) else (i % 4,)
        for align in aligns:
            got = device_coded(n_info, rate, align)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (rate, n_info, align, f"{bad.size} bytes differ, first at {bad[0]} of {want.size}")


def test_the_reed_solomon_encoder_is_the_hosts_byte_for_byte():
    assert max(el.KS) == 257 * 223 + 5
    for k in el.KS:
        want = el.stream(k)
        for in_place in (False, True):
            for lead in (65, 64):                           # the stream at an odd and at an aligned address
                got = device_stream(k, in_place, lead)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (k, in_place, lead, f"{bad.size} bytes differ, first at {bad[0]} of {want.size}")


def test_the_tile_is_soft_tile():
    for period in el.PERIODS:
        for n_out in el.tile_lengths(period):
            want = el.tiled(period, n_out)
            for align in range(4):
                got = device_tiled(period, n_out, align)
                assert np.array_equal(got, want), (period, n_out, align)
    # a coded stream tiled to a capacity, as the public path does it: several workgroups, the last copy cut
    period, n_out = fec.coded_bits(1019, 34), 4 * 512 * 9 + 77
    assert np.array_equal(device_tiled(period, n_out, 1), el.tiled(period, n_out))


def test_a_second_stream_gives_the_same_bytes():
    lib = native.load()
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for rate in el.RATES:
            assert np.array_equal(device_coded(el.LARGEST, rate, 1, stream), host_coded(el.LARGEST, rate)), rate
        for k, in_place in ((257 * 223 + 5, False), (64 * 223 + 1, True), (447, False)):
            assert np.array_equal(device_stream(k, in_place, 65, stream), el.stream(k)), (k, in_place)
        for period, n_out in ((14, 3 * 14 + 5), (4794, 3 * 4794 + 5)):
            assert np.array_equal(device_tiled(period, n_out, 3, stream), el.tiled(period, n_out)), (period, n_out)
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def test_the_staged_calls_and_the_empty_ones():
    assert np.array_equal(enc.rs_encode(el.data(447)), rs.encode_array(el.data(447)))
    assert np.array_equal(enc.rs_encode(el.data(225).tobytes()), el.stream(225))
    for rate in (2, 56):
        got = enc.fec_encode(el.info(1019), rate)
        assert got.dtype == np.uint8 and np.array_equal(got, fec.encode(el.info(1019), rate))
    for n_bits in (0, 5, 33, 100):
        assert np.array_equal(enc.tile(el.tile_bits(33), n_bits), soft.tile(el.tile_bits(33), n_bits))
    assert enc.rs_encode(b"").size == 0 and enc.fec_encode([], 3).size == 0
    enc.rs_encode_device(0, 0, 0, 0)                        # k = 0, n_info = 0, n_out_bits = 0: SVS_OK, no pointer is looked at,
    enc.fec_encode_device(0, 0, 23, 0, 0)                   # nothing is launched
    enc.tile_device(0, 7, 0, 0, 0)
    _sync()


# ---- the public path ------------------------------------------------------------------------------------------------------------------
SHAPE, DELTA, N_AC, CAP = (3, 96, 160), 20, 10, 7200


@pytest.fixture(scope="module")
def cover():
    frames = np.random.default_rng(17).integers(16, 240, SHAPE).astype(np.uint8)
    frames.setflags(write=False)
    return frames


def payload(rate, copies, outer):
    """a payload that fills the capacity (copies = 1) or half of it; without the outer code three bits short of that, so that it
    is no whole number of bytes"""
    room = CAP if copies == 1 else CAP // 2
    n = rs.payload_bits(room, rate) if outer else fec.info_bits(room, rate) - 3
    return np.random.default_rng([rate, n]).integers(0, 2, n).astype(np.uint8)


@pytest.mark.parametrize("outer", (False, True))
@pytest.mark.parametrize("rate", (2, 3, 34, 78))
def test_embed_coded_frames_with_the_device_encoder_is_the_host_path(rate, outer, cover):
    assert batch.capacity_bits(*SHAPE, N_AC) == CAP
    for copies in (1, 2, None):
        bits = payload(rate, copies, outer)
        want = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=rate, copies=copies, outer=outer, encoder="host")
        got = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=rate, copies=copies, outer=outer, encoder="device")
        assert got[1:] == want[1:] and got[2] == bits.size, (rate, outer, copies, got[1:], want[1:])
        assert want[1] == (CAP if copies is None else (1 if copies == 1 else 2) * fec.coded_bits(8 * rs.coded_bytes(bits.size // 8) if outer else bits.size, rate))
        assert np.array_equal(got[0], want[0]), (rate, outer, copies, int((got[0] != want[0]).sum()))
        assert not np.array_equal(got[0], cover)


def test_embed_coded_frames_with_the_device_encoder_takes_the_embed_keywords(cover):
    bits = payload(34, 2, True)
    for kw in (dict(coeffs="zigzag", dither_key=77, block_key=5, first_frame=3), dict(readback=True), dict(mode="exact", nearest=True)):
        want = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=34, copies=2, outer=True, **kw)
        got = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=34, copies=2, outer=True, encoder="device", **kw)
        assert got[1:] == want[1:] and len(got) == len(want) == (4 if "readback" in kw else 3), (kw, got[1:], want[1:])
        assert np.array_equal(got[0], want[0]), kw
    plain = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=34, copies=2, outer=True)[0]
    assert not np.array_equal(want[0], plain)


def test_embed_coded_device_on_a_payload_that_lies_on_the_device(cover):
    lib = native.load()
    f, h, w = SHAPE
    planes = Planes.contiguous(f, h, w)
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for rate, copies, outer in ((78, None, True), (2, 1, False), (3, 2, True)):
            bits = payload(rate, copies, outer)
            want, used, _ = batch.embed_coded_frames(cover, DELTA, N_AC, bits, rate=rate, copies=copies, outer=outer)
            packed = np.packbits(bits)
            work = batch.coded_workspace_bytes(bits.size, rate, copies, outer, CAP)
            d_gray, d_stego, d_payload, d_work = _Dev(cover.size), _Dev(cover.size), _Dev(packed.size + 4), _Dev(work + GUARD)
            d_gray.put(cover)
            host_payload = np.full(packed.size + 4, SENTINEL, np.uint8)
            host_payload[1: 1 + packed.size] = packed        # at an odd address
            d_payload.put(host_payload)
            d_work.put(np.full(work + GUARD, SENTINEL, np.uint8))
            done = batch.embed_coded_device(d_gray.ptr.value, d_stego.ptr.value, planes, DELTA, N_AC, d_payload.ptr.value + 1, bits.size,
                                            d_work.ptr.value, work, rate=rate, copies=copies, outer=outer, stream=stream.value)
            _sync(stream)
            assert done == used, (rate, copies, outer)
            assert np.array_equal(d_stego.get().reshape(SHAPE), want), (rate, copies, outer)
            assert np.array_equal(d_payload.get(), host_payload) and np.array_equal(d_gray.get().reshape(SHAPE), cover)
            assert (d_work.get()[work:] == SENTINEL).all(), "the chain wrote behind its workspace"
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def _requantise_on_device(frames, quality):
    f, h, w = frames.shape
    d = _Dev(frames.size)
    d.put(frames)
    batch.requantise_device(d.ptr.value, d.ptr.value, Planes.contiguous(f, h, w), quality)
    _sync()
    return d.get().reshape(frames.shape)


def test_round_trip_through_the_channel():
    """the cell of tests/test_fec_punctured_gpu.py with the device encoder: rate 3/4 behind Q = 75, delta = 20, n = 10, reference
    rule - 0 wrong payload bits of 5 394"""
    code = 34
    clip, info = pl.coded_clip(code)
    stego, used, n_info = batch.embed_coded_frames(clip, 20, 10, info, rate=code, encoder="device")
    assert n_info == info.size == fec.info_bits(7200, code) == 5394 and used == fec.coded_bits(n_info, code) <= 7200
    got = batch.extract_coded_frames(_requantise_on_device(stego, 75), 20, 10, n_info, rate=code)
    wrong = int((got != info).sum())
    print(f"code {code}, device encoder, through Q = 75: {wrong} wrong payload bits of {n_info}")
    assert got.size == 5394 and wrong == 0
