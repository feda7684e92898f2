"""The Reed-Solomon decoder on the GPU (svs_rs_decode_dev, include/svsrs.h) against the NumPy model of tests/rs_lib.py - stream,
status bytes and both counters, byte for byte and without a tolerance - at the lengths at which the kernel takes another path
(one byte, a codeword one byte short of full, full, two codewords of equal and of unequal length, three, exactly the 64
codewords of one workgroup, one more, five workgroups with a ragged last one and k mod C != 0), on clean, repairable, unrepairable and random
streams; what a call leaves behind; a second stream; and the round trips of batch.embed_coded_frames / extract_coded_frames with
outer=True through the requantisation channel.  No case passes an out-of-range argument: those are refused on the host
(tests/test_rs_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import rs_lib as rl
from test_gpu_parity import _Dev
from svsdct import batch, fec, native, rs
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

GUARD = 64                              # sentinel bytes before and behind the status bytes and behind the stream
LEAD = 65                               # sentinel bytes before the stream: it starts at an odd address
SENTINEL = 0xA5
BEFORE = (1000, 4000000000)             # what the counters hold before a call: the call adds


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    rs.load()


def device_decode(received, k, stream=None, with_counts=True):
    """one decoder call -> (stream, status, counts added); checks what the call leaves behind"""
    lib = native.load()
    n_cw, total = rl.codewords(k), rl.coded_bytes(k)
    host = np.concatenate([np.full(LEAD, SENTINEL, np.uint8), received, np.full(GUARD, SENTINEL, np.uint8)])
    d_stream = _Dev(host.size)
    d_stream.put(host)
    d_status = _Dev(n_cw + 2 * GUARD)
    d_status.put(np.full(n_cw + 2 * GUARD, SENTINEL, np.uint8))
    d_counts = _Dev(16)
    d_counts.put(np.array([0xDEADBEEF, BEFORE[0], BEFORE[1], 0xDEADBEEF], np.uint32))
    assert (d_stream.ptr.value + LEAD) % 2 == 1 and (d_counts.ptr.value + 4) % 4 == 0
    rs.decode_device(d_stream.ptr.value + LEAD, k, d_status.ptr.value + GUARD, n_cw, d_counts.ptr.value + 4 if with_counts else 0, stream or 0)
    native.check(lib.svs_stream_synchronize(stream), "svs_stream_synchronize")
    got, st, cnt = d_stream.get(), d_status.get(), d_counts.get(dtype=np.uint32)
    assert (got[:LEAD] == SENTINEL).all() and (got[LEAD + total:] == SENTINEL).all(), "the call wrote outside the stream"
    assert (st[:GUARD] == SENTINEL).all() and (st[GUARD + n_cw:] == SENTINEL).all(), "the call wrote outside the status bytes"
    assert cnt[0] == cnt[3] == 0xDEADBEEF, "the call wrote outside the counters"
    added = ((int(cnt[1]) - BEFORE[0]) % 2 ** 32, (int(cnt[2]) - BEFORE[1]) % 2 ** 32)
    if not with_counts:
        assert added == (0, 0)
    return got[LEAD: LEAD + total], st[GUARD: GUARD + n_cw], added


@pytest.mark.parametrize("kind", rl.KINDS)
def test_the_device_is_the_model_byte_for_byte(kind):
    for k in rl.KS:
        received, want, status, counts = rl.case(kind, k)
        got, got_status, added = device_decode(received, k)
        bad = np.flatnonzero(got_status != status)
        assert bad.size == 0, (kind, k, f"{bad.size} status bytes differ, first at {bad[0]}: {got_status[bad[0]]} for {status[bad[0]]}")
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (kind, k, f"{bad.size} stream bytes differ, first at {bad[0]}")
        assert added == counts, (kind, k)
    if kind == "seventeen":
        assert all((rl.case(kind, k)[2] == rl.UNCORRECTABLE).any() for k in rl.KS)


def test_the_counters_may_be_null_and_a_second_stream_gives_the_same_bytes():
    lib = native.load()
    for kind, k in (("sixteen", 447), ("seventeen", 225), ("ends", 257 * 223 + 5)):
        received, want, status, _ = rl.case(kind, k)
        got, got_status, _ = device_decode(received, k, with_counts=False)
        assert np.array_equal(got, want) and np.array_equal(got_status, status), (kind, k)
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for kind, k in (("sixteen", 257 * 223 + 5), ("random", 64 * 223 + 1), ("burst", 446)):
            received, want, status, counts = rl.case(kind, k)
            got, got_status, added = device_decode(received, k, stream)
            assert np.array_equal(got, want) and np.array_equal(got_status, status) and added == counts, (kind, k)
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def test_the_staged_call_and_an_empty_stream():
    received, want, status, _ = rl.case("sixteen", 225)
    data, got_status = rs.decode(received.tobytes(), 225)
    assert data == want[:225].tobytes() and np.array_equal(got_status, status)
    assert rs.decode(b"", 0)[0] == b""
    rs.decode_device(0, 0, 0, 0)                            # k = 0: SVS_OK, no pointer is looked at, nothing is launched


def _requantise_on_device(frames, quality):
    f, h, w = frames.shape
    d = _Dev(frames.size)
    d.put(frames)
    batch.requantise_device(d.ptr.value, d.ptr.value, Planes.contiguous(f, h, w), quality)
    native.check(native.load().svs_stream_synchronize(None), "svs_stream_synchronize")
    return d.get().reshape(frames.shape)


@pytest.mark.parametrize("rate,quality", ((3, 60), (78, 80)))
def test_round_trip_of_both_codes_through_the_channel(rate, quality):
    """the CPU test's cells on the device, cover seed 5: the Viterbi decoder leaves wrong bits, the outer code delivers the
    payload and says how many bytes it corrected in each codeword - bits and status are the CPU model's"""
    model = rl.outer_survival(rate, quality, 5)
    cover, data = rl.outer_clip(rate, 5)
    bits = np.unpackbits(data)
    assert bits.size == rs.payload_bits(7200, rate)
    stego, used, n_info = batch.embed_coded_frames(cover, 20, 10, bits, rate=rate, outer=True)
    assert n_info == bits.size and used == fec.coded_bits(8 * rs.coded_bytes(data.size), rate)
    received = _requantise_on_device(stego, quality)
    inner = batch.extract_coded_frames(received, 20, 10, 8 * rs.coded_bytes(data.size), rate=rate)          # the Viterbi output alone
    assert np.array_equal(np.packbits(inner), model["received"])
    assert int((inner[: bits.size] != bits).sum()) == model["viterbi_bits"] > 0
    got, status = batch.extract_coded_frames(received, 20, 10, n_info, rate=rate, outer=True)
    print(f"rate code {rate}, Q = {quality}: {model['viterbi_bits']} wrong payload bits after Viterbi, status {list(status)}, "
          f"{int((got != bits).sum())} wrong after the outer code")
    assert np.array_equal(status, model["status"]) and (status != 0).all() and (status <= 16).all()
    assert int((got != bits).sum()) == 0 == model["wrong_bits"]
