"""The errors-and-erasures decoder on the GPU (svs_rse_decode_dev, include/svsrse.h) against the NumPy model of tests/rse_lib.py -
stream, status bytes and both counters, byte for byte and without a tolerance - at the lengths of tests/rs_lib.py, where the
kernel takes another path (one short codeword of 33 bytes, k mod C != 0, exactly one workgroup, one codeword more, a ragged last
workgroup), on every kind of input of rse_lib.KINDS and, with a NULL and with an all-zero mask, on the parent decoder's inputs
and results; what a call leaves behind, the mask included; a second stream; the staged call; and the round trip of
batch.embed_coded_frames / extract_coded_frames with a lost frame.  No case passes an out-of-range argument: those are refused
on the host (tests/test_rse_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import rs_lib as rl
import rse_lib as el
from test_gpu_parity import _Dev
from svsdct import batch, fec, native, rs, rse

pytestmark = pytest.mark.gpu

GUARD = 64                              # sentinel bytes before and behind the status bytes and behind the stream and the mask
LEAD = 65                               # sentinel bytes before the stream: it starts at an odd address
MASK_LEAD = 67                          # and before the mask: another odd address
SENTINEL = 0xA5
BEFORE = (1000, 4000000000)             # what the counters hold before a call: the call adds


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)
    rse.load()


def device_decode(received, k, mask, stream=None, with_counts=True):
    """one decoder call -> (stream, status, counts added); checks what the call leaves behind.  mask: None (a NULL pointer) or
    coded_bytes(k) bytes"""
    lib = native.load()
    n_cw, total = rl.codewords(k), rl.coded_bytes(k)
    host = np.concatenate([np.full(LEAD, SENTINEL, np.uint8), received, np.full(GUARD, SENTINEL, np.uint8)])
    d_stream = _Dev(host.size)
    d_stream.put(host)
    d_mask, mask_host = None, None
    if mask is not None:
        mask_host = np.concatenate([np.full(MASK_LEAD, SENTINEL, np.uint8), mask, np.full(GUARD, SENTINEL, np.uint8)])
        d_mask = _Dev(mask_host.size)
        d_mask.put(mask_host)
        assert (d_mask.ptr.value + MASK_LEAD) % 2 == 1
    d_status = _Dev(n_cw + 2 * GUARD)
    d_status.put(np.full(n_cw + 2 * GUARD, SENTINEL, np.uint8))
    d_counts = _Dev(16)
    d_counts.put(np.array([0xDEADBEEF, BEFORE[0], BEFORE[1], 0xDEADBEEF], np.uint32))
    assert (d_stream.ptr.value + LEAD) % 2 == 1 and (d_counts.ptr.value + 4) % 4 == 0
    rse.decode_device(d_stream.ptr.value + LEAD, k, d_mask.ptr.value + MASK_LEAD if d_mask else 0, d_status.ptr.value + GUARD, n_cw,
                      d_counts.ptr.value + 4 if with_counts else 0, stream or 0)
    native.check(lib.svs_stream_synchronize(stream), "svs_stream_synchronize")
    got, st, cnt = d_stream.get(), d_status.get(), d_counts.get(dtype=np.uint32)
    assert (got[:LEAD] == SENTINEL).all() and (got[LEAD + total:] == SENTINEL).all(), "the call wrote outside the stream"
    assert (st[:GUARD] == SENTINEL).all() and (st[GUARD + n_cw:] == SENTINEL).all(), "the call wrote outside the status bytes"
    assert cnt[0] == cnt[3] == 0xDEADBEEF, "the call wrote outside the counters"
    if d_mask:
        assert np.array_equal(d_mask.get(), mask_host), "the call wrote the mask or round it"
    added = ((int(cnt[1]) - BEFORE[0]) % 2 ** 32, (int(cnt[2]) - BEFORE[1]) % 2 ** 32)
    if not with_counts:
        assert added == (0, 0)
    return got[LEAD: LEAD + total], st[GUARD: GUARD + n_cw], added


def _same(kind, k, got, got_status, added, want, status, counts):
    bad = np.flatnonzero(got_status != status)
    assert bad.size == 0, (kind, k, f"{bad.size} status bytes differ, first at {bad[0]}: {got_status[bad[0]]} for {status[bad[0]]}")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (kind, k, f"{bad.size} stream bytes differ, first at {bad[0]}")
    assert added == counts, (kind, k)


@pytest.mark.parametrize("kind", el.KINDS)
def test_the_device_is_the_model_byte_for_byte(kind):
    for k in el.KS:
        received, mask, _, want, status, counts = el.case(kind, k)
        _same(kind, k, *device_decode(received, k, mask), want, status, counts)


@pytest.mark.parametrize("kind", el.NOMASK_KINDS)
def test_without_erasures_the_device_is_the_parent_decoder(kind):
    """a NULL mask and a mask of zeros: exactly rs_lib.case's stream, status and counts"""
    for k in el.KS:
        received, want, status, counts = rl.case(kind, k)
        _same(kind, k, *device_decode(received, k, None), want, status, counts)
        _same(kind, k, *device_decode(received, k, np.zeros(received.size, np.uint8)), want, status, counts)


def test_the_counters_may_be_null_and_a_second_stream_gives_the_same_bytes():
    lib = native.load()
    for kind, k in (("mixed", 447), ("over", 225), ("f33", 64 * 223 + 1), ("right", 257 * 223 + 5)):
        received, mask, _, want, status, _ = el.case(kind, k)
        got, got_status, _ = device_decode(received, k, mask, with_counts=False)
        assert np.array_equal(got, want) and np.array_equal(got_status, status), (kind, k)
    stream = C.c_void_p()
    native.check(lib.svs_stream_create(C.byref(stream)), "svs_stream_create")
    try:
        for kind, k in (("mixed", 257 * 223 + 5), ("random", 64 * 223 + 1), ("burst32", 446)):
            received, mask, _, want, status, counts = el.case(kind, k)
            _same(kind, k, *device_decode(received, k, mask, stream), want, status, counts)
    finally:
        native.check(lib.svs_stream_destroy(stream), "svs_stream_destroy")


def test_the_staged_call_and_an_empty_stream():
    received, mask, sent, want, status, _ = el.case("mixed", 225)
    data, got_status = rse.decode(received.tobytes(), 225, mask)
    assert data == want[:225].tobytes() == sent[:225].tobytes() and np.array_equal(got_status, status)
    received, want, status, _ = rl.case("sixteen", 225)
    data, got_status = rse.decode(received, 225)
    assert data == want[:225].tobytes() and np.array_equal(got_status, status)
    assert rse.decode(b"", 0)[0] == b""
    rse.decode_device(0, 0, 0, 0, 0)                        # k = 0: SVS_OK, no pointer is looked at, nothing is launched


def test_round_trip_with_a_lost_frame():
    """the CPU table's cell of seed 1, frame 5 on the device: the frame is replaced by noise behind the embed; told so, the
    receiver returns the model's bits - the payload - and status; not told, the model's 255s"""
    cell = el.lost_frame(1, 5)
    bits = np.unpackbits(cell["data"])
    assert bits.size == rs.payload_bits(12 * 2400, 2) == 8 * 1561
    stego, used, n_info = batch.embed_coded_frames(cell["cover"], 20, 10, bits, rate=2, outer=True)
    assert n_info == bits.size and used == fec.coded_bits(8 * rs.coded_bytes(1561), 2)
    received = stego.copy()
    received[5] = cell["received"][5]                       # the model's noise frame
    got, status = batch.extract_coded_frames(received, 20, 10, n_info, rate=2, outer=True, lost_frames=[5])
    print(f"frame 5 of 12 lost: status with the span erased {list(status)}, {int((got != bits).sum())} wrong payload bits")
    assert np.array_equal(status, cell["erased"][1]) and (status <= 32).all()
    assert np.array_equal(got, np.unpackbits(cell["erased"][0][:1561])) and np.array_equal(got, bits)
    got, status = batch.extract_coded_frames(received, 20, 10, n_info, rate=2, outer=True)
    assert np.array_equal(status, cell["plain"][1]) and (status == 255).any()
    assert np.array_equal(got, np.unpackbits(cell["plain"][0][:1561]))
