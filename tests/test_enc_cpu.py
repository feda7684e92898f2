"""CPU tier of the device encoders (include/svsenc.h, libsvsenc.so, svsdct/enc.py): the library's exports; the host build of
csrc/svs_enc.hpp (tests/hostemu/enc_emu.cpp, lane after lane) against the host encoders and the NumPy models at every length the
GPU tier runs - and once as a stand-alone program under the address and undefined-behaviour sanitizers; the word functions at
output positions round 2^32, 2^40 and 2^43 bits against the formats evaluated bit by bit; the refusals in the documented order;
and the ValueErrors of the public path.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import enc_lib as el
import rs_lib as rl
from testlib import check_header_is_plain_c, check_library_exports, run_sanitized_emu
from svsdct import batch, enc, fec, native, rs, soft
from svsdct.native import Planes

I, CAP = native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_the_header():
    # the library holds svs_rs.hpp's LFSR table as both Reed-Solomon libraries do, and all are loaded into one process: a dynamic
    # symbol of one would be interposed by another's
    undefined = check_library_exports("svsenc.h", enc, "svs_enc", 5, hidden=("_kernel", "d_lfsr", "d_field"))
    assert enc.ABI_VERSION == 1
    assert "hipMalloc" not in undefined and "Synchronize" not in undefined                   # allocates nothing, never waits


def test_the_header_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, ("svsdct.h", "svsfec.h", "svsrs.h", "svsenc.h"),
                            "SVS_ENC_ABI_VERSION == 1 && SVS_ENC_MAX_TILE_BITS == (1ull << 43) && SVS_ERR_CAPACITY == -4")


# ---- the host build against the host encoders and the models ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_emu")


def test_the_lengths_cover_the_units():
    assert el.LARGEST == max(el.N_INFOS) and {7, 8, 9, 25, 26, 31, 32, 33} <= set(el.N_INFOS)
    for rate in el.RATES:
        steps = el.UNIT_STEPS[rate]
        assert el.emu().enc_emu_unit_steps(rate) == steps
        assert fec.coded_bits(steps - fec.TAIL, rate) == el.UNIT_BITS[rate]                    # a unit sends whole dwords
        assert {steps * m - fec.TAIL + e for m in (1, 64) for e in (-1, 0, 1)} <= set(el.N_INFOS)


@pytest.mark.parametrize("rate", el.RATES)
def test_the_convolutional_emulation_is_the_host_encoder_and_the_model(rate, emu_dir):
    for n_info in el.N_INFOS:
        got = el.emu_fec_encode(n_info, rate, emu_dir)
        want = el.coded(n_info, rate)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (rate, n_info, f"{bad.size} bytes differ from the model, first at {bad[0]} of {want.size}")
        assert np.array_equal(np.unpackbits(got, count=fec.coded_bits(n_info, rate)), fec.encode(el.info(n_info), rate)), (rate, n_info)


def test_the_reed_solomon_emulation_is_the_host_encoder(emu_dir):
    for k in el.KS:
        want = el.stream(k)
        for in_place in (False, True):
            assert np.array_equal(el.emu_rs_encode(k, in_place, emu_dir), want), (k, in_place)
    for k in (1, 225, 700):                                                                   # and the host encoder the model's
        assert np.array_equal(rs.encode_array(el.data(k)), rl.encode(el.data(k)))


def test_the_tile_emulation_is_soft_tile(emu_dir):
    for period in el.PERIODS:
        for n_out in el.tile_lengths(period):
            assert np.array_equal(el.emu_tile(period, n_out, emu_dir), el.tiled(period, n_out)), (period, n_out)
    assert fec.coded_bits(1, 2) == 14 in el.PERIODS                                           # the period below a dword of the issue


def test_the_sanitized_stand_alone_program(tmp_path):
    """the host build's windows, xor networks, interleaves, compaction, LFSR walk and tile, driven by enc_emu.cpp's own main on
    buffers of exactly the bytes a call may touch, under the address and undefined-behaviour sanitizers: a stand-alone program,
    run once; nothing is loaded into python"""
    run_sanitized_emu("enc_emu.cpp", "ENC_EMU_MAIN", tmp_path, "enc emu ok", extra_flags=("-w",))


# ---- 64-bit positions ----------------------------------------------------------------------------------------------------------------
def test_the_synthetic_stream_is_the_same_on_both_sides():
    for i in (0, 1, 255, 2 ** 32 - 1, 2 ** 32, 2 ** 37 + 12345, 2 ** 40 // 8):
        assert el.emu().enc_emu_hashed_byte(i) == el.hashed_byte(i)
    assert len({el.hashed_byte(i) for i in range(4096)}) > 200                                 # it is no constant


@pytest.mark.parametrize("rate", el.RATES)
def test_units_round_2_32_and_2_40_output_bits(rate):
    """n_info = 2^40, the largest: the units that hold output bits 2^32 and 2^40 and their neighbours, the first unit (steps
    before the stream) and the last three (the tail and the zeros behind it), against the parity formula bit by bit"""
    n_info = 1 << 40
    bits = el.UNIT_BITS[rate]
    last = (fec.coded_bits(n_info, rate) - 1) // bits
    units = [0, 1, last - 1, last, last + 1]
    for at in (1 << 32, 1 << 40):
        units += [at // bits - 1, at // bits, at // bits + 1]
    nonzero = 0
    for u in units:
        got = (C.c_uint32 * 3)()
        assert el.emu().enc_emu_fec_unit_hashed(n_info, rate, u, got) == bits // 32
        want = el.unit_words(u, n_info, rate)
        assert list(got)[: bits // 32] == want, (rate, u, [hex(v) for v in got], [hex(v) for v in want])
        nonzero += any(want)
    assert nonzero >= len(units) - 1 and not any(el.unit_words(last + 1, n_info, rate))


def test_a_step_index_that_does_not_fit_32_bits_changes_the_unit():
    """the check above can tell a truncated index: the unit 2^32 steps further on holds other bits"""
    for rate in el.RATES:
        u = (1 << 32) // el.UNIT_BITS[rate]
        assert el.unit_words(u, 1 << 40, rate) != el.unit_words(u + (1 << 32) // el.UNIT_STEPS[rate], 1 << 40, rate)


def test_the_tile_residue_near_2_43_bits():
    period, n_out = (1 << 43) - 11, 1 << 43
    last = n_out // 32 - 1
    for d in (0, period // 32 - 1, period // 32, period // 32 + 1, last, (1 << 32) // 32, (1 << 32) // 32 + 1):
        got = el.emu().enc_emu_tile_dword_hashed(period, d, n_out)
        assert got == el.tile_word(d, period, n_out), (d, hex(got))
    period = (1 << 42) + 5                                                                     # two copies, the second cut
    for d in (period // 32, period // 32 + 1, last):
        assert el.emu().enc_emu_tile_dword_hashed(period, d, n_out) == el.tile_word(d, period, n_out), d
    assert el.emu().enc_emu_tile_dword_hashed(14, (1 << 38) - 1, n_out - 7) == el.tile_word((1 << 38) - 1, 14, n_out - 7)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order():
    """each call breaks the rule under test and every later one: the earlier refusal must be the one reported.  No call here
    reaches a launch: an out-of-range argument is refused on the host before any device work."""
    lib = enc.load()
    err = lambda: lib.svs_enc_last_error().decode()   # noqa: E731
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    assert p % 4 == 0
    rse = lib.svs_rs_encode_dev
    big = (1 << 37) + 1
    assert rse(None, 0, None, 0, None) == 0                                                            # 1. k = 0: no pointer looked at
    assert rse(None, big, None, 0, None) == I and "SVS_RS_MAX_DATA_BYTES" in err() and "svs_rs_encode_dev" in err()   # 2. the length
    assert rse(None, 2 ** 64 - 1, None, 0, None) == I and "SVS_RS_MAX_DATA_BYTES" in err()
    assert rse(None, 10, p + 5, 0, None) == I and "NULL" in err()                                      # 3. NULL pointers
    assert rse(p, 10, None, 0, None) == I and "NULL" in err()
    assert rse(p, 10, p + 5, 41, None) == CAP and "42" in err()                                        # 4. before the overlap
    assert rse(p, 10, p, 41, None) == CAP
    for out in (p + 1, p + 10, p + 45, p + 50):                                                        # 5. the data is p + 41 .. p + 50
        assert rse(p + 41, 10, out, 42, None) == I and "overlap" in err()
    fece = lib.svs_fec_encode_dev
    for rate in (0, 1, 4, 12, 32, 43, 67, 87, -2):
        assert fece(None, 0, rate, None, 0, None) == I and "rate" in err() and "svs_fec_encode_dev" in err()   # 1. before n_info = 0
    assert fece(None, 0, 34, None, 0, None) == 0                                                       # 2. n_info = 0
    assert fece(None, (1 << 40) + 1, 2, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()       # 3. the length
    assert fece(None, 10, 2, p + 1, 0, None) == I and "NULL" in err()                                  # 4. NULL pointers
    assert fece(p + 1, 10, 2, None, 0, None) == I and "NULL" in err()
    for off in (1, 2, 3):
        assert fece(p + 1, 10, 2, p + 64 + off, 0, None) == I and "aligned" in err()                   # 5. before the capacity
    assert fece(p + 1, 10, 2, p + 64, 3, None) == CAP and "4" in err()                                 # 6. 32 coded bits
    assert fece(p + 1, 10, 78, p + 64, 2, None) == CAP and "3" in err()                                #    S(16) = 19 sent bits
    tile = lib.svs_bits_tile_dev
    assert tile(None, 0, None, 0, 0, None) == 0                                                        # 1. n_out_bits = 0
    assert tile(None, 0, None, 5, 0, None) == I and "SVS_ENC_MAX_TILE_BITS" in err() and "svs_bits_tile_dev" in err()   # 2. the lengths
    assert tile(None, (1 << 43) + 1, None, 5, 0, None) == I and "SVS_ENC_MAX_TILE_BITS" in err()
    assert tile(None, 5, None, (1 << 43) + 1, 0, None) == I and "SVS_ENC_MAX_TILE_BITS" in err()
    assert tile(None, 5, p + 1, 5, 0, None) == I and "NULL" in err()                                   # 3. NULL pointers
    assert tile(p, 5, None, 5, 0, None) == I and "NULL" in err()
    for off in (1, 2, 3):
        assert tile(p, 40, p + off, 64, 0, None) == I and "aligned" in err()                           # 4. before the capacity
    assert tile(p, 40, p + 4, 64, 7, None) == CAP and "8" in err()                                     # 5. before the overlap
    assert tile(p, 40, p + 4, 64, 8, None) == I and "overlap" in err()                                 # 6. bytes 0 .. 4 against 4 .. 11
    assert tile(p + 8, 40, p + 4, 64, 8, None) == I and "overlap" in err()
    assert tile(p + 1, 9, p, 9, 2, None) == I and "overlap" in err()
    # the Python layer raises before the library is asked
    for call in (lambda: enc.rs_encode_device(1, (1 << 37) + 1, 1, 1), lambda: enc.fec_encode_device(1, 8, 4, 4, 4),
                 lambda: enc.fec_encode_device(1, (1 << 40) + 1, 2, 4, 4), lambda: enc.tile_device(1, 0, 4, 8, 1),
                 lambda: enc.tile_device(1, 8, 4, (1 << 43) + 1, 1), lambda: enc.rs_encode(np.zeros(4, np.int32)),
                 lambda: enc.fec_encode(np.zeros(4, np.uint8), 5), lambda: enc.tile(np.zeros(0, np.uint8), 8),
                 lambda: enc.tile(np.zeros(3, np.uint8), -1)):
        with pytest.raises((ValueError, TypeError)):
            call()
    # and the empty forms touch no device
    assert enc.rs_encode(b"").size == 0 and enc.fec_encode(np.zeros(0, np.uint8), 34).size == 0 and enc.tile([1, 0], 0).size == 0
    enc.rs_encode_device(0, 0, 0, 0)
    enc.fec_encode_device(0, 0, 78, 0, 0)
    enc.tile_device(0, 5, 0, 0, 0)


# ---- the public path ----------------------------------------------------------------------------------------------------------------
def test_the_coded_calls_with_a_device_encoder_refuse_before_the_device():
    frames = np.zeros((3, 96, 160), np.uint8)                 # capacity 7 200 at n = 10
    planes = Planes.contiguous(3, 96, 160)
    on_frames = lambda bits, **kw: batch.embed_coded_frames(frames, 20, 10, bits, encoder="device", **kw)   # noqa: E731
    on_device = lambda bits, **kw: batch.embed_coded_device(4, 4, planes, 20, 10, 4, bits.size, 4, 1 << 20, **kw)   # noqa: E731
    for call in (on_frames, on_device):
        with pytest.raises(ValueError, match="whole bytes"):
            call(np.zeros(15, np.uint8), rate=2, outer=True)
        with pytest.raises(ValueError, match=f"capacity.*{8 * 385} payload bits"):
            call(np.zeros(8 * 386, np.uint8), rate=2, outer=True)
        with pytest.raises(ValueError, match=f"capacity of 7200.*{fec.info_bits(7200, 34)} payload bits"):
            call(np.zeros(fec.info_bits(7200, 34) + 1, np.uint8), rate=34)
        with pytest.raises(ValueError, match="margin|matrix"):
            call(np.zeros(8, np.uint8), matrix=2)
        with pytest.raises(ValueError, match="copies"):
            call(np.zeros(8, np.uint8), copies=0)
        with pytest.raises(ValueError, match="bit_offset"):
            call(np.zeros(8, np.uint8), bit_offset=0)
        with pytest.raises(ValueError):
            call(np.zeros(8, np.uint8), rate=4)
        with pytest.raises(ValueError, match="empty"):
            call(np.zeros(0, np.uint8))
    with pytest.raises(ValueError, match="encoder"):
        batch.embed_coded_frames(frames, 20, 10, np.zeros(8, np.uint8), encoder="gpu")
    with pytest.raises(ValueError, match="workspace"):
        batch.embed_coded_device(4, 4, planes, 20, 10, 4, 64, 4, 3)
    with pytest.raises(ValueError, match="workspace"):
        batch.embed_coded_device(4, 4, planes, 20, 10, 4, 64, 6, 1 << 20)


def test_the_workspace_holds_every_stage_rounded_to_four_bytes():
    cap = 7200
    assert batch.coded_workspace_bytes(10, 2, 1, False, cap) == 4                              # 32 coded bits
    assert batch.coded_workspace_bytes(11, 2, 1, False, cap) == 8                              # 34
    assert batch.coded_workspace_bytes(11, 2, 2, False, cap) == 8 + 12                         # and 68 tiled bits
    assert batch.coded_workspace_bytes(11, 2, None, False, cap) == 8 + 900
    assert batch.coded_workspace_bytes(11, 2, 1000, False, cap) == 8 + 900                     # cut at the capacity
    k = 10
    inner = 8 * rs.coded_bytes(k)
    assert batch.coded_workspace_bytes(8 * k, 34, 1, True, cap) == 44 + -(-fec.coded_bits(inner, 34) // 32) * 4
    assert soft.tile([1, 0, 1], 7).tolist() == [1, 0, 1, 1, 0, 1, 1]
