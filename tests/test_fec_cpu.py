"""CPU tier of the convolutional code (include/svsfec.h, libsvsfec.so, svsdct/fec.py): the library's exports, the host encoder
against the NumPy model of tests/fec_lib.py, the refusals in the documented order, the host build of csrc/svs_fec.hpp against
the model on the GPU test's inputs (and once as a stand-alone program under the address and undefined-behaviour sanitizers),
the tie rules, and the channel experiment of the README's table.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import channel_lib as cl
import fec_lib as fl
from testlib import check_header_is_plain_c, check_library_exports, run_sanitized_emu
from svsdct import batch, fec, native

I, CAP = native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_the_header():
    check_library_exports("svsfec.h", fec, "svs_fec", 7)
    assert fec.ABI_VERSION == 1


def test_the_header_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, ("svsdct.h", "svsfec.h"), "SVS_FEC_SEGMENT == 512 && SVS_ERR_CAPACITY == -4")


def test_lengths():
    lib = fec.load()
    for rate in (2, 3):
        for n in (0, 1, 7, 506, 10 ** 9, 1 << 40):
            assert lib.svs_fec_coded_bits(n, rate) == fec.coded_bits(n, rate) == fl.coded_bits(n, rate) == rate * (n + 6)
        for cap in (0, 1, 11, 12, 13, 14, 15, 20, 21, 7200, 10 ** 12):
            assert lib.svs_fec_info_bits(cap, rate) == fec.info_bits(cap, rate) == fl.info_bits(cap, rate)
            n = fec.info_bits(cap, rate)
            assert fec.coded_bits(n, rate) <= cap or n == 0
            assert fec.coded_bits(n + 1, rate) > cap
    assert fec.info_bits(7200, 3) == 2394 and fec.info_bits(7200, 2) == 3594
    assert lib.svs_fec_coded_bits(5, 4) == 0 == lib.svs_fec_info_bits(100, 1) == lib.svs_fec_coded_bits((1 << 40) + 1, 2)
    assert lib.svs_fec_coded_bits(2 ** 64 - 1, 3) == 0                          # a coded length that would leave uint64
    for bad in (0, 1, 4, True, None, 2.5):
        with pytest.raises(ValueError):
            fec.coded_bits(8, bad)


@pytest.mark.parametrize("rate", fl.RATES)
def test_the_encoder_is_the_models(rate):
    rng = np.random.default_rng(3)
    for n_info in (1, 2, 7, 8, 9, 506, 507, 1030):
        info = rng.integers(0, 2, n_info).astype(np.uint8)
        want = fl.encode(info, rate)
        assert np.array_equal(fec.encode(info, rate), want), (rate, n_info)
        # the raw call: exactly ceil(n_coded / 8) bytes, the pad bits 0, nothing behind them, the input untouched
        packed = np.packbits(info)
        keep = packed.copy()
        nbytes = (want.size + 7) // 8
        out = np.full(nbytes + 8, 0xEE, np.uint8)
        got = C.c_uint64(7)
        assert fec.load().svs_fec_encode(packed.ctypes.data, n_info, rate, out.ctypes.data, nbytes, C.byref(got)) == 0
        assert got.value == want.size and np.array_equal(out[:nbytes], np.packbits(want)) and (out[nbytes:] == 0xEE).all()
        assert np.array_equal(packed, keep)
        assert fec.load().svs_fec_encode(packed.ctypes.data, n_info, rate, out.ctypes.data, nbytes, None) == 0    # n_coded_out may be NULL
    assert fec.encode([], rate).size == 0


def test_refusals_in_the_documented_order():
    """each call breaks the rule under test and every later one: the earlier refusal must be the one reported.  No call here
    reaches a launch: an out-of-range argument is refused on the host before any device work."""
    lib = fec.load()
    err = lambda: lib.svs_fec_last_error().decode()   # noqa: E731
    buf = np.zeros(64, np.uint8)
    p, odd, big = buf.ctypes.data, buf.ctypes.data + 1, (1 << 40) + 1
    assert p % 4 == 0
    decoders = {"svs_fec_decode_soft_dev": lib.svs_fec_decode_soft_dev, "svs_fec_decode_weights_dev": lib.svs_fec_decode_weights_dev}
    for name, fn in decoders.items():
        for rate in (0, 1, 4, -2):
            assert fn(None, big, rate, None, 0, None) == I and "rate" in err() and name in err()       # 1. the rate
        for rate in (2, 3):
            assert fn(None, 0, rate, None, 0, None) == 0                                               # 2. n_info = 0: no pointer looked at
            assert fn(None, big, rate, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()        # 3. the length
            assert fn(None, 2 ** 64 - 1, rate, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()
            assert fn(None, 100, rate, odd, 0, None) == I and "NULL" in err()                          # 4. NULL pointers
            assert fn(odd, 100, rate, None, 0, None) == I and "NULL" in err()
            assert fn(p, 100, rate, p, 12, None) == CAP and "13" in err()                              # 6. the output: ceil(100 / 8) = 13
        assert fn(p, 1, 1, p, 0, None) == I and "rate" in err()
    assert lib.svs_fec_decode_weights_dev(odd, 100, 2, p, 0, None) == I and "aligned" in err()        # 5. before the capacity
    assert lib.svs_fec_decode_weights_dev(odd + 1, 100, 2, p, 13, None) == I and "aligned" in err()
    assert lib.svs_fec_decode_soft_dev(odd, 100, 2, p, 12, None) == CAP                                # soft bytes: any alignment
    enc = lib.svs_fec_encode
    got = C.c_uint64(9)
    assert enc(None, big, 5, None, 0, None) == I and "rate" in err()
    assert enc(None, 0, 2, None, 0, C.byref(got)) == 0 and got.value == 0
    assert enc(None, big, 2, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()
    assert enc(None, 10, 2, p, 0, None) == I and "NULL" in err()
    assert enc(p, 10, 2, None, 0, None) == I and "NULL" in err()
    assert enc(p, 10, 2, p + 32, 3, None) == CAP and "4" in err()                                      # 2 * 16 bits: 4 bytes
    assert enc(p, 10, 3, p + 32, 5, None) == CAP                                                       # 3 * 16 bits: 6 bytes
    # the Python layer raises before the library is asked
    for call in (lambda: fec.decode_soft(np.zeros(10, np.uint8), 1, 2), lambda: fec.decode_soft(np.zeros(14, np.int32), 1, 2),
                 lambda: fec.decode_weights(np.zeros(14, np.uint8), 1, 2), lambda: fec.decode_soft(np.zeros(14, np.uint8), 1, 5),
                 lambda: fec.coded_bits(-1, 2), lambda: fec.coded_bits((1 << 40) + 1, 2)):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_the_coded_frame_calls_refuse_before_the_library_is_loaded():
    frames = np.zeros((1, 16, 16), np.uint8)                  # capacity 40 at n = 10
    with pytest.raises(ValueError, match="margin|matrix"):
        batch.embed_coded_frames(frames, 20, 10, [1, 0, 1], matrix=2, steps=np.full(64, 20))
    with pytest.raises(ValueError, match="margin|matrix"):
        batch.extract_coded_frames(frames, 20, 10, 3, matrix=2)
    with pytest.raises(ValueError, match="capacity"):
        batch.embed_coded_frames(frames, 20, 10, np.zeros(15, np.uint8), rate=2)          # 42 coded bits
    with pytest.raises(ValueError, match="capacity"):
        batch.extract_coded_frames(frames, 20, 10, 15, rate=2)
    for bad in (dict(rate=4), dict(copies=0), dict(bit_offset=3)):
        with pytest.raises(ValueError):
            batch.embed_coded_frames(frames, 20, 10, [1, 0, 1], **bad)
    with pytest.raises(ValueError):
        batch.embed_coded_frames(frames, 20, 10, [])


# ---- the model and the host build of svs_fec.hpp -----------------------------------------------------------------------------------
def test_the_models_own_pieces():
    assert fl.GENERATORS[3] == (0b1011011, 0b1111001, 0b1110101) and all(g & 1 and g >> 6 for g in fl.GENERATORS[3])
    assert list(fl.encode([1], 2)[:4]) == [1, 1, 0, 1]        # reg 1000000 -> 1, 1; reg 0100000 -> 0 (133 has no bit 5), 1
    assert list(fl.weights_of_soft(np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8))) == [-1, -255, 1, 255]
    assert list(fl.weights_of_int32(np.array([fl.I32_MIN, -32768, -5, 0, 32767, 32768, fl.I32_MAX], np.int32))) == \
        [-32767, -32767, -5, 0, 32767, 32767, 32767]
    assert 640 * 3 * 32767 < 1 << 30                          # the header's bound
    sg = fl._branch_signs(3)
    assert set(np.unique(sg)) == {-1, 1} and len({tuple(r) for r in sg}) == 8


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fec_emu")


@pytest.mark.parametrize("rate", fl.RATES)
@pytest.mark.parametrize("kind", fl.SOFT_KINDS + fl.INT32_KINDS)
def test_the_host_build_is_the_model_on_the_gpu_tests_inputs(kind, rate, emu_dir):
    for n_info in fl.N_INFOS:
        values, info, want = fl.case(kind, n_info, rate)
        got = fl.emu_decode(values, n_info, rate, emu_dir)
        assert np.array_equal(got, want), (kind, rate, n_info, int((got != want).sum()))
        if kind == "clean":
            assert np.array_equal(want, info), (kind, rate, n_info)


def test_the_noiseless_round_trip_is_the_identity(emu_dir):
    rng = np.random.default_rng(9)
    for rate in fl.RATES:
        for n_info in (1, 5, 8, 506, 507, 1500):
            info = rng.integers(0, 2, n_info).astype(np.uint8)
            coded = fec.encode(info, rate)
            for margin in (0, 127):
                soft = fl.soft_of_bits(coded, margin)
                assert np.array_equal(fl.decode_soft(soft, n_info, rate), info)
                assert np.array_equal(fl.emu_decode(soft, n_info, rate, emu_dir), info)
            assert np.array_equal(fl.decode_full(fl.weights_of_soft(soft), n_info, rate), info)
            assert np.array_equal(fl.emu_decode((2 * coded.astype(np.int32) - 1) * 40000, n_info, rate, emu_dir), info)


def test_the_tie_rules_on_hard_decisions(emu_dir):
    """weights of +-1: path metrics are small integers and equal sums are frequent, so both tie rules - p1 wins only when
    strictly larger, the traceback starts from the lowest-numbered best state - decide bits.  Ties must occur on this input."""
    rng = np.random.default_rng(31)
    for rate in fl.RATES:
        n_info = 1600
        coded = fl.encode(rng.integers(0, 2, n_info).astype(np.uint8), rate)
        noisy = coded ^ (rng.random(coded.size) < 0.09).astype(np.uint8)
        soft = fl.soft_of_bits(noisy, 0)
        counts = {}
        want = fl.decode_soft(soft, n_info, rate, counts)
        assert counts["ties"] > counts["steps"], counts
        assert np.array_equal(fl.emu_decode(soft, n_info, rate, emu_dir), want)
    for kind in ("all00", "all80"):
        counts = {}
        values, _, want = fl.case(kind, 1019, 2)
        fl.decode_soft(values, 1019, 2, counts)
        assert counts["ties"] > 8 * counts["steps"], counts
        assert np.array_equal(fl.emu_decode(values, 1019, 2, emu_dir), want)
    # weights of 0: every compare a tie and no window has a unique best state - the lowest-numbered one starts the traceback
    counts, zeros = {}, np.zeros(fl.coded_bits(1019, 3), np.int32)
    want = fl.decode_int32(zeros, 1019, 3, counts)
    assert counts["start_ties"] >= 1 and counts["ties"] > 50 * counts["steps"], counts
    assert not want.any() and np.array_equal(fl.emu_decode(zeros, 1019, 3, emu_dir), want)


def test_the_sanitized_stand_alone_program(tmp_path):
    """the host build's step and traceback, driven by fec_emu.cpp's own main, under the address and undefined-behaviour
    sanitizers: a stand-alone program, run once; nothing is loaded into python"""
    run_sanitized_emu("fec_emu.cpp", "FEC_EMU_MAIN", tmp_path, "fec emu ok")


# ---- the README's table -----------------------------------------------------------------------------------------------------------
def test_the_channel_table(capsys):
    """delta = 20, n = 10, reference rule, channel_lib.survival's cover, seed and frames: what the 7 200 capacity bits deliver"""
    rep = cl.survival(20, 10, None, "reference", 75)
    rows = [("three copies, soft vote", 2400, "/".join(map(str, rep["single"])) + " a copy", rep["soft"], f"{rep['majority']} (majority)", "")]
    cells = {}
    for rate, q in ((3, 75), (2, 75), (3, 60), (2, 60), (2, 85)):
        r = cells[rate, q] = fl.coded_survival(rate, q)
        rows.append((f"rate 1/{rate}, Q = {q}", r["n_info"], r["coded_wrong"], r["soft"], r["hard"], r["full"]))
    import stepped_lib as st
    m = fl.coded_survival(2, 40, steps=st.matched(75, 2))
    rows.append(("rate 1/2, matched(75, 2), Q = 40", m["n_info"], m["coded_wrong"], m["soft"], m["hard"], m["full"]))
    m3 = fl.coded_survival(3, 40, steps=st.matched(75, 2))
    rows.append(("rate 1/3, matched(75, 2), Q = 40", m3["n_info"], m3["coded_wrong"], m3["soft"], m3["hard"], m3["full"]))
    with capsys.disabled():
        print("\n| what the 7 200 capacity bits carry | payload bits | wrong coded bits | wrong payload bits, soft | hard | untruncated Viterbi, soft |")
        print("|---|---|---|---|---|---|")
        for row in rows:
            print("| " + " | ".join(str(v) for v in row) + " |")
    assert cells[2, 75]["n_info"] == 3594 and cells[3, 75]["n_info"] == 2394
    assert cells[2, 75]["soft"] == 0 and cells[3, 75]["soft"] == 0
    assert cells[2, 75]["hard"] > 0
    assert rep["soft"] > 0
