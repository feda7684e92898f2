"""CPU tier of the punctured codes (include/svsfec.h "Punctured codes", svsdct/fec.py): the lengths of the library, the binding
and the NumPy model of tests/fec_punctured_lib.py; the host encoder against the model; the refusals in the documented order; the
host build of csrc/svs_fec.hpp's window load against the model on the GPU test's inputs (and once as a stand-alone program under
the address and undefined-behaviour sanitizers); and the channel experiment of the README's punctured table.  Nothing here
needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import fec_lib as fl
import fec_punctured_lib as pl
from testlib import run_sanitized_emu
from svsdct import batch, fec, native

I, CAP = native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY


def test_the_binding_names_the_headers_codes():
    assert fec.RATES == (2, 3) and fec.PUNCTURED == pl.CODES == (fec.RATE_2_3, fec.RATE_3_4, fec.RATE_5_6, fec.RATE_7_8)
    for code in pl.CODES:
        out0, out1 = fec.PATTERNS[code]
        assert ("".join(map(str, out0)), "".join(map(str, out1))) == pl.PATTERNS[code]
        p, k, pre = pl.period(code)
        assert k == p + 1 and pre[0] == 0 and all(b > a for a, b in zip(pre, pre[1:] + [k]))    # every step sends a bit


def test_S_against_a_count_and_python_integers():
    lib = pl.emu()
    for code in pl.CODES:
        m = pl.mask(200, code)
        for t in range(200):
            want = int(m[: 2 * t].sum())
            assert pl.S(t, code) == fec.sent_before(t, code) == lib.fec_punctured_emu_sent_before(t, code) == want
        p, k, pre = pl.period(code)
        t = (1 << 40) + 6
        want = (t // p) * k + pre[t % p]
        assert want > 1 << 40
        assert lib.fec_punctured_emu_sent_before(t, code) == want == fec.load().svs_fec_coded_bits(1 << 40, code) == fec.coded_bits(1 << 40, code)


def test_lengths():
    lib = fec.load()
    emu = pl.emu()
    for code in pl.CODES:
        p, k, _ = pl.period(code)
        for n in (0, 1, 7, 506, 10 ** 9, 1 << 40):
            assert lib.svs_fec_coded_bits(n, code) == fec.coded_bits(n, code) == pl.coded_bits(n, code) == pl.S(n + 6, code)
        # every residue of K and of P, around the first payload bit, further out, and far out
        caps = list(range(0, 4 * k * p + 40)) + [7200 + i for i in range(2 * k)] + [10 ** 12 + i for i in range(2 * k)] + [2 ** 64 - 1]
        for cap in caps:
            n = fec.info_bits(cap, code)
            assert lib.svs_fec_info_bits(cap, code) == n == pl.info_bits(cap, code), (code, cap)
            assert emu.fec_punctured_emu_steps_that_fit(cap, code) == pl.steps_that_fit(cap, code), (code, cap)
            if n > 0 and n <= 1 << 40:
                assert fec.coded_bits(n, code) <= cap < fec.coded_bits(n + 1, code), (code, cap)
            elif n == 0:
                assert fec.coded_bits(1, code) > cap, (code, cap)
        assert lib.svs_fec_coded_bits((1 << 40) + 1, code) == 0
        with pytest.raises(ValueError):
            fec.coded_bits((1 << 40) + 1, code)
    assert [fec.info_bits(7200, c) for c in pl.CODES] == [4794, 5394, 5994, 6294]
    for bad in (0, 1, 4, 5, 12, 24, 79, True, None, 2.5):
        with pytest.raises(ValueError, match="rate"):
            fec.coded_bits(8, bad)
    for bad in (0, 1, 4, 5, 12, 24, 79):
        assert lib.svs_fec_coded_bits(8, bad) == 0 == lib.svs_fec_info_bits(7200, bad)


@pytest.mark.parametrize("code", pl.CODES)
def test_the_encoder_is_the_models(code):
    rng = np.random.default_rng(3)
    p, _, _ = pl.period(code)
    n_infos = (1, 2, 7, 8, 9, 506, 507) + tuple(range(1019, 1019 + p))
    assert {(n + 6) % p for n in n_infos} == set(range(p))
    for n_info in n_infos:
        info = rng.integers(0, 2, n_info).astype(np.uint8)
        want = pl.encode(info, code)
        assert want.size == pl.coded_bits(n_info, code)
        assert np.array_equal(fec.encode(info, code), want), (code, n_info)
        # the raw call: exactly ceil(n_sent / 8) bytes, the pad bits 0, nothing behind them, the input untouched
        packed = np.packbits(info)
        keep = packed.copy()
        nbytes = (want.size + 7) // 8
        out = np.full(nbytes + 8, 0xEE, np.uint8)
        got = C.c_uint64(7)
        assert fec.load().svs_fec_encode(packed.ctypes.data, n_info, code, out.ctypes.data, nbytes, C.byref(got)) == 0
        assert got.value == want.size and np.array_equal(out[:nbytes], np.packbits(want)) and (out[nbytes:] == 0xEE).all()
        assert np.array_equal(packed, keep)
    assert fec.encode([], code).size == 0


def test_refusals_in_the_documented_order():
    """each call breaks the rule under test and every later one: the earlier refusal must be the one reported.  No call here
    reaches a launch."""
    lib = fec.load()
    err = lambda: lib.svs_fec_last_error().decode()   # noqa: E731
    buf = np.zeros(64, np.uint8)
    p, odd, big = buf.ctypes.data, buf.ctypes.data + 1, (1 << 40) + 1
    assert p % 4 == 0
    decoders = {"svs_fec_decode_soft_dev": lib.svs_fec_decode_soft_dev, "svs_fec_decode_weights_dev": lib.svs_fec_decode_weights_dev}
    for name, fn in decoders.items():
        for rate in (0, 1, 4, 5, 12, 24, 79, -23):
            assert fn(None, big, rate, None, 0, None) == I and "rate" in err() and name in err()       # 1. the rate
        for code in pl.CODES:
            assert fn(None, 0, code, None, 0, None) == 0                                               # 2. n_info = 0
            assert fn(None, big, code, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()        # 3. the length
            assert fn(None, 100, code, odd, 0, None) == I and "NULL" in err()                          # 4. NULL pointers
            assert fn(odd, 100, code, None, 0, None) == I and "NULL" in err()
            assert fn(p, 100, code, p, 12, None) == CAP and "13" in err()                              # 6. the output
    for code in pl.CODES:
        assert lib.svs_fec_decode_weights_dev(odd, 100, code, p, 0, None) == I and "aligned" in err()  # 5. before the capacity
        assert lib.svs_fec_decode_soft_dev(odd, 100, code, p, 12, None) == CAP                         # soft bytes: any alignment
    enc = lib.svs_fec_encode
    got = C.c_uint64(9)
    for rate in (0, 1, 4, 5, 12, 24, 79):
        assert enc(None, big, rate, None, 0, None) == I and "rate" in err()
    assert enc(None, 0, 34, None, 0, C.byref(got)) == 0 and got.value == 0
    assert enc(None, big, 34, None, 0, None) == I and "SVS_FEC_MAX_INFO_BITS" in err()
    assert enc(None, 10, 34, p, 0, None) == I and "NULL" in err()
    assert enc(p, 10, 34, None, 0, None) == I and "NULL" in err()
    assert pl.coded_bits(10, 34) == 22
    assert enc(p, 10, 34, p + 32, 2, None) == CAP and "3" in err()                                     # 22 bits: 3 bytes
    assert enc(p, 10, 34, p + 32, 3, None) == 0
    # the Python layer raises before the library is asked
    for call in (lambda: fec.decode_soft(np.zeros(14, np.uint8), 1, 23), lambda: fec.decode_weights(np.zeros(11, np.uint8), 1, 23),
                 lambda: fec.decode_soft(np.zeros(11, np.uint8), 1, 24), lambda: fec.coded_bits(-1, 56)):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_the_coded_frame_calls_take_the_codes_and_refuse_before_the_library_is_loaded():
    frames = np.zeros((1, 16, 16), np.uint8)                  # capacity 40 at n = 10
    assert fec.info_bits(40, 34) == 24 and fec.coded_bits(24, 34) == 40
    with pytest.raises(ValueError, match="capacity"):
        batch.embed_coded_frames(frames, 20, 10, np.zeros(25, np.uint8), rate=34)
    with pytest.raises(ValueError, match="capacity"):
        batch.extract_coded_frames(frames, 20, 10, 25, rate=34)
    for bad in (12, 24, 79):
        with pytest.raises(ValueError, match="rate"):
            batch.embed_coded_frames(frames, 20, 10, [1, 0, 1], rate=bad)


# ---- the model and the host build ---------------------------------------------------------------------------------------------------
def test_the_models_own_pieces():
    assert [pl.period(c)[:2] for c in pl.CODES] == [(2, 3), (3, 4), (5, 6), (7, 8)]
    assert pl.period(78)[2] == [0, 2, 3, 4, 5, 6, 7]
    info = np.array([1, 0, 1, 1], np.uint8)
    mother = fl.encode(info, 2)
    assert list(pl.encode(info, 34)) == [mother[i] for i in (0, 1, 2, 5, 6, 7, 8, 11, 12, 13, 14, 17, 18, 19)]
    w = np.arange(1, pl.coded_bits(4, 23) + 1)
    assert list(pl.depuncture(w, 4, 23)[:8]) == [1, 2, 3, 0, 4, 5, 6, 0]


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fec_punctured_emu")


@pytest.mark.parametrize("code", pl.CODES)
@pytest.mark.parametrize("kind", pl.KINDS)
def test_the_host_build_is_the_model_on_the_gpu_tests_inputs(kind, code, emu_dir):
    for n_info in pl.lengths(kind):
        values, _, want, _ = pl.case(kind, n_info, code)
        got = pl.emu_decode(values, n_info, code, emu_dir)
        assert np.array_equal(got, want), (kind, code, n_info, int((got != want).sum()))


def test_the_noiseless_round_trip_is_the_identity(emu_dir):
    rng = np.random.default_rng(9)
    for code in pl.CODES:
        for n_info in (1, 5, 8, 506, 507, 1500):
            info = rng.integers(0, 2, n_info).astype(np.uint8)
            coded = fec.encode(info, code)
            for margin in (0, 127):
                soft = fl.soft_of_bits(coded, margin)
                assert np.array_equal(pl.decode_soft(soft, n_info, code), info), (code, n_info, margin)
                assert np.array_equal(pl.emu_decode(soft, n_info, code, emu_dir), info), (code, n_info, margin)
            assert np.array_equal(pl.emu_decode((2 * coded.astype(np.int32) - 1) * 40000, n_info, code, emu_dir), info)


def test_the_sanitized_stand_alone_program(tmp_path):
    """the host build's window load, driven by fec_punctured_emu.cpp's own main, under the address and undefined-behaviour
    sanitizers: a stand-alone program, run once; nothing is loaded into python"""
    run_sanitized_emu("fec_punctured_emu.cpp", "FEC_PUNCTURED_EMU_MAIN", tmp_path, "fec punctured emu ok")


# ---- the README's table -------------------------------------------------------------------------------------------------------------
def test_the_channel_table(capsys):
    """delta = 20, n = 10, reference rule, channel_lib.survival's cover, seed and frames: what the 7 200 capacity bits deliver
    at the punctured rates.  A cell: wrong coded bits before decoding / wrong payload bits, soft decisions / hard decisions"""
    qualities = (85, 80, 75, 70)
    cells = {(code, q): pl.coded_survival(code, q) for code in pl.CODES for q in qualities}
    with capsys.disabled():
        print("\n| rate (payload bits of 7 200) | " + " | ".join(f"Q = {q}" for q in qualities) + " |")
        print("|---|" + "---|" * len(qualities))
        for code in pl.CODES:
            row = [f"{c['coded_wrong']} / {c['soft']} / {c['hard']}" for c in (cells[code, q] for q in qualities)]
            print(f"| {pl.NAMES[code]} ({cells[code, 75]['n_info']}) | " + " | ".join(row) + " |")
    assert [cells[c, 75]["n_info"] for c in pl.CODES] == [4794, 5394, 5994, 6294]
    for code in (23, 34):
        assert cells[code, 75]["soft"] == 0 and cells[code, 75]["hard"] > 0, (code, cells[code, 75])
    assert cells[56, 75]["soft"] > 0
    assert cells[56, 80]["soft"] == 0 and cells[78, 80]["soft"] > 0
