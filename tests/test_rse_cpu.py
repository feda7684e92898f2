"""CPU tier of errors-and-erasures decoding (include/svsrse.h, libsvsrse.so, svsdct/rse.py): the library's exports, the format's
known answers, the NumPy model of tests/rse_lib.py against the format's definition on every input of the GPU test, the two facts
the format rests on (2 e + f <= 32 returns the sent word, 2 e + f = 33 returns 255), the host build of the new steps of
csrc/svs_rs.hpp against the model (and once as a stand-alone program under the address and undefined-behaviour sanitizers), the
refusals in the documented order, fec.steps_of_sent_bits against brute force, the refusals of lost_frames, and the lost-frame
experiment of the README's table.  Nothing here needs a GPU."""

import numpy as np
import pytest

import rs_lib as rl
import rse_lib as el
from testlib import check_header_is_plain_c, check_library_exports, run_sanitized_emu
from svsdct import batch, fec, native, rs, rse

I, CAP = native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_the_header():
    # both Reed-Solomon libraries hold the kernel and the tables of csrc/svs_rs_decode.hpp and are loaded into one process: a
    # dynamic symbol of either would be interposed by the other's
    check_library_exports("svsrse.h", rse, "svs_rse", 3, hidden=("decode_kernel", "d_field", "d_lfsr"))
    assert rse.ABI_VERSION == 1


def test_the_header_is_plain_c(tmp_path):
    for order in (("svsdct.h", "svsfec.h", "svsrs.h", "svsrse.h"), ("svsrse.h", "svsrs.h"), ("svsrse.h",)):
        check_header_is_plain_c(tmp_path, order, "SVS_RS_PARITY == 32 && SVS_RS_UNCORRECTABLE == 255 && SVS_RSE_MAX_ERASED == 32 && "
                                                 "SVS_ERR_CAPACITY == -4 && SVS_RS_MAX_DATA_BYTES == (1ull << 37)")


# ---- the format's known answers ---------------------------------------------------------------------------------------------------
def test_the_known_answers():
    sent = rl.encode(np.arange(10, dtype=np.uint8))
    assert sent.size == 42 and rl.EXP[41] == 0xD4
    gamma = el.erasure_locator(np.array([[41, 0] + [0] * 30]), np.array([2]))[0]
    assert list(gamma[:3]) == [0x01, 0xD5, 0xD4] and not gamma[3:].any()

    def run(erased, received):
        mask = np.zeros(42, np.uint8)
        mask[erased] = 1
        stream, status, _ = el.decode(received, 10, mask)
        return stream, int(status[0])

    first_ff = sent.copy()
    first_ff[0] = 0xFF
    stream, status = run([0, 41], first_ff)
    assert status == 1 and np.array_equal(stream, sent)
    assert run([0, 41], sent)[1] == 0
    wrong = sent.copy()
    wrong[:32] = 0xFF
    assert (wrong != sent).sum() == 32
    stream, status = run(np.arange(32), wrong)
    assert status == 32 and np.array_equal(stream, sent)
    wrong = sent.copy()
    wrong[:31], wrong[41] = 0xFF, 0x04
    assert (wrong != sent).sum() == 32
    stream, status = run(np.arange(31), wrong)
    assert status == 255 and np.array_equal(stream, wrong)
    assert run(np.arange(33), sent)[1] == 255


# ---- the model against the definition ---------------------------------------------------------------------------------------------
MUST = {"erasures32": 32, "right": 11, "right0": 0, "ends": 17, "over": 255, "f33": 255}


@pytest.mark.parametrize("kind", el.KINDS)
def test_the_model_meets_the_definition(kind):
    """every input of the GPU test: what the model calls decoded is a code word that differs from the received one in exactly
    `status` bytes, e of them outside the mask with 2 e + f <= 32; what it calls uncorrectable is as received - and each kind
    gives what its construction forces"""
    for k in el.KS:
        received, mask, sent, decoded, status, counts = el.case(kind, k)
        el.check_definition(received, decoded, status, k, mask)
        good = status != el.UNCORRECTABLE
        assert counts == (int(status[good].sum()), int((~good).sum()))
        c = np.arange(rl.codewords(k))
        if kind in MUST:
            assert (status == MUST[kind]).all(), (kind, k, status)
        if kind in ("mixed", "values"):
            assert np.array_equal(status, 2 * (c % 17) + (32 - 2 * (c % 17)) // 2), (kind, k)
        if kind in ("over", "f33"):
            assert np.array_equal(decoded, received)
        elif kind != "random":
            assert np.array_equal(decoded, sent), (kind, k)
        if kind == "burst32":
            assert (status == 32).all()
            assert (rl.decode(received, k)[1] == rl.UNCORRECTABLE).any(), "without the mask a codeword must fail"
        if kind == "values":
            assert set(np.unique(mask)) <= {0, 1, 0x80, 0xFF} and (k < 64 * 223 or len(set(np.unique(mask))) == 4)


def test_without_erasures_the_model_is_the_parents():
    for kind in el.NOMASK_KINDS:
        for k in el.KS:
            received, want, status, counts = rl.case(kind, k)
            for mask in (None, np.zeros(received.size, np.uint8)):
                got, got_status, got_counts = el.decode(received, k, mask)
                assert np.array_equal(got, want) and np.array_equal(got_status, status) and got_counts == counts, (kind, k)


def _draw(rng, k, f, e):
    """a sent stream and what is received with f erased (and wrong) and e more wrong bytes in every codeword"""
    sent = rl.encode(rng.integers(0, 256, k).astype(np.uint8))
    received, mask = sent.copy(), np.zeros(sent.size, np.uint8)
    for c in range(rl.codewords(k)):
        places = rng.choice(int(rl.lengths(k)[c]) + 32, f + e, replace=False)
        rl._hit(received, rng, k, c, places)
        mask[[el._at(k, c, int(i)) for i in places[:f]]] = 1
    return sent, received, mask


def test_within_reach_comes_back_and_one_past_it_never_does():
    """fresh seeds: 2 e + f <= 32 always returns the sent word with status e + f; 2 e + f = 33 always returns 255 - a word
    within reach would lie e + e' + f < 33 from the sent one, so the failure is forced, not merely likely"""
    rng = np.random.default_rng(2026)
    for k in (1, 5, 100, 223, 700):
        for f in range(0, 33):
            e = int(rng.integers(0, (32 - f) // 2 + 1))
            sent, received, mask = _draw(rng, k, f, e)
            decoded, status, _ = el.decode(received, k, mask)
            assert np.array_equal(decoded, sent) and (status == e + f).all(), (k, f, e)
        for f in range(1, 33, 2):
            sent, received, mask = _draw(rng, k, f, (33 - f) // 2)
            decoded, status, _ = el.decode(received, k, mask)
            assert np.array_equal(decoded, received) and (status == 255).all(), (k, f)


# ---- the host build against the model -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rse_emu")


@pytest.mark.parametrize("kind", el.KINDS)
def test_the_host_build_is_the_model_on_the_gpu_tests_inputs(kind, emu_dir):
    for k in el.KS:
        received, mask, _, want, status, counts = el.case(kind, k)
        keep = mask.copy()
        got, got_status, got_counts = el.emu_decode(received, k, mask, (11, 5), emu_dir)
        assert np.array_equal(got, want) and np.array_equal(got_status, status), (kind, k)
        assert got_counts == (11 + counts[0], 5 + counts[1]), (kind, k)
        assert np.array_equal(mask, keep)


@pytest.mark.parametrize("kind", el.NOMASK_KINDS)
def test_the_host_build_without_erasures_is_the_parents_model(kind, emu_dir):
    for k in el.KS:
        received, want, status, counts = rl.case(kind, k)
        for mask in (None, np.zeros(received.size, np.uint8)):
            got, got_status, got_counts = el.emu_decode(received, k, mask, (0, 0), emu_dir)
            assert np.array_equal(got, want) and np.array_equal(got_status, status) and got_counts == counts, (kind, k)


def test_the_sanitized_stand_alone_program(tmp_path):
    """the host build's screening with a mask, erasure locator, Berlekamp-Massey, root search and Forney, driven by rs_emu.cpp's
    -DRSE_EMU_MAIN main, under the address and undefined-behaviour sanitizers: a stand-alone program, run once; nothing is loaded into python"""
    run_sanitized_emu("rs_emu.cpp", "RSE_EMU_MAIN", tmp_path, "rse emu ok")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order():
    """each call breaks the rule under test and every later one: the earlier refusal must be the one reported.  No call here
    reaches a launch: an out-of-range argument is refused on the host before any device work."""
    lib = rse.load()
    err = lambda: lib.svs_rse_last_error().decode()   # noqa: E731
    buf = np.zeros(64, np.uint8)
    p, big = buf.ctypes.data, (1 << 37) + 1
    assert p % 4 == 0
    dec = lib.svs_rse_decode_dev
    for mask in (None, p + 3):
        assert dec(None, 0, mask, None, 0, p + 1, None) == 0                                            # 1. k = 0: no pointer looked at
        assert dec(None, big, mask, None, 0, p + 1, None) == I and "SVS_RS_MAX_DATA_BYTES" in err() and "svs_rse_decode_dev" in err()   # 2.
        assert dec(None, 2 ** 64 - 1, mask, None, 0, p + 1, None) == I and "SVS_RS_MAX_DATA_BYTES" in err()
        assert dec(None, 500, mask, p, 0, p + 1, None) == I and "NULL" in err()                         # 3. NULL pointers
        assert dec(p + 1, 500, mask, None, 0, p + 1, None) == I and "NULL" in err()
        for off in (1, 2, 3):
            assert dec(p + 1, 500, mask, p, 0, p + off, None) == I and "aligned" in err()               # 4. before the capacity
        assert dec(p + 1, 500, mask, p, 2, p + 4, None) == CAP and "3" in err()                         # 5. ceil(500 / 223) = 3
        assert dec(p + 1, 500, mask, p, 2, None, None) == CAP
    # the Python layer raises before the library is asked
    for call in (lambda: rse.decode(b"\x00" * 40, 10), lambda: rse.decode(np.zeros(42, np.int32), 10),
                 lambda: rse.decode(b"\x00" * 42, 10, b"\x00" * 41), lambda: rse.decode_device(1, (1 << 37) + 1, 0, 1, 1),
                 lambda: rse.mask(10, [(3, 2)]), lambda: rse.mask(10, [(-1, 2)]), lambda: rse.mask(-1, [])):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_the_mask_helper():
    assert rse.mask(10, []).size == 42 and not rse.mask(10, []).any() and rse.mask(10, []).dtype == np.uint8
    m = rse.mask(500, [(0, 2), (100, 103), (590, 10 ** 6), (7, 7)])
    assert m.size == rs.coded_bytes(500) == 596 and list(np.flatnonzero(m)) == [0, 1, 100, 101, 102] + list(range(590, 596))


# ---- the inner code's side of a lost span -------------------------------------------------------------------------------------------
def _sent_before(t, rate):
    """S(t) of include/svsfec.h, step by step"""
    out0, out1 = fec.PATTERNS.get(rate, ((1,), (rate - 1,)))
    return sum(out0[i % len(out0)] + out1[i % len(out0)] for i in range(t))


@pytest.mark.parametrize("rate", fec.RATES + fec.PUNCTURED)
def test_steps_of_sent_bits_against_brute_force(rate):
    limit = 60
    s = [_sent_before(t, rate) for t in range(limit + 2)]
    assert all(s[t] == (fec.sent_before(t, rate) if rate in fec.PUNCTURED else rate * t) for t in range(limit + 2))
    for lo in range(0, 40):
        for hi in range(lo + 1, 48):
            touched = [t for t in range(limit) if s[t] < hi and s[t + 1] > lo]
            assert fec.steps_of_sent_bits(lo, hi, rate) == (touched[0], touched[-1] + 1) == el.steps_of_sent_bits(lo, hi, rate), (lo, hi)
    if rate in fec.RATES:
        assert fec.steps_of_sent_bits(7, 20, rate) == (7 // rate, -(-20 // rate))
    big = 10 ** 12 + 7
    t0, t1 = fec.steps_of_sent_bits(big, big + 1, rate)
    assert t1 == t0 + 1 and (fec.sent_before(t0, rate) if rate in fec.PUNCTURED else rate * t0) <= big
    for bad in ((3, 3), (4, 3), (-1, 2)):
        with pytest.raises(ValueError):
            fec.steps_of_sent_bits(*bad, rate)
    with pytest.raises(ValueError):
        fec.steps_of_sent_bits(0, 1, 4)


def test_a_lost_span_in_bytes():
    k = 1561
    total = rs.coded_bytes(k)
    assert total == 1785
    assert batch.lost_span(0, 2400, 2, k, 0) == (0, 150) and batch.lost_span(0, 2400, 2, k, 1) == (0, 151)
    assert batch.lost_span(12000, 14400, 2, k) == (749, 901) == el.erased_span(5, 12, 28800, 2, k)
    assert batch.lost_span(26400, 28572, 2, k) == (1649, total)                   # the six tail steps fall away
    assert batch.lost_span(26400, 28572, 2, k, 0) == (1650, total) == el.erased_span(11, 12, 28800, 2, k, 0)
    assert batch.lost_span(8, 9, 3, k, 0) == (0, 1) and batch.lost_span(23, 25, 3, k, 0) == (0, 2)


def test_lost_frames_are_refused_before_the_device():
    frames = np.zeros((3, 96, 160), np.uint8)                 # capacity 7 200 at n = 10
    n_info = 8 * 385
    with pytest.raises(ValueError, match="outer"):
        batch.extract_coded_frames(frames, 20, 10, n_info, rate=2, lost_frames=[1])
    for copies in (2, None):
        with pytest.raises(ValueError, match="copies"):
            batch.extract_coded_frames(frames, 20, 10, 8 * 100, rate=2, copies=copies, outer=True, lost_frames=[1])
    for bad in ([3], [-1], [0, 7], [1.0], ["1"], [True], [None]):
        with pytest.raises(ValueError, match="lost_frames"):
            batch.extract_coded_frames(frames, 20, 10, n_info, rate=2, outer=True, lost_frames=bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="erase_margin"):
            batch.extract_coded_frames(frames, 20, 10, n_info, rate=2, outer=True, lost_frames=[1], erase_margin=bad)


# ---- the README's table -----------------------------------------------------------------------------------------------------------
def test_the_lost_frame_table(capsys):
    """twelve 96 x 160 frames at n = 10, delta = 20, rate 1/2, full capacity (k = 1 561, C = 7); one frame replaced by noise.
    Today's chain loses codewords; with the frame's soft bytes zeroed and its span erased every codeword decodes and the
    payload is exact.  Printed, not asserted: the wrong bytes the Viterbi decoder leaves outside the erased span - what the
    default erase_margin of one byte has to cover is a choice, not a measurement."""
    cells = {(seed, frame): el.lost_frame(seed, frame) for seed in el.LOST_SEEDS for frame in el.LOST_FRAMES}
    with capsys.disabled():
        print("\n| seed, lost frame | erased bytes | wrong stream bytes after Viterbi: noise / zeroed soft bytes | of the latter outside the span "
              "| status without the mask | status with it | wrong payload bytes with it |")
        print("|---|---|---|---|---|---|---|")
        for (seed, frame), c in cells.items():
            lo, hi = c["span"]
            print(f"| {seed}, {frame} | [{lo}, {hi}) | {c['plain_wrong']} / {c['wrong']} | {c['outside']} | " + ",".join(str(int(v)) for v in c["plain"][1])
                  + " | " + ",".join(str(int(v)) for v in c["erased"][1]) + f" | {int((c['erased'][0][:c['k']] != c['data']).sum())} |")
    for (seed, frame), c in cells.items():
        assert c["k"] == 1561 and c["erased"][1].size == 7
        assert (c["plain"][1] == 255).any(), (seed, frame)
        assert (c["erased"][1] <= 32).all(), (seed, frame, c["erased"][1])
        assert np.array_equal(c["erased"][0][: c["k"]], c["data"]), (seed, frame)
