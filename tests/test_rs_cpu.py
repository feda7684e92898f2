"""CPU tier of the Reed-Solomon outer code (include/svsrs.h, libsvsrs.so, svsdct/rs.py): the library's exports, the format's known
answers, the sizes, the host encoder against the NumPy model of tests/rs_lib.py, the model's decoder against the format's
definition, the refusals in the documented order, the host build of csrc/svs_rs.hpp against the model on the GPU test's inputs
(and once as a stand-alone program under the address and undefined-behaviour sanitizers), and the channel experiment of the
README's table.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import channel_lib as cl
import rs_lib as rl
from testlib import check_header_is_plain_c, check_library_exports, run_sanitized_emu
from svsdct import batch, fec, native, rs

I, CAP = native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY
G_HEX = "01 74 40 34 ae 36 7e 10 c2 a2 21 21 9d b0 c5 e1 0c 3b 37 fd e4 94 2f b3 b9 18 8a fd 14 8e 37 ac 58"
PARITY_0_TO_9 = "6c 22 8c 86 1c 3e 14 d2 52 a2 ca 9c 2f a1 28 9a 54 02 15 8d b4 09 81 5c 43 eb 09 72 0b ef 59 fb"


def _hex(a):
    return " ".join(f"{int(v):02x}" for v in a)


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_the_header():
    # both Reed-Solomon libraries hold the kernel and the tables of csrc/svs_rs_decode.hpp and are loaded into one process: a
    # dynamic symbol of either would be interposed by the other's
    check_library_exports("svsrs.h", rs, "svs_rs", 7, hidden=("decode_kernel", "d_field", "d_lfsr"))
    assert rs.ABI_VERSION == 1


def test_the_header_is_plain_c(tmp_path):
    check_header_is_plain_c(tmp_path, ("svsdct.h", "svsfec.h", "svsrs.h"),
                            "SVS_RS_PARITY == 32 && SVS_RS_UNCORRECTABLE == 255 && SVS_ERR_CAPACITY == -4")


# ---- the format's known answers ---------------------------------------------------------------------------------------------------
def test_the_field_and_the_generator():
    assert rl.EXP[8] == 0x1D and rl.EXP[1] == 2 and len(set(rl.EXP[:255])) == 255            # alpha = 2 generates the field mod 0x11D
    assert _hex(rl.G) == G_HEX
    for j in range(32):                                                                      # alpha^0 .. alpha^31 are its roots
        assert not rl.syndromes(np.array([rl.G], np.uint8))[0, j]
    assert rl.syndromes(np.array([[1, 0]], np.uint8))[0, 5] == rl.EXP[5]


def test_the_known_answers():
    for encode in (rs.encode, lambda d: rl.encode(np.frombuffer(d, np.uint8)).tobytes()):
        assert _hex(encode(b"\x01")[1:]) == G_HEX[3:]                                        # one data byte 01: the parity is g(x)
        assert _hex(encode(bytes(range(10)))[10:]) == PARITY_0_TO_9
        stream = encode(bytes(range(224)))
        assert len(stream) == 288 and stream[:224] == bytes(range(224)) and _hex(stream[224:232]) == "99 cc f0 92 3b 6e eb 31"


def test_sizes(tmp_path):
    lib, emu = rs.load(), rl.emu(tmp_path)
    examples = {32: 0, 33: 1, 255: 223, 256: 223, 287: 223, 288: 224, 449: 385, 786: 669, 0: 0}
    for total, k in examples.items():
        assert lib.svs_rs_data_bytes(total) == rs.data_bytes(total) == rl.data_bytes(total) == emu.rs_emu_data_bytes(total) == k
    for total in list(range(0, 1200)) + [10 ** 6, 10 ** 9 + 7]:
        k = rs.data_bytes(total)
        assert k == lib.svs_rs_data_bytes(total) == rl.data_bytes(total)
        assert k == 0 or rs.coded_bytes(k) <= total
        assert rs.coded_bytes(k + 1) > total
    for k in (1, 222, 223, 224, 446, 447, 10 ** 9, 1 << 37):
        assert lib.svs_rs_codewords(k) == rs.codewords(k) == rl.codewords(k) == -(-k // 223)
        assert lib.svs_rs_coded_bytes(k) == rs.coded_bytes(k) == rl.coded_bytes(k) == emu.rs_emu_coded_bytes(k) == k + 32 * rs.codewords(k)
    assert lib.svs_rs_coded_bytes(0) == 0 == lib.svs_rs_coded_bytes((1 << 37) + 1) == lib.svs_rs_codewords((1 << 37) + 1)
    assert lib.svs_rs_data_bytes(2 ** 64 - 1) == 1 << 37
    assert rs.payload_bits(7200, 3) == 8 * 235 and rs.payload_bits(7200, 78) == 8 * 669
    assert rs.payload_bits(7200, 2) == 8 * 385 and rs.payload_bits(7200, 34) == 8 * 578
    for bad in (-1, (1 << 37) + 1):
        with pytest.raises(ValueError):
            rs.coded_bytes(bad)


def test_the_encoder_is_the_models(tmp_path):
    rng = np.random.default_rng(3)
    for k in (1, 2, 222, 223, 224, 225, 446, 447, 700, 5000):
        data = rng.integers(0, 256, k).astype(np.uint8)
        want = rl.encode(data)
        assert rs.encode(data.tobytes()) == want.tobytes(), k
        out = np.full(want.size + 8, 0xEE, np.uint8)                 # the raw call: exactly k + 32 C bytes, the input untouched
        keep, got = data.copy(), C.c_uint64(7)
        assert rs.load().svs_rs_encode(data.ctypes.data, k, out.ctypes.data, want.size, C.byref(got)) == 0
        assert got.value == want.size and np.array_equal(out[: want.size], want) and (out[want.size:] == 0xEE).all()
        assert np.array_equal(data, keep)
        assert rs.load().svs_rs_encode(data.ctypes.data, k, out.ctypes.data, want.size, None) == 0          # n_out may be NULL
        emu_out = np.empty(want.size, np.uint8)
        rl.emu(tmp_path).rs_emu_encode(data.ctypes.data, k, emu_out.ctypes.data)
        assert np.array_equal(emu_out, want)
        assert not rl.syndromes(rl.codeword_matrix(want, k)).any()                                            # g(x) divides every codeword
    assert rs.encode(b"") == b""
    with pytest.raises(TypeError):
        rs.encode(np.zeros(4, np.int32))


def test_a_burst_of_c_bytes_puts_one_byte_into_a_codeword():
    k = 1000
    index, valid = rl.gather(k)
    owner = np.empty(rl.coded_bytes(k), np.int64)
    owner[index[valid]] = np.broadcast_to(np.arange(index.shape[0])[:, None], index.shape)[valid]
    n_cw = rl.codewords(k)
    for start in range(owner.size - n_cw + 1):
        assert len(set(owner[start: start + n_cw])) == n_cw


# ---- the model against the definition, and the host build against the model ---------------------------------------------------------
def test_the_model_meets_the_definition():
    """every case of the GPU test: what the model calls decoded is a code word that differs from the received one in exactly
    `status` bytes, at most 16; what it calls uncorrectable is as received.  And up to 16 errors always come back as sent."""
    for kind in rl.KINDS:
        for k in rl.KS:
            received, decoded, status, counts = rl.case(kind, k)
            rl.check_definition(received, decoded, status, k)
            good = status != rl.UNCORRECTABLE
            assert counts == (int(status[good].sum()), int((~good).sum()))
            if kind in ("clean", "zero"):
                assert not status.any() and np.array_equal(decoded, received)
            if kind in ("one", "sixteen"):
                assert (status == {"one": 1, "sixteen": 16}[kind]).all()
            if kind == "seventeen":
                assert (status == rl.UNCORRECTABLE).any(), "this seed must show a codeword that does not decode"
            if kind == "ends":
                assert (status[[0, -1]] == 3).all() and not status[1:-1].any()
            if kind == "burst":
                assert status.sum() == min(rl.codewords(k), 40) and status.max() == 1
    rng = np.random.default_rng(8)
    for k in (1, 225, 700):
        for errors in range(0, 17):
            sent = rl.encode(rng.integers(0, 256, k).astype(np.uint8))
            received = sent.copy()
            for c in range(rl.codewords(k)):
                rl._hit(received, rng, k, c, rng.choice(int(rl.lengths(k)[c]) + 32, errors, replace=False))
            decoded, status, _ = rl.decode(received, k)
            assert np.array_equal(decoded, sent) and (status == errors).all(), (k, errors)


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rs_emu")


@pytest.mark.parametrize("kind", rl.KINDS)
def test_the_host_build_is_the_model_on_the_gpu_tests_inputs(kind, emu_dir):
    for k in rl.KS:
        received, want, status, counts = rl.case(kind, k)
        got, got_status, got_counts = rl.emu_decode(received, k, (11, 5), emu_dir)
        assert np.array_equal(got, want) and np.array_equal(got_status, status), (kind, k)
        assert got_counts == (11 + counts[0], 5 + counts[1]), (kind, k)


def test_the_sanitized_stand_alone_program(tmp_path):
    """the host build's LFSR, syndromes, Berlekamp-Massey, root search and Forney, driven by rs_emu.cpp's own main, under the
    address and undefined-behaviour sanitizers: a stand-alone program, run once; nothing is loaded into python"""
    run_sanitized_emu("rs_emu.cpp", "RS_EMU_MAIN", tmp_path, "rs emu ok")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order():
    """each call breaks the rule under test and every later one: the earlier refusal must be the one reported.  No call here
    reaches a launch: an out-of-range argument is refused on the host before any device work."""
    lib = rs.load()
    err = lambda: lib.svs_rs_last_error().decode()   # noqa: E731
    buf = np.zeros(64, np.uint8)
    p, big = buf.ctypes.data, (1 << 37) + 1
    assert p % 4 == 0
    dec = lib.svs_rs_decode_dev
    assert dec(None, 0, None, 0, p + 1, None) == 0                                                     # 1. k = 0: no pointer looked at
    assert dec(None, big, None, 0, p + 1, None) == I and "SVS_RS_MAX_DATA_BYTES" in err() and "svs_rs_decode_dev" in err()   # 2. the length
    assert dec(None, 2 ** 64 - 1, None, 0, p + 1, None) == I and "SVS_RS_MAX_DATA_BYTES" in err()
    assert dec(None, 500, p, 0, p + 1, None) == I and "NULL" in err()                                  # 3. NULL pointers
    assert dec(p + 1, 500, None, 0, p + 1, None) == I and "NULL" in err()
    for off in (1, 2, 3):
        assert dec(p + 1, 500, p, 0, p + off, None) == I and "aligned" in err()                        # 4. before the capacity
    assert dec(p + 1, 500, p, 2, p + 4, None) == CAP and "3" in err()                                  # 5. ceil(500 / 223) = 3
    assert dec(p + 1, 500, p, 2, None, None) == CAP
    enc = lib.svs_rs_encode
    got = C.c_uint64(9)
    assert enc(None, 0, None, 0, C.byref(got)) == 0 and got.value == 0
    assert enc(None, big, None, 0, None) == I and "SVS_RS_MAX_DATA_BYTES" in err()
    assert enc(None, 10, p, 0, None) == I and "NULL" in err()
    assert enc(p, 10, None, 0, None) == I and "NULL" in err()
    assert enc(p, 10, p + 16, 41, None) == CAP and "42" in err()
    # the Python layer raises before the library is asked
    for call in (lambda: rs.decode(b"\x00" * 40, 10), lambda: rs.decode(np.zeros(42, np.int32), 10), lambda: rs.coded_bytes(-1),
                 lambda: rs.decode_device(1, (1 << 37) + 1, 1, 1), lambda: rs.data_bytes(-1)):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_the_coded_frame_calls_with_an_outer_code_refuse_before_the_device():
    frames = np.zeros((3, 96, 160), np.uint8)                 # capacity 7 200 at n = 10
    with pytest.raises(ValueError, match="whole bytes"):
        batch.embed_coded_frames(frames, 20, 10, np.zeros(15, np.uint8), rate=2, outer=True)
    with pytest.raises(ValueError, match="whole bytes"):
        batch.extract_coded_frames(frames, 20, 10, 15, rate=2, outer=True)
    with pytest.raises(ValueError, match=f"capacity.*{8 * 385} payload bits"):
        batch.embed_coded_frames(frames, 20, 10, np.zeros(8 * 386, np.uint8), rate=2, outer=True)
    with pytest.raises(ValueError, match=f"capacity.*{8 * 385} payload bits"):
        batch.extract_coded_frames(frames, 20, 10, 8 * 386, rate=2, outer=True)
    with pytest.raises(ValueError, match="margin|matrix"):
        batch.extract_coded_frames(frames, 20, 10, 8, matrix=2, outer=True)
    with pytest.raises(ValueError):
        batch.extract_coded_frames(frames, 20, 10, 0, outer=True)
    # what the sender embeds with outer=True is the inner code over the bits of the RS stream
    data = np.random.default_rng(2).integers(0, 256, 385).astype(np.uint8)
    assert fec.coded_bits(8 * rs.coded_bytes(385), 2) <= 7200 < fec.coded_bits(8 * rs.coded_bytes(386), 2)
    assert np.array_equal(np.unpackbits(rs.encode_array(data)), np.unpackbits(rl.encode(data)))


# ---- the README's table -----------------------------------------------------------------------------------------------------------
ROWS = ((3, 60), (78, 80), (56, 77), (34, 73), (2, 67))
SEEDS = (cl.SURVIVAL_SEED, 11, 12, 13)


def test_the_channel_table(capsys):
    """delta = 20, n = 10, reference rule, three 96 x 160 frames of noise in [64, 192) at full capacity, four cover seeds: what
    the Viterbi decoder leaves near its cliff and what the outer code makes of it"""
    assert cl.SURVIVAL_SEED == 5
    cells = {(rate, q, seed): rl.outer_survival(rate, q, seed) for rate, q in ROWS for seed in SEEDS}
    with capsys.disabled():
        print("\n| inner rate, Q | data bytes, codewords | wrong payload bits after Viterbi, per seed | wrong stream bytes after Viterbi, per seed "
              "| status bytes, per seed | wrong payload bits after the outer code, per seed |")
        print("|---|---|---|---|---|---|")
        for rate, q in ROWS:
            r = [cells[rate, q, seed] for seed in SEEDS]
            print(f"| {rl.NAMES[rate]}, Q = {q} | {r[0]['k']}, {r[0]['C']} | " + " / ".join(str(c["viterbi_bits"]) for c in r) + " | "
                  + " / ".join(str(int((c["received"] != rl.encode(c["data"])).sum())) for c in r) + " | "
                  + " / ".join(",".join(str(int(v)) for v in c["status"]) for c in r) + " | "
                  + " / ".join(str(c["wrong_bits"]) for c in r) + " |")
    assert [cells[rate, q, 5]["k"] for rate, q in ROWS] == [235, 669, rs.data_bytes(fec.info_bits(7200, 56) // 8), 578, 385]
    assert [cells[rate, q, 5]["C"] for rate, q in ROWS] == [2, 3, 3, 3, 2]
    for rate, q in ((3, 60), (78, 80)):
        c = cells[rate, q, 5]
        assert c["viterbi_bits"] > 0 and c["wrong_bits"] == 0
        assert ((c["status"] >= 1) & (c["status"] <= 16)).all()
    c = cells[2, 67, 5]
    assert (c["status"] == 255).all() and np.array_equal(c["decoded"], c["received"])
    c = cells[34, 73, 12]
    assert (c["status"] == 255).any() and ((c["status"] >= 1) & (c["status"] <= 16)).any()
