"""CPU tier of the soft, vote and histogram calls under per-coefficient steps (include/svsdct.h, svs_stepped_soft_*; GPU tier:
test_stepped_soft_gpu.py): the scale identity the format rests on, the host build of the stepped soft block body against the NumPy
model of the byte, the uniform identity on the host, the route and the launch tables, the survival table of the README from the
model, and what Python and the C ABI refuse without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channel_lib as cl
import stepped_lib as st
import stepped_soft_lib as ss
import tie_lib as tl
from svsdct import batch, native, steps

KEY = st.DITHER_KEY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("u20", "u16", "u7", "m75x2", "odd")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return ss.emu(tmp_path_factory.mktemp("stepped_soft_emu"))


def frames_of(kind, shape=(2, 32, 48)):
    return cl.content(kind, shape)


# ---- 1. the scale --------------------------------------------------------------------------------------------------------------
def test_the_scale_is_the_soft_calls_scale_for_every_integer_step():
    """254.0f / dk == (float)(254.0 / (double)dk) bit for bit, dk = 1..4095: the stepped byte's s_k is make_soft_args' scale"""
    d = np.arange(1, 4096)
    once = np.float32(254.0) / d.astype(np.float32)
    twice = (254.0 / d.astype(np.float64)).astype(np.float32)
    assert once.dtype == np.float32 and np.array_equal(once.view(np.uint32), twice.view(np.uint32))
    half = np.float32(0.5) * d.astype(np.float32)
    assert np.array_equal(half.astype(np.float64), 0.5 * d)          # h_k is exact


# ---- 2. the host build of the block body is the model --------------------------------------------------------------------------
def _options():
    """stepped_lib.OPTIONS on one frame: (name, selection, dither key); an order permutes whole blocks and leaves the body alone"""
    for name, (order_key, index, key) in st.OPTIONS.items():
        yield name, index, key, order_key


def _against_model(gray, table, n_ac, stats, t=st.FIRST_FRAME):
    n_blocks = (gray.shape[0] // 8) * (gray.shape[1] // 8)
    for name, index, key, order_key in _options():
        want = ss.model_soft(gray, table, n_ac, index, key, t, stats=stats)
        got = ss.host_soft(gray, table, n_ac, index, key, t)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if order_key is not None:       # the model under the order is the raster bytes, block by block, in the order's places
            perm = st.dl._perm(order_key, t, n_blocks)
            n = want.size // n_blocks
            assert np.array_equal(ss.model_soft(gray, table, n_ac, index, key, t, perm), got.reshape(n_blocks, n)[perm].reshape(-1)), name


def test_the_host_build_of_the_stepped_soft_body_is_the_model(emu):
    """extract_block_stepped_soft byte for byte under the uniform tables 20, 16 and 7, matched(75, 2) and the odd-step table x
    plain, order, select, dither, all, on clipping noise, mid noise, flat blocks and stepped stego; and on the tie corpus under the
    uniform tables of its integer deltas, as test_stepped_cpu.py reaches half-integer quantiser inputs.  Both kinds of edge are
    counted: inputs exactly on a half-integer, and coefficients exactly on a lattice point (m = 127)."""
    stats = {}
    for name in TABLES:
        table = st.TABLES[name]
        for kind in ("full", "mid", "flat"):
            for gray in frames_of(kind):
                _against_model(gray, table, 10, stats)
        for f, gray in enumerate(frames_of("mid")):          # stepped stego: the bytes sit near the lattice
            cap = (gray.shape[0] // 8) * (gray.shape[1] // 8) * 10
            for name_o, index, key, _ in _options():
                stego = st.model_embed(gray, table, st.dl.payload(cap - 7, seed=f), 10, "nearest", index, key, st.FIRST_FRAME)[0]
                want = ss.model_soft(stego, table, 10, index, key, st.FIRST_FRAME, stats=stats)
                got = ss.host_soft(stego, table, 10, index, key, st.FIRST_FRAME)
                assert np.array_equal(got, want), (name, name_o)
    assert stats["lattice"] > 0                            # flat blocks: every AC coefficient is exactly 0, a lattice point
    before = stats["half"]
    for d in (8, 20):                                      # the corpus's integer deltas, as uniform tables
        for n in (10, 63):
            frames, _ = tl.frames_for(n, d, 136)
            for f, gray in enumerate(frames):
                for key in (None, KEY):
                    want = ss.model_soft(gray, st.uniform(d), n, None, key, tl.FIRST_FRAME + f, stats=stats)
                    assert np.array_equal(ss.host_soft(gray, st.uniform(d), n, None, key, tl.FIRST_FRAME + f), want), (d, n, f, key)
    print("quantiser inputs exactly on a half-integer:", stats["half"], " coefficients exactly on a lattice point:", stats["lattice"])
    assert stats["half"] > before >= 0 and stats["half"] > 0 and stats["lattice"] > 0


def test_a_black_block_sits_on_the_lattice_and_a_boundary_reads_0(emu):
    """through the host build of the block body: every coefficient of a black block is exactly 0, a lattice point of every
    table, so without a dither every byte is the model's byte of x = 0 for its step - bit 0 and m = (int)(h_k * s_k), which is
    127, or 126 where the float32 product 0.5f * dk * (254.0f / dk) falls just below 127 (some odd steps; the existing soft call
    does the same at such a delta) - and under a dither it is the model's byte of -d.
    The format's two ends, stated on the model for steps where h_k * s_k is 127: 127 on a lattice point, 0 on a boundary."""
    black = np.zeros((16, 24), np.uint8)
    n_blocks = 6
    seen = set()
    for name in TABLES:
        table = st.TABLES[name]
        for index in (None, st.SELECTION):
            k = np.asarray(st.dl._index(10, index))
            dk = np.ascontiguousarray(np.broadcast_to(st._steps_f32(table)[k][None, :], (n_blocks, k.size)))
            got = ss.host_soft(black, table, 10, index, None, 0)
            assert np.array_equal(got, ss.model_bytes(np.zeros_like(dk), dk).reshape(-1)), (name, index)
            assert got.min() >= 126 and got.max() <= 127, (name, index, got)
            if name in ("u20", "u16"):
                assert (got == 0x7F).all(), (name, index)
            seen |= set(int(b) for b in got)
            d = st.dither_values(KEY, 5, n_blocks, table)[:, k]
            assert np.array_equal(ss.host_soft(black, table, 10, index, KEY, 5), ss.model_bytes(-d, dk).reshape(-1)), (name, index)
    assert seen == {126, 127}
    for dk in (1, 7, 16, 20, 62, 4095):
        d = np.float32(dk)
        x = np.array([0, dk, -3 * dk, 0.5 * dk, 1.5 * dk, -0.5 * dk], np.float32)
        got = ss.model_bytes(x, np.full(x.shape, d))
        assert [int(b) & 127 for b in got] == [127, 127, 127, 0, 0, 0], (dk, got)
        assert [int(b) >> 7 for b in got[:3]] == [0, 1, 1]


# ---- 3. the uniform identity on the host -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 16, 7))
def test_a_uniform_table_is_the_soft_body_at_that_delta(emu, d):
    """extract_block_stepped_soft under every delta[k] = D against extract_block_soft at delta = D in the quantiser mode the route
    gives it (16: QM_POW2, a multiply by 1 / 16 where the stepped body divides), with and without a dither; and the two models"""
    import soft_lib as sl
    table = st.uniform(d)
    for kind in ("full", "mid", "flat"):
        for gray in frames_of(kind):
            for index in (None, st.SELECTION):
                for key in (None, KEY):
                    got = ss.host_soft(gray, table, 10, index, key, 3)
                    assert np.array_equal(got, ss.host_uniform(gray, d, 10, index, key, 3)), (d, kind, index, key)
                    assert np.array_equal(got, sl.model_soft(gray, d, 10, index, key, 3)), (d, kind, index, key)
    for n in (10, 63):                                    # and on rounding ties
        if d in (20,):
            frames, _ = tl.frames_for(n, d, 136)
            for f, gray in enumerate(frames):
                assert np.array_equal(ss.host_soft(gray, table, n, None, None, f), ss.host_uniform(gray, d, n, None, None, f))


# ---- 4. the route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1, 2), ids=("fast", "pocketfft", "guarded"))
@pytest.mark.parametrize("n_ac", (3, 10, 63))
def test_a_stepped_soft_call_plans_the_holders_of_the_stepped_side(emu, mode, n_ac):
    """soft && stepped: EXACT, eight rows, QM_POW2 in every mode, steps.on = soft.on = 1, the soft side's table never empty (the
    selection or the prefix table of n_ac); a vote or a histogram adds only its own flag; a histogram is never keyed"""
    prefix = list(range(1, n_ac + 1))
    scattered = [int(k) for k in st.sl.ZIGZAG[5:5 + min(n_ac, 20)]]
    for extra in (0, 16, 32, 48):
        for index in (None, prefix, scattered):
            count = n_ac if index is None else len(index)
            plans = {kind: ss.host_plan(kind, n_ac, 600, mode | extra, index, st.TABLES["m75x2"], period=977, bit0=5)
                     for kind in ("soft", "vote", "hist")}
            for kind, p in plans.items():
                assert (p["path"], p["rows"], p["qm"], p["stepped"], p["soft"]) == (ss.PATH_EXACT, 8, ss.QM_POW2, 1, 1), (kind, p)
                assert p["steps_on"] == 1 and p["soft_on"] == 1, (kind, p)
                assert p["soft_table_count"] == count and p["sel_count"] == count, (kind, p)
                assert p["dith_on"] == int(bool(extra & 16)), (kind, p)
                assert p["sizeof_soft_args"] == 56
            assert (plans["soft"]["vote"], plans["soft"]["hist"], plans["soft"]["soft_vote"], plans["soft"]["soft_hist"]) == (0, 0, 0, 0)
            assert (plans["vote"]["vote"], plans["vote"]["hist"], plans["vote"]["soft_vote"], plans["vote"]["soft_hist"]) == (1, 0, 1, 0)
            assert (plans["hist"]["vote"], plans["hist"]["hist"], plans["hist"]["soft_vote"], plans["hist"]["soft_hist"]) == (0, 1, 0, 1)
            assert plans["soft"]["keyed"] == plans["vote"]["keyed"] == int(bool(extra & 32))
            assert plans["hist"]["keyed"] == 0


# ---- 5. the survival table -----------------------------------------------------------------------------------------------------
# {label: {quality: (errors of each copy, hard majority, soft vote)}}: the table of the README, three 96 x 160 frames of noise in
# [64, 192), one 2 400-bit copy per frame, matched(75, 2)
SURVIVAL = {
    "1..10; reference": {50: ([0, 0, 1], 0, 0), 40: ([353, 361, 358], 219, 71)},
    "zig-zag 1..10; reference": {50: ([0, 0, 0], 0, 0), 40: ([475, 490, 486], 352, 96)},
    "zig-zag 1..10; nearest": {50: ([0, 0, 0], 0, 0), 40: ([496, 476, 479], 359, 110)},
    "zig-zag 6..15; reference": {50: ([1, 0, 1], 0, 0), 40: ([426, 450, 385], 291, 74)},
}


def test_the_survival_table():
    table = st.matched(75, 2)
    rows = [(label, ss.survival(table, index, rule)) for label, index, rule in ss.SURVIVAL_ROWS]
    print("\n" + ss.format_survival(rows))
    for label, e in rows:
        for q in (50, 40):
            assert (e[q][0], e[q][1], e[q][2]) == SURVIVAL[label][q], (label, q, e[q])
        single, majority, soft = e[40]
        assert 3 * soft <= min(single), (label, e[40])           # at most a third of the best single copy's errors
        assert majority > 2 * soft, (label, e[40])               # the hard majority has more than twice the soft vote's
    # the model is the project's: the per-copy columns are stepped_lib.survival's, and uniform 40 on 1..10 votes down to 99 at Q = 50
    _, hard = st.survival(table, st.ROW_1_10, "reference", qualities=(50, 40))
    assert [hard[q] for q in (50, 40)] == [rows[0][1][q][0] for q in (50, 40)]
    u40 = ss.survival(st.uniform(40), st.ROW_1_10, "reference", qualities=(50,))[50]
    assert u40[0] == [141, 145, 133] and u40[2] == 99, u40


# ---- 6. what needs no device -------------------------------------------------------------------------------------------------
def test_python_refuses_a_malformed_table_before_any_call():
    frames = np.zeros((1, 8, 8), np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    bad = np.zeros(64, np.uint16)
    for call in (lambda t: batch.extract_soft_frames(frames, 20, 3, steps=t),
                 lambda t: batch.extract_vote_frames(frames, 20, 3, 5, steps=t),
                 lambda t: batch.extract_histogram_frames(frames, 20, 3, steps=t),
                 lambda t: batch.extract_soft_device(64, planes, 20, 3, 128, 64, steps=t),
                 lambda t: batch.extract_vote_device(64, planes, 20, 3, 128, 5, steps=t),
                 lambda t: batch.extract_histogram_device(64, planes, 20, 3, 128, steps=t)):
        with pytest.raises(ValueError, match=r"delta\[1\]"):
            call(bad)
        with pytest.raises(ValueError):
            call(np.ones(63, np.uint16))
        with pytest.raises(ValueError):
            call(np.full(64, 4096, np.uint32))


INVALID = native.SVS_ERR_INVALID_ARG


def _call(name, dev, table=None, flags=0, dither=None, coeffs=None, period=7):
    """svs_stepped_soft_<name>[_dev] on 2 x 16 x 24 planes with pointers no refusal looks through -> (rc, message, n_bits_out)"""
    ref = lambda s: C.byref(s) if s is not None else None   # noqa: E731
    lib = native.load()
    done = C.c_uint64(12345)
    planes = native.Planes.contiguous(2, 16, 24)
    middle = {"extract": [128, 1 << 20], "vote": [period, 0, 128], "histogram": [128]}[name]
    order = [] if name == "histogram" else [None]
    rc = getattr(lib, f"svs_stepped_soft_{name}" + ("_dev" if dev else ""))(
        64, C.byref(planes), *order, ref(coeffs), ref(dither), ref(table), 10, *middle, flags, C.byref(done), *([None] if dev else []))
    return rc, lib.svs_last_error().decode(), int(done.value)


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
@pytest.mark.parametrize("name", ("extract", "vote", "histogram"))
def test_the_table_is_checked_first_and_the_flags_before_any_pointer(name, dev):
    table = steps.steps_struct(st.uniform(20))
    rc, msg, done = _call(name, dev)
    assert rc == INVALID and "steps is NULL" in msg and done == 12345
    for k, v in ((1, 0), (63, 4096)):
        bad = steps.steps_struct(st.uniform(20))
        bad.delta[k] = v
        rc, msg, done = _call(name, dev, bad, flags=1 << 30, dither=native.Dither(5, 0, 1))
        assert rc == INVALID and f"delta[{k}] = {v}" in msg and done == 12345, msg
    rc, msg, done = _call(name, dev, table, dither=native.Dither(5, 0, 1), flags=1 << 30)
    assert rc == INVALID and "svs_dither.reserved" in msg and done == 12345
    header = open(os.path.join(ROOT, "include", "svsdct.h")).read()
    for flag in ("SVS_NEAREST", "SVS_MINMOVE", "SVS_READBACK"):
        m = re.search(r"#define\s+" + flag + r"\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\s*(?:<<\s*(\d+))?", header)
        value = int(m.group(1), 0) << int(m.group(2) or 0)
        rc, msg, done = _call(name, dev, table, flags=value)
        assert rc == INVALID and "takes the mode bits only" in msg and done == 12345, (flag, msg)
    rc, msg, done = _call(name, dev, table, flags=1 << 30)
    assert rc == INVALID and "takes the mode bits only" in msg and done == 12345


def test_the_documents_no_longer_say_the_form_is_missing():
    header = open(os.path.join(ROOT, "include", "svsdct.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    example = open(os.path.join(ROOT, "examples", "recompression_survival.py")).read()
    assert "no read-back, soft, vote, histogram" not in header
    assert "stepped soft / vote / histogram calls" not in readme
    assert "no soft, vote or histogram form" not in example
    for name in ("svs_stepped_soft_extract", "svs_stepped_soft_vote", "svs_stepped_soft_histogram"):
        assert name + "_dev(" in header and name + "(" in header
        assert name in readme
