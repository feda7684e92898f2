"""The fused soft vote without a GPU (include/svsdct.h, svs_soft_vote*): the declarations, the refusals of the two entry points
through the real library (none reaches the device), the NumPy model of the tally (svsdct/soft.py: tally, tally_bits, tile)
against soft.combine, the host build of the vote's integer side (tests/hostemu) against Python integers, a whole call's tally
through the host walker against the model's, and the README's +-8 row decoded through the tally."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soft_lib as sl
import soft_vote_lib as vl
from svsdct import native
from svsdct import soft as sv
from testlib import REPO, hostemu

SYMBOLS = ("svs_soft_vote_dev", "svs_soft_vote")


# ---- declarations ----------------------------------------------------------------------------------------------------------
def test_both_calls_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    lib = native.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.SIGNATURES
        assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
    assert len(native.SIGNATURES["svs_soft_vote_dev"][1]) == len(native.SIGNATURES["svs_soft_vote"][1]) + 1      # the stream
    assert re.search(r"#define\s+SVS_ABI_VERSION\s+4\b", header)
    assert lib.svs_abi_version() == native.ABI_VERSION == 4


def test_the_words_no_repeat_option_are_gone_where_they_are_no_longer_true():
    pkg = os.path.dirname(sv.__file__)
    for path in (os.path.join(REPO, "include", "svsdct.h"), os.path.join(REPO, "README.md"), os.path.join(pkg, "soft.py")):
        assert "there is no repeat option" not in open(path).read().lower(), path


# ---- refusals through the real library: none reaches the device ------------------------------------------------------------
FAKE_IN, FAKE_TALLY = 0x10000, 0x20000       # never dereferenced: every case returns before any device work
SENTINEL = -0x5A5A5A5B
HUGE = (4096, 2048, 2048, 0, 2048, 2048 * 2048)      # 2^28 blocks: at n = 63 a capacity of 63 * 2^28 > 1 * 2^22


def _call(lib, dev, planes=(1, 16, 16, 0, 16, 256), gray=FAKE_IN, tally="own", order=None, dither=None, delta=8.0, n_ac=10,
          period=40, stream_bit0=0, flags=0):
    """-> (rc, message, *n_bits_out, the host tally after the call or None).  tally: "own" - the device form gets a fake
    device pointer, the host form a real array of `period` sentinels; None; or an address."""
    pl = native.Planes(*planes)
    o = native.BlockOrder(*order) if order else None
    d = native.Dither(*dither) if dither else None
    host = None
    if tally == "own":
        if dev:
            tally = FAKE_TALLY
        else:
            host = np.full(max(1, min(int(period), 4096)), SENTINEL, np.int32)
            tally = host.ctypes.data
    got = C.c_uint64(0xDEAD)
    ref = lambda s: C.byref(s) if s is not None else None    # noqa: E731
    args = [gray, C.byref(pl), ref(o), None, ref(d), float(delta), int(n_ac), int(period), int(stream_bit0), tally, flags, C.byref(got)]
    rc = getattr(lib, SYMBOLS[0] if dev else SYMBOLS[1])(*args, *([None] if dev else []))
    return rc, "" if rc == 0 else lib.svs_last_error().decode(), int(got.value), host


REFUSALS = [
    ("period 0", dict(period=0), "period"),
    ("tally NULL", dict(tally=None), "pointer is NULL"),
    ("SVS_NEAREST", dict(flags=native.SVS_NEAREST), "flags"),
    ("SVS_MINMOVE", dict(flags=native.SVS_MINMOVE), "flags"),
    ("SVS_READBACK", dict(flags=native.SVS_READBACK), "flags"),
    ("unknown flag", dict(flags=0x400), "flags"),
    ("delta 0", dict(delta=0.0), "delta"),
    ("delta -1", dict(delta=-1.0), "delta"),
    ("capacity above period * 2^22", dict(planes=HUGE, n_ac=63, period=1), "2^22"),
    ("unequal first_frame", dict(order=(1, 4, 0), dither=(2, 5, 0)), "first_frame"),
    ("order.reserved", dict(order=(1, 0, 1)), "svs_block_order.reserved"),
    ("dither.reserved", dict(dither=(1, 0, 1)), "svs_dither.reserved"),
    ("planes.reserved", dict(planes=(1, 16, 16, 1, 16, 256)), "svs_planes.reserved"),
    ("gray NULL", dict(gray=None), "pointer is NULL"),
    ("period above 2^61 - 1", dict(period=1 << 61), "period"),
]


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_any_device_work_and_leave_the_out_parameters(case, dev):
    _, kw, text = case
    rc, message, got, host = _call(native.load(), dev, **kw)
    assert rc == native.SVS_ERR_INVALID_ARG and text in message, (rc, message)
    assert got == 0xDEAD                                     # *n_bits_out: untouched
    assert host is None or (host == SENTINEL).all()          # the host form's tally: untouched


def test_an_unaligned_device_tally_is_refused():
    lib = native.load()
    for off in (1, 2, 3):
        rc, message, got, _ = _call(lib, True, tally=FAKE_TALLY + off)
        assert rc == native.SVS_ERR_INVALID_ARG and "4-byte aligned" in message and got == 0xDEAD
    assert _call(lib, True, gray=FAKE_IN + 4)[0] == native.SVS_ERR_INVALID_ARG


def test_the_bound_is_on_the_capacity_over_the_period():
    """63 * 2^28 bits take a period of at least 4032 for 2^22 copies to cover them: one less is refused.
    The accepted side of the bound cannot be called without a device, so only the refused side is pinned here."""
    cap = 4096 * 256 * 256 * 63
    least = -(-cap // (1 << 22))
    assert least == 4032
    rc, message, got, _ = _call(native.load(), True, planes=HUGE, n_ac=63, period=least - 1)
    assert rc == native.SVS_ERR_INVALID_ARG and "2^22" in message and got == 0xDEAD


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
def test_the_empty_call_is_ok(dev):
    lib = native.load()
    for kw in (dict(planes=(0, 16, 16, 0, 16, 256)), dict(n_ac=0), dict(n_ac=-3), dict(planes=(0, 16, 16, 0, 16, 256), gray=None),
               dict(n_ac=0, flags=native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED)):
        rc, message, got, host = _call(lib, dev, **kw)
        assert (rc, message, got) == (native.SVS_OK, "", 0), kw
        assert host is None or not host.any()                # the host form writes its period values: all zero
    assert _call(lib, dev, planes=(0, 16, 16, 0, 16, 256), tally=None)[:3] == (native.SVS_OK, "", 0)


def test_python_level_raises_before_the_library_is_loaded():
    from svsdct import batch
    frames = np.zeros((1, 16, 16), np.uint8)
    for period in (0, -1, 1 << 61):
        with pytest.raises(ValueError):
            batch.extract_vote_frames(frames, 8, 10, period)
        with pytest.raises(ValueError):
            batch.extract_vote_device(0, native.Planes.contiguous(1, 16, 16), 8, 10, 0, period)
    with pytest.raises(ValueError):
        batch.extract_vote_frames(frames, 8, 10, 40, coeffs=[1, 2, 3])           # len != n_ac
    with pytest.raises(ValueError):
        batch.embed_repeated_frames(frames, 8, 10, [])
    with pytest.raises(ValueError):
        batch.embed_repeated_frames(frames, 8, 10, [1, 0], copies=0)
    with pytest.raises(ValueError):
        batch.embed_repeated_frames(frames, 8, 10, [1, 0], n_bits=2)


# ---- the model's own properties ------------------------------------------------------------------------------------------
def _random_soft(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size).astype(np.uint8)


@pytest.mark.parametrize("size", (1, 2, 10, 641, 6000))
def test_the_tally_is_combine(size):
    a = _random_soft(size, size)
    for period in sorted({1, 7, size - 1, size} & set(range(1, size + 1))):
        bits, score = sv.combine(a, period)
        t = sv.tally(a, period)
        assert t.dtype == np.int32 and t.shape == (period,)
        assert (t % 2 != 0).all()                             # copy 0 has been counted everywhere: odd, never zero
        assert np.array_equal(sv.tally_bits(t), bits), period
        b0 = (a[:period] >> 7).astype(np.int64)
        assert np.array_equal((t.astype(np.int64) - (2 * b0 - 1)) // 2, score) and not ((t - (2 * b0 - 1)) % 2).any(), period
    assert sv.tally_bits(sv.tally(a, 1)).dtype == np.uint8


def test_a_tie_goes_to_copy_0():
    for first, second in ((0x85, 0x05), (0x05, 0x85), (0xFF, 0x7F), (0x00, 0x80)):
        a = np.array([first, second], np.uint8)
        bits, score = sv.combine(a, 1)
        assert score[0] == 0 and bits[0] == first >> 7
        t = sv.tally(a, 1)
        assert t.tolist() == [2 * (first >> 7) - 1] and sv.tally_bits(t).tolist() == [first >> 7]


def test_tallies_of_the_pieces_of_a_stream_add_up():
    a = _random_soft(1000, 3)
    for period in (1, 7, 64, 999, 1000, 1500):
        for s in (0, 5, period - 1, period, 3 * period + 2, (1 << 32) + 3):
            whole = sv.tally(a, period, s)
            for cut in (0, 1, 333, 1000):
                parts = sv.tally(a[:cut], period, s) + sv.tally(a[cut:], period, s + cut)
                assert np.array_equal(whole, parts), (period, s, cut)


def test_a_period_beyond_the_bytes_at_a_far_offset_lands_on_the_right_residues():
    a = _random_soft(10, 9)
    period, s = 1000, (1 << 32) + 3
    t = sv.tally(a, period, s)
    first = s % period
    assert first == 299
    want = np.zeros(period, np.int64)
    for i, byte in enumerate(a):
        want[(s + i) % period] += 2 * (2 * (int(byte) >> 7) - 1) * (2 * (int(byte) & 127) + 1)       # no bit of copy 0: p >= period
    assert np.array_equal(t, want) and np.flatnonzero(t).tolist() == list(range(first, first + 10))
    # at offset 0 every byte lies in copy 0 and the entries are the single votes, odd
    t0 = sv.tally(a, period)
    assert np.flatnonzero(t0).tolist() == list(range(10)) and (t0[:10] % 2 != 0).all() and not t0[10:].any()


def test_tile_cuts_the_last_copy():
    assert sv.tile([1, 0, 0], 8).tolist() == [1, 0, 0, 1, 0, 0, 1, 0]
    assert sv.tile([1, 0, 0], 2).tolist() == [1, 0] and sv.tile([1], 0).size == 0
    assert sv.tile(np.array([1, 1, 0], np.uint8), 3).dtype == np.uint8
    with pytest.raises(ValueError):
        sv.tile([], 4)
    with pytest.raises(ValueError):
        sv.tally(np.zeros(4, np.uint8), 0)


# ---- the integer side of the kernel's vote tail on the host (tests/hostemu) -----------------------------------------------
def test_a_vote_call_plans_the_soft_side_with_the_vote_on():
    for delta in (8, 20, 12.5, 0.1):
        for n in (1, 10, 63):
            plan, args = vl.host_vote_args(delta, n, 2400, 7205)
            assert plan == dict(path=sl.PATH_EXACT, rows=8, soft=1, vote=1)
            assert args == dict(vote=1, period=2400, base=5, head=0)
    assert vl.host_vote_args(20, 10, 2400, 2390)[1] == dict(vote=1, period=2400, base=2390, head=10)
    # a soft call that is no vote: the fields at the end of SoftArgs are off
    assert sl.host_plan(20, 10)["soft"] == 1


def test_the_residue_without_a_division_is_the_residue():
    """vote_residue: (base + i) mod period through one double-precision multiply and one correction, for every kind of period -
    small, around the 2^38 below which the quotient is taken, and up to the largest accepted - at the i a call can reach
    (below 63 * 2^31) and the stream offsets of the issue"""
    top = int(hostemu().emu_vote_period_max())
    assert top == (1 << 61) - 1
    rng = np.random.default_rng(11)
    edge_i = [0, 1, 62, 63, 64, 4031, 4032, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, 63 * ((1 << 31) - 1) - 1, (1 << 38) - 1]
    periods = [1, 2, 3, 7, 63, 64, 65, 640, 2400, 6000, 100_000, 10**6, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1,
               (1 << 38) - 1, 1 << 38, (1 << 38) + 1, (1 << 53) + 1, top]
    periods += [int(p) for p in rng.integers(1, 1 << 38, 40)] + [3 ** k for k in range(1, 24)]
    for period in periods:
        i = edge_i + [int(v) for v in rng.integers(0, 1 << 38, 200)]
        i += [k * period + d for k in (1, 2, 1000, (1 << 37) // period) for d in (-1, 0, 1) if 0 <= k * period + d < 1 << 38]
        for s in (0, 5, period - 1, period, (1 << 32) + 3, top, (1 << 64) - 1):
            res, head = vl.host_residues(period, s, i)
            assert res == [(s + v) % period for v in i], (period, s)
            assert head == [s + v < period for v in i], (period, s)


def test_the_vote_of_a_byte():
    emu = hostemu()
    for byte in range(256):
        b, m = byte >> 7, byte & 127
        assert emu.emu_vote_of(byte, 0) == 2 * (2 * b - 1) * (2 * m + 1)
        assert emu.emu_vote_of(byte, 1) == 2 * (2 * b - 1) * (2 * m + 1) + (2 * b - 1)
    assert abs(emu.emu_vote_of(0xFF, 1)) == 511                      # the most one copy contributes


@pytest.mark.parametrize("form", ("prefix", "dither+zigzag+order"))
@pytest.mark.parametrize("shape", ((2, 16, 24), (5, 64, 120)))
def test_the_walkers_tally_is_the_models(shape, form):
    """a whole vote call through the product headers on the host - extract_block_soft with the launch's tables, vote_residue and
    vote_of per byte - against soft.tally of the NumPy model's bytes, exactly: every landmark period of the shape, stream offsets
    at both ends of copy 0 and far behind it, without and with an order, a selection and a dither"""
    import dither_lib as dl
    delta, n, key, order_key, first_frame = 20, 10, 0x5EED0FD17E12, 0xB10C0DE, 3
    frames = dl.noise(shape, 0, 256, seed=9)
    cap = shape[0] * (shape[1] // 8) * (shape[2] // 8) * n
    keyed = form != "prefix"
    kw = dict(index=sl.zigzag(n), key=key, order_key=order_key, first_frame=first_frame) if keyed else {}
    call = dict(index=sl.zigzag(n), dither_key=key, block_key=order_key, first_frame=first_frame) if keyed else {}
    soft = sl.model_batch_soft(frames, delta, n, **kw)
    assert soft.size == cap
    for period in vl.landmark_periods(*shape, n):
        for s0 in (0, 1, cap - 1, 10**12 + 7):
            got = vl.host_tally(frames, delta, n, period, s0, **call)
            assert np.array_equal(got, sv.tally(soft, period, s0)), (shape, form, period, s0)


# ---- robustness: the README's +-8 row through the tally ------------------------------------------------------------------
def test_three_disturbed_copies_decode_through_the_tally_as_through_combine():
    """delta = 20, n_ac = 10, three 96 x 160 frames, pixel noise of +-8, the seeds of tests/test_soft_extract_cpu.py
    (soft_lib.vote_experiment, seed 4): the same steps with the streams kept, decoded once by combine and once by the tally"""
    from oracle.qim_dct_oracle import frame_embed
    delta, n_ac, amp, seed = 20, 10, 8, 4
    rng = np.random.default_rng(seed)
    h, w = sl.VOTE_SHAPE
    cap = (h // 8) * (w // 8) * n_ac
    pay = rng.integers(0, 2, cap).astype(np.uint8)
    streams = []
    for _ in range(3):
        cover = rng.integers(64, 192, (h, w)).astype(np.uint8)
        _, stego, used = frame_embed(cover, delta, pay, n_ac)
        assert used == cap
        noisy = np.clip(stego.astype(np.int64) + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)
        streams.append(sl.model_soft(noisy, delta, n_ac))
    soft = np.concatenate(streams)
    bits, _ = sv.combine(soft, cap)
    voted = sv.tally_bits(sv.tally(soft, cap))
    assert np.array_equal(voted, bits)
    errors = int((bits != pay).sum())
    print(f"payload bit errors of the soft vote over three copies at +-{amp}: combine {errors}, tally {int((voted != pay).sum())}")
    assert int((voted != pay).sum()) == errors == sl.vote_experiment(delta, n_ac, amp, seed)["soft"]
    # frame by frame, as a receiver that reads the clip in batches adds its tallies
    parts = sum(sv.tally(s, cap, k * cap).astype(np.int64) for k, s in enumerate(streams))
    assert np.array_equal(parts, sv.tally(soft, cap))
