"""Soft-decision extraction without a GPU (include/svsdct.h, svs_soft_extract*): the NumPy model of the format against the host
build of the new block body, the identity of its hard bits with the hard extraction, the routing of a soft call, the refusals of
the two entry points through the real library, what the reliability means on stego, on a cover and under a foreign dither, the
three-copy vote the README quotes, and svsdct/soft.py."""
import ctypes as C

import numpy as np
import pytest

import dither_lib as dl
import soft_lib as sl
import tie_lib as tl
from svsdct import native
from svsdct import soft as sv

DELTAS = (8, 20, 12.5, 0.1)
KEY = 0x5EED0FD17E12
ORDER_KEY = 0xB10C0DE


def _flat_frames():
    """two frames of constant blocks: every AC coefficient is 0 (or float32 dust of the transform), levels 0 and 255 included"""
    levels = np.array([0, 1, 2, 7, 64, 127, 128, 129, 200, 254, 255, 33], np.uint8)
    blocks = np.repeat(levels, 64).reshape(1, 12, 8, 8)
    return np.concatenate([tl.from_blocks(blocks, 16, 48), tl.from_blocks(blocks[:, ::-1], 16, 48)])


def _inputs():
    """(name, frames, deltas, dither key, first frame): noise over the whole byte range, flat blocks, and the tie corpus at the
    delta each of its frame sets was made for (its dither ties are ties under its own key and first frame)"""
    out = [("noise", dl.noise((2, 32, 48), 0, 256, seed=5), DELTAS, KEY, 3), ("flat", _flat_frames(), DELTAS, KEY, 0)]
    for family, n, delta in tl.one_setting_per_family_and_mode():
        frames, _ = tl.frames_for(n, delta, tl.WIDTHS[0])
        out.append((f"ties-{tl.setting_id((family, n, delta))}", frames, (delta,) + DELTAS, tl.KEY, tl.FIRST_FRAME))
    return out


INPUTS = _inputs()
FORMS = ("prefix", "zigzag", "dither", "dither+zigzag+order")


def _form(form, n, key, first_frame):
    """-> keyword arguments shared by model_batch_soft, host_soft and dither_lib.model_batch_extract"""
    kw = dict(index=sl.zigzag(n) if "zigzag" in form else None, key=key if "dither" in form else None,
              order_key=ORDER_KEY if "order" in form else None)
    kw["first_frame"] = first_frame if kw["key"] is not None or kw["order_key"] is not None else 0
    return kw


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", INPUTS, ids=[c[0] for c in INPUTS])
def test_host_body_equals_the_model_and_its_hard_bits_are_the_hard_extraction(case, form):
    name, frames, deltas, key, first_frame = case
    for delta in deltas:
        for n in (1, 10, 63):
            kw = _form(form, n, key, first_frame)
            want = sl.model_batch_soft(frames, delta, n, **kw)
            got = sl.host_soft(frames, delta, n, **kw)
            assert want.size == frames.shape[0] * (frames.shape[1] // 8) * (frames.shape[2] // 8) * n
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (name, form, delta, n, diff[:5], got[diff[:5]], want[diff[:5]])
            hard = dl.model_batch_extract(frames, delta, n, **kw)
            assert np.array_equal(sl.packed_hard(got), np.packbits(hard)), (name, form, delta, n)


def test_model_bytes_on_hand_made_inputs():
    """the seven steps on values whose bytes can be read off: on the lattice 127, at the boundary 0, the parity in bit 7"""
    x = np.array([0.0, 20.0, 40.0, -20.0, 10.0, 30.0, 25.0, 15.0, 5.0, -5.0, 29.999, 20.04], np.float32)
    got = sl.model_bytes(x, 20)
    # q = rint(x / 20): 0 1 2 -1 | 0 (tie to even) 2 (tie to even) | 1 1 0 -0 | 1 1;  m = trunc((10 - |x - 20 q|) * 12.7)
    want = [127, 128 | 127, 127, 128 | 127, 0, 0, 128 | 63, 128 | 63, 63, 63, 128 | 0, 128 | 126]
    assert got.tolist() == want
    assert sl.model_bytes(np.array([3.0, 4.1], np.float32), 8).tolist() == [int((4 - 3) * 31.75), 128 | int((4 - 3.9) * 31.75)]


@pytest.mark.parametrize("n", (0, 70))
def test_n_ac_clamps(n):
    frames = dl.noise((1, 16, 16), 0, 256, seed=2)
    assert sl.host_soft(frames, 8, n).size == 4 * min(max(n, 0), 63)
    assert np.array_equal(sl.host_soft(frames, 8, n), sl.model_batch_soft(frames, 8, n))


def test_delta_not_positive_gives_zero_bytes():
    frames = dl.noise((1, 16, 16), 0, 256, seed=2)
    for delta in (0, -1):
        got = sl.host_soft(frames, delta, 10)
        assert got.size == 40 and not got.any()
        assert np.array_equal(got, sl.model_batch_soft(frames, delta, 10))


# ---- routing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 10, 63))
@pytest.mark.parametrize("flags", (0, native.SVS_EXACT_POCKETFFT, native.SVS_EXACT_GUARDED))
def test_a_soft_call_plans_the_eight_row_exact_kernel(n, flags):
    for delta in DELTAS:
        for index in (None, sl.zigzag(n), list(range(1, n + 1))):
            for dither in (False, True):
                for order in (False, True):
                    p = sl.host_plan(delta, n, index, dither, order, flags)
                    assert (p["path"], p["rows"], p["soft"]) == (sl.PATH_EXACT, 8, 1), (delta, n, index, dither, order, p)
                    assert p["dithered"] == int(dither) and p["keyed"] == int(order)
                    assert p["selected"] == int(index is not None and index != list(range(1, n + 1)))
                    assert p["qm"] == (2 if delta == 8 else 0)      # QM_POW2 / QM_F32: no QM_DOUBLE instantiation (0.1, 12.5)


def test_hard_plans_are_what_they_were():
    """the soft field defaults to off: tests/hostemu's calls (which never set it) route as before"""
    from testlib import host_extract_call
    frames = dl.noise((1, 16, 16), 0, 256, seed=2)
    _, res, _ = host_extract_call(frames, 8, 10, guarded=True)
    assert (int(res.path), int(res.rows)) == (2, 2)             # FAST, two rows
    _, res, _ = host_extract_call(frames, 8, 3)
    assert (int(res.path), int(res.rows)) == (1, 1)


# ---- refusals through the real library: none reaches the device ------------------------------------------------------------
FAKE_IN, FAKE_OUT = 0x10000, 0x20000       # never dereferenced: every case returns before any device work


def _call(lib, dev, planes=(1, 16, 16, 0, 16, 256), gray=FAKE_IN, out=FAKE_OUT, order=None, coeffs=None, dither=None, delta=8.0,
          n_ac=10, cap=None, flags=0, planes_null=False):
    pl = native.Planes(*planes)
    o = native.BlockOrder(*order) if order else None
    d = native.Dither(*dither) if dither else None
    c = None
    if coeffs is not None:
        c = native.Coeffs()
        c.count = coeffs[0]
        for i, k in enumerate(coeffs[1:]):
            c.index[i] = k
    got = C.c_uint64(0xDEAD)
    n = c.count if c is not None else max(0, min(n_ac, 63))
    cap = pl.n_frames * (pl.height // 8) * (pl.width // 8) * n if cap is None else cap
    ref = lambda s: C.byref(s) if s is not None else None    # noqa: E731
    args = [gray, None if planes_null else C.byref(pl), ref(o), ref(c), ref(d), float(delta), int(n_ac), out, cap, flags, C.byref(got)]
    rc = getattr(lib, "svs_soft_extract_dev" if dev else "svs_soft_extract")(*args, *([None] if dev else []))
    return rc, "" if rc == 0 else lib.svs_last_error().decode(), int(got.value)


REFUSALS = [
    ("planes NULL", dict(planes_null=True), native.SVS_ERR_INVALID_ARG, "planes is NULL"),
    ("gray NULL", dict(gray=None), native.SVS_ERR_INVALID_ARG, "pointer is NULL"),
    ("out NULL", dict(out=None), native.SVS_ERR_INVALID_ARG, "pointer is NULL"),
    ("planes.reserved", dict(planes=(1, 16, 16, 1, 16, 256)), native.SVS_ERR_INVALID_ARG, "svs_planes.reserved"),
    ("bad selection: DC", dict(coeffs=(2, 0, 5)), native.SVS_ERR_INVALID_ARG, "svs_coeffs.index"),
    ("bad selection: twice", dict(coeffs=(2, 5, 5)), native.SVS_ERR_INVALID_ARG, "svs_coeffs.index"),
    ("bad selection: count", dict(coeffs=(64,)), native.SVS_ERR_INVALID_ARG, "svs_coeffs.count"),
    ("bad selection: behind count", dict(coeffs=(1, 5, 6)), native.SVS_ERR_INVALID_ARG, "behind count"),
    ("dither.reserved", dict(dither=(1, 0, 1)), native.SVS_ERR_INVALID_ARG, "svs_dither.reserved"),
    ("order.reserved", dict(order=(1, 0, 1)), native.SVS_ERR_INVALID_ARG, "svs_block_order.reserved"),
    ("unequal first_frame", dict(order=(1, 4, 0), dither=(2, 5, 0)), native.SVS_ERR_INVALID_ARG, "first_frame"),
    ("SVS_READBACK", dict(flags=native.SVS_READBACK), native.SVS_ERR_INVALID_ARG, "flags"),
    ("SVS_NEAREST", dict(flags=native.SVS_NEAREST), native.SVS_ERR_INVALID_ARG, "flags"),
    ("SVS_MINMOVE", dict(flags=native.SVS_MINMOVE), native.SVS_ERR_INVALID_ARG, "flags"),
    ("SVS_KEEP_COLOUR", dict(flags=native.SVS_KEEP_COLOUR), native.SVS_ERR_INVALID_ARG, "flags"),
    ("unknown flag", dict(flags=0x400), native.SVS_ERR_INVALID_ARG, "flags"),
    ("output one byte short", dict(cap=39), native.SVS_ERR_CAPACITY, "extract needs 40 bytes, buffer has 39"),
    ("output short under a selection", dict(coeffs=(3, 1, 8, 16), n_ac=63, cap=11), native.SVS_ERR_CAPACITY, "needs 12 bytes"),
    ("packed size is not enough", dict(cap=5), native.SVS_ERR_CAPACITY, "extract needs 40 bytes"),
]


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_any_device_work(case, dev):
    _, kw, want_rc, text = case
    rc, message, got = _call(native.load(), dev, **kw)
    assert rc == want_rc and text in message, (rc, message)
    assert got in (0, 0xDEAD)                     # n_bits_out: untouched, or cleared once the planes were valid


def test_misaligned_device_pointers_are_refused():
    lib = native.load()
    assert _call(lib, True, gray=FAKE_IN + 4)[0] == native.SVS_ERR_INVALID_ARG
    assert _call(lib, True, out=FAKE_OUT + 2)[0] == native.SVS_ERR_INVALID_ARG


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
def test_the_empty_call_is_ok(dev):
    lib = native.load()
    for kw in (dict(planes=(0, 16, 16, 0, 16, 256)), dict(n_ac=0), dict(n_ac=-3), dict(planes=(0, 16, 16, 0, 16, 256), gray=None, out=None)):
        assert _call(lib, dev, **kw) == (native.SVS_OK, "", 0), kw
    # the mode bits are accepted (and, with nothing to extract, nothing else happens)
    assert _call(lib, dev, n_ac=0, flags=native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED)[0] == native.SVS_OK


def test_python_level_raises_before_the_library_is_loaded():
    from svsdct import batch
    frames = np.zeros((1, 16, 16), np.uint8)
    with pytest.raises(ValueError):
        batch.extract_soft_frames(frames, 8, 10, coeffs=[1, 2, 3])           # len != n_ac
    with pytest.raises(ValueError):
        batch.extract_soft_frames(frames, 8, 10, dither_key=-1)
    with pytest.raises(ValueError):
        batch.extract_soft_device(0, native.Planes.contiguous(1, 16, 16), 8, 10, 0, 40, mode="bogus")


# ---- what the reliability means ----------------------------------------------------------------------------------------------
STEGO_DELTA, STEGO_N = 20, 10


@pytest.fixture(scope="module")
def stego_set():
    """one 96 x 160 frame of noise in [64, 192), the full 2 400-bit payload: the cover, reference-rule stego and dithered stego"""
    from oracle.qim_dct_oracle import frame_embed
    cover = dl.noise((96, 160), 64, 192, seed=21)
    pay = dl.payload(2400, seed=4)
    _, stego, used = frame_embed(cover, STEGO_DELTA, pay, STEGO_N)
    dithered, used_d = dl.model_embed(cover, STEGO_DELTA, pay, STEGO_N, key=KEY)
    assert used == used_d == 2400
    return cover, stego, dithered


def test_reliability_of_undisturbed_stego_is_bounded_by_the_truncation_margin(stego_set):
    """A stego pixel block that does not clip moved each payload coefficient by less than MARGIN[k] <= 4.0625
    (csrc/svs_block.hpp) off its lattice point, so a <= 4.0625 and m >= floor((delta / 2 - 4.0625) * 254 / delta) = 75."""
    _, stego, _ = stego_set
    bound = int(np.floor((STEGO_DELTA / 2 - 4.0625) * 254 / STEGO_DELTA))
    assert bound == 75
    m = sv.reliability(sl.model_soft(stego, STEGO_DELTA, STEGO_N)).reshape(-1, STEGO_N)
    blocks = tl.to_blocks(stego[None])[0].reshape(-1, 64)
    unclipped = (blocks.min(1) > 0) & (blocks.max(1) < 255)
    assert unclipped.sum() > 200
    print(f"minimum reliability of {int(unclipped.sum())} unclipped stego blocks: {int(m[unclipped].min())} (bound {bound})")
    assert m[unclipped].min() >= bound


def test_comb_share(stego_set):
    """share of m >= 64 (within delta / 4 of the lattice): all of lattice stego; a fair coin - 0.5 +- 0.05 is ten standard
    deviations at 2 400 samples - for dithered stego read without the key and for the never-embedded cover"""
    cover, stego, dithered = stego_set
    share = lambda frame, **kw: float((sv.reliability(sl.model_soft(frame, STEGO_DELTA, STEGO_N, **kw)) >= 64).mean())   # noqa: E731
    s_stego, s_keyless, s_cover, s_keyed = share(stego), share(dithered), share(cover), share(dithered, key=KEY)
    print(f"share of m >= 64: stego {s_stego:.3f}, dithered stego without the key {s_keyless:.3f}, cover {s_cover:.3f}, "
          f"dithered stego with the key {s_keyed:.3f}; mean m of the cover "
          f"{sv.reliability(sl.model_soft(cover, STEGO_DELTA, STEGO_N)).mean():.1f}")
    assert s_stego == 1.0 and s_keyed == 1.0
    assert 0.45 <= s_keyless <= 0.55
    assert 0.45 <= s_cover <= 0.55
    hist = sv.margin_histogram(np.concatenate([sl.model_soft(f, STEGO_DELTA, STEGO_N) for f in (stego, cover)]), 2)
    assert hist.shape == (2, 128) and hist.dtype == np.int64 and hist.sum(1).tolist() == [2400, 2400]
    assert hist[0, :64].sum() == 0 and abs(int(hist[1, 64:].sum()) - 1200) <= 120


VOTE_SEED = 4


def test_three_copies_soft_vote_beats_majority_beats_one_copy():
    """Fixed seeds (soft_lib.vote_experiment).  The asserted row is delta = 20, n_ac = 10, pixel noise +-8; the others are
    printed for the README's table."""
    print("| delta, n, a | each copy alone | hard majority | soft vote |")
    print("|---|---|---|---|")
    rows = {}
    for delta, n, amp in sl.VOTE_ROWS:
        r = rows[(delta, n, amp)] = sl.vote_experiment(delta, n, amp, VOTE_SEED)
        print(f"| {delta}, {n}, +-{amp} | {' / '.join(str(e) for e in r['single'])} | {r['majority']} | {r['soft']} |")
    r = rows[(20, 10, 8)]
    assert min(r["single"]) > 0
    assert r["soft"] <= r["majority"] < min(r["single"]), r


# ---- svsdct/soft.py ------------------------------------------------------------------------------------------------------------
def _byte(bit, m):
    return (bit << 7) | m


def test_combine_with_a_period_that_does_not_divide_the_length():
    # period 3, 8 bytes: bit 0 has copies 0, 3, 6; bit 1 has 1, 4, 7; bit 2 has 2, 5 (the last copy is partial)
    soft = np.array([_byte(1, 10), _byte(0, 100), _byte(1, 5), _byte(0, 3), _byte(1, 20), _byte(0, 1), _byte(0, 2), _byte(1, 90)],
                    np.uint8)
    bits, score = sv.combine(soft, 3)
    assert score.dtype == np.int32 and bits.dtype == np.uint8
    assert score.tolist() == [21 - 7 - 5, -201 + 41 + 181, 11 - 3]
    assert bits.tolist() == [1, 1, 1]


def test_combine_zero_score_takes_the_first_copy():
    soft = np.array([_byte(1, 7), _byte(0, 7), _byte(0, 7), _byte(1, 7)], np.uint8)
    bits, score = sv.combine(soft, 2)
    assert score.tolist() == [0, 0] and bits.tolist() == [1, 0]


def test_combine_with_one_copy_is_the_hard_decision():
    soft = dl.noise(37, 0, 256, seed=9)
    bits, score = sv.combine(soft, soft.size)
    assert np.array_equal(bits, soft >> 7) and np.array_equal(bits, sv.hard_bits(soft))
    assert np.array_equal(np.abs(score), 2 * sv.reliability(soft).astype(np.int32) + 1)
    for bad in (0, 38):
        with pytest.raises(ValueError):
            sv.combine(soft, bad)
    with pytest.raises(TypeError):
        sv.combine(soft.astype(np.int32), 3)


def test_margin_histogram_needs_whole_frames():
    with pytest.raises(ValueError):
        sv.margin_histogram(np.zeros(7, np.uint8), 2)
    h = sv.margin_histogram(np.array([_byte(1, 5), 5, 127, _byte(1, 0)], np.uint8), 2)
    assert h[0, 5] == 2 and h[1, 127] == 1 and h[1, 0] == 1 and h.sum() == 4
