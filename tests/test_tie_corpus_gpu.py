"""GPU tier of the tie corpus (CPU tier: test_tie_corpus_cpu.py; tests/golden/make_tie_corpus.py): the four forms of the
quantiser as hipcc compiles them for the device, on frames whose payload coefficients sit on rounding ties, one float32 next
to them, in the window of the division fallback, where the reciprocal shortcut alone is wrong, and exactly on lattice points.
Everything goes through the C ABI; stego bytes, bit counts and bits are compared with the oracle or the NumPy model of the
rule, and a failure names the class and k of the first corpus block that differs (tie_lib.blame).

The ties are in the COVER frames: extraction is run on the covers (a stego's coefficients sit on lattice points), embedding
quantises the cover's coefficients."""
import numpy as np
import pytest

import coeff_select_lib as csl
import dither_lib as dl
import minmove_lib as ml
import nearest_lib as nl
import tie_lib as tl
from oracle import qim_dct_oracle as orc
from readback_lib import host_readback
from test_gpu_parity import _Dev
from test_keep_colour_cpu import TABLES, gray_of, keep_colour_rule
from svsdct import batch, coeffs, native, order
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

SETTINGS = tl.settings()
IDS = [tl.setting_id(s) for s in SETTINGS]
ONE_EACH = tl.one_setting_per_family_and_mode()
ONE_EACH_IDS = [tl.setting_id(s) for s in ONE_EACH]
MODES = ("fast", "guarded", "exact")
STR_SETTINGS = {("row1", 7, 20), ("row2", 15, 20), ("row8", 63, 20)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def bits_of(packed, n):
    return np.unpackbits(np.asarray(packed), count=n)


def dev_embed(frames, delta, n, bits, in_place=False, **kw):
    """svs_embed*_dev (the entry batch.embed_device routes **kw to) from one device buffer into another, or in place
    -> (stego, bits embedded)"""
    f, h, w = frames.shape
    packed = batch.pack_bits(bits)
    d_in, d_bits = _Dev(frames.nbytes), _Dev(packed.size + 8)
    d_out = d_in if in_place else _Dev(frames.nbytes)
    d_in.put(frames)
    if not in_place:
        d_out.put(np.full(frames.nbytes, 0xEE, np.uint8))
    d_bits.put(np.concatenate([packed, np.zeros(8, np.uint8)]))
    used = batch.embed_device(d_in.ptr.value, d_out.ptr.value, Planes.contiguous(f, h, w), delta, n, d_bits.ptr.value, 0, bits.size,
                              **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    if not in_place:
        assert np.array_equal(d_in.get().reshape(frames.shape), frames), "the call wrote to its input"
    return d_out.get().reshape(frames.shape), used


def dev_extract(frames, delta, n, **kw):
    """svs_extract*_dev -> 0/1 bits; the bytes behind the stream stay as they were"""
    f, h, w = frames.shape
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    d_in, d_out = _Dev(frames.nbytes), _Dev(nbytes + 8)
    d_in.put(frames)
    d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
    got = batch.extract_device(d_in.ptr.value, Planes.contiguous(f, h, w), delta, n, d_out.ptr.value, nbytes, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    res = d_out.get()
    assert got == cap and (res[nbytes:] == 0x5A).all()
    return bits_of(res[:nbytes], cap)


def case(n, delta, width, index=None):
    frames, where = tl.frames_for(n, delta, width)
    return np.array(frames), where, tl.payload_for(frames, where, n, index)


# ---- embed -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_embed_calls_give_the_oracles_pixels(setting):
    _, n, delta = setting
    for width in tl.WIDTHS:
        frames, where, bits = case(n, delta, width)
        want, used = orc.batch_embed(frames, delta, bits, n)
        for mode in MODES:
            what = (setting, width, mode)
            got, u = batch.embed_frames(frames, delta, n, bits, mode=mode)                   # svs_embed
            assert u == used == bits.size and np.array_equal(got, want), (what, "svs_embed", tl.blame(where, got, want))
            for in_place in (False, True):                                                    # svs_embed_dev
                got, u = dev_embed(frames, delta, n, bits, in_place, mode=mode)
                assert u == used and np.array_equal(got, want), (what, "svs_embed_dev", in_place, tl.blame(where, got, want))


# ---- extract from the covers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_extract_calls_give_the_oracles_bits_of_the_covers(setting):
    _, n, delta = setting
    for width in tl.WIDTHS:
        frames, where, _ = case(n, delta, width)
        want = orc.batch_extract_bits(frames, delta, n)
        for mode in MODES:
            what = (setting, width, mode)
            packed, got_n = batch.extract_frames(frames, delta, n, mode=mode)                  # svs_extract
            got = bits_of(packed, got_n)
            assert got_n == want.size and np.array_equal(got, want), (what, "svs_extract", tl.blame(where, got, want, n))
            got = dev_extract(frames, delta, n, mode=mode)                                     # svs_extract_dev
            assert np.array_equal(got, want), (what, "svs_extract_dev", tl.blame(where, got, want, n))
            if setting in STR_SETTINGS:
                text = batch.extract_frames_str(frames, delta, n, mode=mode)                   # svs_extract_str
                assert text == orc.bits_to_str(want), (what, "svs_extract_str")


# ---- keyed block order -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ONE_EACH, ids=ONE_EACH_IDS)
def test_ordered_calls_give_the_oracles_result_on_permuted_frames(setting):
    _, n, delta = setting
    width = tl.WIDTHS[n % 2]
    frames, where, bits = case(n, delta, width)
    nblk = (frames.shape[1] // 8) * (frames.shape[2] // 8)
    perm = [order.slot_to_block(tl.ORDER_KEY, tl.FIRST_FRAME + f, nblk) for f in range(2)]
    permuted = order.permute_blocks(frames, tl.ORDER_KEY, tl.FIRST_FRAME)
    stego, used = orc.batch_embed(permuted, delta, bits, n)
    want = order.unpermute_blocks(stego, tl.ORDER_KEY, tl.FIRST_FRAME)
    want_bits = orc.batch_extract_bits(permuted, delta, n)
    o = batch.block_order(tl.ORDER_KEY, tl.FIRST_FRAME)
    for mode in MODES:
        what = (setting, mode)
        got, u = batch.embed_frames(frames, delta, n, bits, mode=mode, block_key=tl.ORDER_KEY, first_frame=tl.FIRST_FRAME)
        assert u == used and np.array_equal(got, want), (what, "svs_embed_ordered", tl.blame(where, got, want))
        got, u = dev_embed(frames, delta, n, bits, mode=mode, order=o)
        assert u == used and np.array_equal(got, want), (what, "svs_embed_ordered_dev", tl.blame(where, got, want))
        packed, got_n = batch.extract_frames(frames, delta, n, mode=mode, block_key=tl.ORDER_KEY, first_frame=tl.FIRST_FRAME)
        got = bits_of(packed, got_n)
        assert np.array_equal(got, want_bits), (what, "svs_extract_ordered", tl.blame(where, got, want_bits, n, perm))
        got = dev_extract(frames, delta, n, mode=mode, order=o)
        assert np.array_equal(got, want_bits), (what, "svs_extract_ordered_dev", tl.blame(where, got, want_bits, n, perm))


# ---- coefficient selection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ONE_EACH, ids=ONE_EACH_IDS)
def test_select_calls_on_the_tie_coefficient_alone(setting):
    family, n, delta = setting
    zigzag6 = [int(k) for k in coeffs.selection("zigzag:6", 3)]          # 3, 10, 17: one tie coefficient of every family
    selections = [[k] for k in tl.FAMILIES[family][1]] + [zigzag6]
    assert any(k in zigzag6 for k in tl.FAMILIES[family][1])
    width = tl.WIDTHS[n % 2]
    for index in selections:
        frames, where, bits = case(n, delta, width, index)
        mine = {fp: r for fp, r in where.items() if r["k"] in index}
        assert len(mine) >= 8
        want, used = csl.select_batch_embed(frames, delta, bits, index)
        want_bits = np.concatenate([csl.select_extract_bits(f, delta, index) for f in frames])
        for mode in ("guarded", "exact"):
            what = (setting, index, mode)
            got, u = dev_embed(frames, delta, len(index), bits, mode=mode, coeffs=index)              # svs_embed_select_dev
            assert u == used == bits.size and np.array_equal(got, want), (what, tl.blame(mine, got, want))
            got = dev_extract(frames, delta, len(index), mode=mode, coeffs=index)                     # svs_extract_select_dev
            assert np.array_equal(got, want_bits), (what, tl.blame(mine, got, want_bits, len(index)))
        if index != zigzag6:
            want_n, _ = csl.select_batch_embed(frames, delta, bits, index, nearest=True)
            got, _ = dev_embed(frames, delta, len(index), bits, coeffs=index, nearest=True)
            assert np.array_equal(got, want_n), (setting, index, "nearest", tl.blame(mine, got, want_n))
            want_m, _ = ml.model_batch(frames, delta, bits, len(index), index=index)
            got, _ = dev_embed(frames, delta, len(index), bits, coeffs=index, minmove=True)
            assert np.array_equal(got, want_m), (setting, index, "minmove", tl.blame(mine, got, want_m))


# ---- rules and read-back -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_nearest_and_minmove_on_every_embed_entry(setting):
    """the `lattice` blocks carry the bit that differs from their index's parity: c == c0, and the direction is the reference's
    (the models', tests/test_tie_corpus_cpu.py::test_lattice_blocks_take_the_reference_direction_in_the_model)"""
    _, n, delta = setting
    width = tl.WIDTHS[n % 2]
    frames, where, bits = case(n, delta, width)
    assert sum(r["class"] == "lattice" for r in where.values()) >= 2
    for flag, (want, used) in ((dict(nearest=True), nl.model_batch(frames, delta, bits, n)),
                               (dict(minmove=True), ml.model_batch(frames, delta, bits, n))):
        for mode in MODES:
            what = (setting, flag, mode)
            got, u = batch.embed_frames(frames, delta, n, bits, mode=mode, **flag)
            assert u == used == bits.size and np.array_equal(got, want), (what, "svs_embed", tl.blame(where, got, want))
            for in_place in (False, True):
                got, u = dev_embed(frames, delta, n, bits, in_place, mode=mode, **flag)
                assert u == used and np.array_equal(got, want), (what, "svs_embed_dev", in_place, tl.blame(where, got, want))


@pytest.mark.parametrize("setting", ONE_EACH, ids=ONE_EACH_IDS)
def test_nearest_and_minmove_on_the_ordered_readback_and_colour_entries(setting):
    """the same two rules through the embed entries the previous test leaves out (the select and dithered entries take them in
    their own tests).  Ordered: the payload is laid out by stream slot, so that every `lattice` block still meets its
    recorded bit; the model runs on the block-permuted frames.  Read-back: the host pass started from the model's stego.
    Fused colour, plain and keep-colour, both weight tables: the gray of the result is the model's stego."""
    _, n, delta = setting
    frames, where, bits = case(n, delta, tl.WIDTHS[n % 2])
    nblk = (frames.shape[1] // 8) * (frames.shape[2] // 8)
    perm = [order.slot_to_block(tl.ORDER_KEY, tl.FIRST_FRAME + f, nblk) for f in range(2)]
    slot_of = [{int(p): s for s, p in enumerate(perm[f])} for f in range(2)]
    by_slot = {(f, slot_of[f][p]): r for (f, p), r in where.items()}
    bits_o = tl.payload_for(frames, by_slot, n)
    permuted = order.permute_blocks(frames, tl.ORDER_KEY, tl.FIRST_FRAME)
    for (f, s), r in by_slot.items():
        assert np.array_equal(tl.to_blocks(permuted)[f, s], tl.to_blocks(frames)[f, perm[f][s]])
    assert sum(r["class"] == "lattice" for r in where.values()) >= 2
    o = batch.block_order(tl.ORDER_KEY, tl.FIRST_FRAME)
    bgr = np.ascontiguousarray(np.repeat(frames[..., None], 3, axis=3))
    d_counts = _Dev(16)
    for flag, model in ((dict(nearest=True), nl.model_batch), (dict(minmove=True), ml.model_batch)):
        # svs_embed_ordered, svs_embed_ordered_dev
        stego, used = model(permuted, delta, bits_o, n)
        want = order.unpermute_blocks(stego, tl.ORDER_KEY, tl.FIRST_FRAME)
        assert used == bits_o.size
        for mode in MODES:
            what = (setting, flag, mode)
            got, u = batch.embed_frames(frames, delta, n, bits_o, mode=mode, block_key=tl.ORDER_KEY, first_frame=tl.FIRST_FRAME, **flag)
            assert u == used and np.array_equal(got, want), (what, "svs_embed_ordered", tl.blame(where, got, want))
            got, u = dev_embed(frames, delta, n, bits_o, mode=mode, order=o, **flag)
            assert u == used and np.array_equal(got, want), (what, "svs_embed_ordered_dev", tl.blame(where, got, want))
        # svs_embed_readback_dev
        start, used = model(frames, delta, bits, n)
        want, want_counts, _ = host_readback(start, delta, n, bits)
        d_counts.put(np.zeros(2, np.uint64))
        got, u = dev_embed(frames, delta, n, bits, readback=True, d_counts=d_counts.ptr.value, **flag)
        assert u == used and np.array_equal(got, want), (setting, flag, "svs_embed_readback_dev", tl.blame(where, got, want))
        assert tuple(int(c) for c in d_counts.get(16, np.uint64)) == want_counts
        # svs_embed_bgr_dev
        for name, weights in TABLES.items():
            for mode in ("guarded", "exact"):
                what = (setting, flag, name, mode)
                got, gray, u = dev_embed_bgr(bgr, delta, n, bits, mode=mode, weights=weights, **flag)
                assert np.array_equal(gray, frames), (what, "the gray plane is not the corpus frame")
                assert u == used and np.array_equal(got, np.repeat(start[..., None], 3, axis=3)), (what, tl.blame(where, got[..., 0], start))
                kept, _, u = dev_embed_bgr(bgr, delta, n, bits, mode=mode, weights=weights, keep_colour=True, **flag)
                assert u == used and np.array_equal(gray_of(kept, weights), start), (what, "keep-colour",
                                                                                      tl.blame(where, gray_of(kept, weights), start))
                assert np.array_equal(kept, keep_colour_rule(bgr, start, weights)), (what, "keep-colour")


@pytest.mark.parametrize("setting", ONE_EACH, ids=ONE_EACH_IDS)
def test_readback_call_equals_the_host_pass(setting):
    _, n, delta = setting
    frames, where, bits = case(n, delta, tl.WIDTHS[n % 2])
    reference, used = orc.batch_embed(frames, delta, bits, n)
    want, want_counts, _ = host_readback(reference, delta, n, bits)
    d_counts = _Dev(16)
    d_counts.put(np.zeros(2, np.uint64))
    got, u = dev_embed(frames, delta, n, bits, readback=True, d_counts=d_counts.ptr.value)          # svs_embed_readback_dev
    assert u == used and np.array_equal(got, want), (setting, tl.blame(where, got, want))
    assert tuple(int(c) for c in d_counts.get(16, np.uint64)) == want_counts


# ---- dither ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [8, 0.25, 20, 12.5, 7.3, 0.1])
def test_dithered_calls_on_the_dither_ties(delta):
    for n in (3, 10):
        frames, where, bits = case(n, delta, tl.WIDTHS[n % 2])
        slotted = {fp: r for fp, r in where.items() if r["class"] == "dither_tie"}
        assert len(slotted) >= (8 if n == 10 else 4)
        kw = dict(dither_key=tl.KEY, first_frame=tl.FIRST_FRAME)
        want_cover = dl.model_batch_extract(frames, delta, n, key=tl.KEY, first_frame=tl.FIRST_FRAME)
        for mode in ("guarded", "exact"):
            got = dev_extract(frames, delta, n, mode=mode, **kw)                                     # svs_extract_dithered_dev
            assert np.array_equal(got, want_cover), (delta, n, mode, "cover", tl.blame(where, got, want_cover, n))
        for rule in ("reference", "nearest", "minmove"):
            want, used = dl.model_batch_embed(frames, delta, bits, n, rule, key=tl.KEY, first_frame=tl.FIRST_FRAME)
            want_bits = dl.model_batch_extract(want, delta, n, key=tl.KEY, first_frame=tl.FIRST_FRAME)
            for in_place in (False, True):
                got, u = dev_embed(frames, delta, n, bits, in_place, nearest=rule == "nearest", minmove=rule == "minmove",
                                    **kw)                                                      # svs_embed_dithered_dev
                assert u == used == bits.size and np.array_equal(got, want), (delta, n, rule, in_place, tl.blame(where, got, want))
            back = dev_extract(got, delta, n, **kw)
            assert np.array_equal(back, want_bits), (delta, n, rule, "stego", tl.blame(where, back, want_bits, n))


# ---- fused colour ------------------------------------------------------------------------------------------------------
def dev_embed_bgr(bgr, delta, n, bits, **kw):
    """svs_embed_bgr_dev -> (stego BGR, the gray reference plane, bits embedded)"""
    f, h, w, _ = bgr.shape
    packed = batch.pack_bits(bits)
    d_in, d_out, d_gray, d_bits = _Dev(bgr.nbytes), _Dev(bgr.nbytes), _Dev(f * h * w), _Dev(packed.size + 8)
    d_in.put(bgr)
    d_bits.put(np.concatenate([packed, np.zeros(8, np.uint8)]))
    used = batch.embed_bgr_device(d_in.ptr.value, d_out.ptr.value, d_gray.ptr.value, Planes.contiguous(f, h, w), delta, n,
                                  d_bits.ptr.value, 0, bits.size, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    return d_out.get().reshape(bgr.shape), d_gray.get().reshape(f, h, w), used


def dev_extract_bgr(bgr, delta, n, **kw):
    f, h, w, _ = bgr.shape
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    d_in, d_out = _Dev(bgr.nbytes), _Dev(nbytes + 8)
    d_in.put(bgr)
    d_out.put(np.full(nbytes + 8, 0x5A, np.uint8))
    got = batch.extract_bgr_device(d_in.ptr.value, Planes.contiguous(f, h, w), delta, n, d_out.ptr.value, nbytes, **kw)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    assert got == cap
    return bits_of(d_out.get()[:nbytes], cap)


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_fused_colour_calls_on_gray_valued_bgr(setting):
    """B = G = R = the corpus gray: both weight tables sum to their power of two, so the kernel's gray plane is the corpus
    frame itself (asserted first) and its quantiser sees the corpus coefficients"""
    _, n, delta = setting
    width = tl.WIDTHS[n % 2]
    frames, where, bits = case(n, delta, width)
    bgr = np.ascontiguousarray(np.repeat(frames[..., None], 3, axis=3))
    want, used = orc.batch_embed(frames, delta, bits, n)
    want_bits = orc.batch_extract_bits(frames, delta, n)
    for name, weights in TABLES.items():
        assert np.array_equal(gray_of(bgr, weights), frames)
        for mode in ("guarded", "exact"):
            what = (setting, name, mode)
            got, gray, u = dev_embed_bgr(bgr, delta, n, bits, mode=mode, weights=weights)
            assert np.array_equal(gray, frames), (what, "the gray plane is not the corpus frame")
            assert u == used and np.array_equal(got, np.repeat(want[..., None], 3, axis=3)), (what, tl.blame(where, got[..., 0], want))
            kept, gray, u = dev_embed_bgr(bgr, delta, n, bits, mode=mode, weights=weights, keep_colour=True)
            assert np.array_equal(gray, frames) and u == used
            assert np.array_equal(gray_of(kept, weights), want), (what, "keep-colour", tl.blame(where, gray_of(kept, weights), want))
            assert np.array_equal(kept, keep_colour_rule(bgr, want, weights)), (what, "keep-colour")
        got = dev_extract_bgr(bgr, delta, n, weights=weights)                                        # the covers
        assert np.array_equal(got, want_bits), (setting, name, tl.blame(where, got, want_bits, n))
