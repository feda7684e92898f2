"""Keyed block order, CPU tier: csrc/svs_order.hpp built for the host by tests/hostemu against the NumPy
restatement svsdct/order.py (both directions, bijections), pinned known-answer values (the order is a format sender and
receiver share), the block permutation helpers, and the Python / ctypes surface of the ordered entry points."""
import ctypes as C
import inspect

import numpy as np
import pytest

from testlib import hostemu
from svsdct import batch, native, order, synth
from svsdct.pipeline import FramePipeline

SIZES = (1, 2, 3, 5, 64, 65, 4800, 14400, 32400, 129600)
KEYS = (0, 1, 0x0123456789ABCDEF, 0xFFFFFFFF00000000, (1 << 64) - 1)


@pytest.fixture(scope="module")
def shim():
    return hostemu()


def _compiled(lib, key, t, n, inverse, first_frame=0):
    out = np.zeros(n, np.uint32)
    lib.bo_map(key, first_frame, t - first_frame, n, int(inverse), out.ctypes.data)
    return out.astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_compiled_order_equals_numpy_and_is_a_bijection(shim, n):
    for key in KEYS:
        for t in (0, 1, 7, 1000, 0xFFFFFFFF):
            fwd, inv = _compiled(shim, key, t, n, False), _compiled(shim, key, t, n, True)
            assert np.array_equal(fwd, order.slot_to_block(key, t, n)), (key, t)
            assert np.array_equal(inv, order.block_to_slot(key, t, n)), (key, t)
            assert np.array_equal(np.sort(fwd), np.arange(n))
            assert np.array_equal(inv[fwd], np.arange(n))


def test_first_frame_and_frame_index_only_add(shim):
    """t = first_frame + f: the split of t between the call and the frame does not matter"""
    a = _compiled(shim, 99, 12, 4800, False, first_frame=0)
    b = _compiled(shim, 99, 12, 4800, False, first_frame=5)
    assert np.array_equal(a, b)


def test_hash_is_shared_with_synth(shim):
    xs = np.arange(0, 1 << 32, 7919 * 104729, dtype=np.uint64)
    assert [shim.bo_lowbias32(int(x)) for x in xs] == [int(v) for v in synth._lowbias32(xs)]


def test_known_answers():
    """pinned: sender and receiver of other builds must compute the same order"""
    key, n = 0x0123456789ABCDEF, 4800
    s0, s7 = order.slot_to_block(key, 0, n), order.slot_to_block(key, 7, n)
    assert s0[:8].tolist() == [3755, 2983, 3810, 2921, 1812, 4706, 2979, 1505]
    assert s0[-3:].tolist() == [508, 830, 1530]
    assert order.block_to_slot(key, 0, n)[:8].tolist() == [1326, 2828, 1922, 301, 4742, 1434, 2939, 4794]
    assert s7[:8].tolist() == [752, 2017, 1201, 4294, 4188, 369, 3158, 4113]
    assert s7[-3:].tolist() == [2889, 866, 3411]
    assert order.block_to_slot(key, 7, n)[:8].tolist() == [520, 2820, 1616, 3847, 4086, 1024, 2354, 4771]
    assert order.slot_to_block(key, 0, 1).tolist() == [0]


def test_orders_differ_by_key_and_frame():
    n = 14400
    a = order.slot_to_block(1, 0, n)
    assert not np.array_equal(a, order.slot_to_block(2, 0, n))
    assert not np.array_equal(a, order.slot_to_block(1, 1, n))
    assert not np.array_equal(a, np.arange(n))
    # a payload that fills a quarter of the frame lands in every quarter of it, not in the top band
    first = np.sort(a[: n // 4])
    assert all(((first >= q * n // 4) & (first < (q + 1) * n // 4)).sum() > n // 32 for q in range(4))


def test_permute_blocks_round_trip():
    frames = synth.synthetic_frames(3, 24, 40, seed=5)
    p = order.permute_blocks(frames, 77, first_frame=4)
    assert not np.array_equal(p, frames)
    assert np.array_equal(order.unpermute_blocks(p, 77, first_frame=4), frames)
    # block sigma_t(j) of frame f is at raster position j
    sigma = order.slot_to_block(77, 5, 15)
    j = 6
    i = sigma[j]
    assert np.array_equal(p[1, (j // 5) * 8:(j // 5) * 8 + 8, (j % 5) * 8:(j % 5) * 8 + 8],
                          frames[1, (i // 5) * 8:(i // 5) * 8 + 8, (i % 5) * 8:(i % 5) * 8 + 8])
    colour = np.stack([frames] * 3, axis=-1)
    assert np.array_equal(order.permute_blocks(colour, 77, 4)[..., 1], p)


def test_key_checks():
    for bad in (-1, 1 << 64, 1.5, "3", True):
        with pytest.raises((TypeError, ValueError)):
            order.check_key(bad)
        with pytest.raises((TypeError, ValueError)):
            batch.block_order(bad)
    assert batch.block_order(None) is None
    o = batch.block_order((1 << 64) - 1, 3)
    assert (o.key, o.first_frame, o.reserved) == ((1 << 64) - 1, 3, 0)
    with pytest.raises(ValueError):
        batch.block_order(1, -1)
    with pytest.raises(ValueError):
        batch.block_order(1, 1 << 32)
    assert order.key_from_env({}) is None
    assert order.key_from_env({"SVS_BLOCK_KEY": ""}) is None
    assert order.key_from_env({"SVS_BLOCK_KEY": "0x10"}) == 16
    assert order.key_from_env({"SVS_BLOCK_KEY": "0"}) == 0
    for bad in ("-1", "0x1" + "0" * 16, "key", "1.0"):
        with pytest.raises(ValueError):
            order.key_from_env({"SVS_BLOCK_KEY": bad})


def test_python_and_ctypes_surface():
    assert C.sizeof(native.BlockOrder) == 16
    for name in ("svs_embed_ordered_dev", "svs_extract_ordered_dev", "svs_embed_ordered", "svs_extract_ordered"):
        assert name in native.SIGNATURES
    assert native.SIGNATURES["svs_embed_ordered_dev"][1][3] is C.POINTER(native.BlockOrder)
    assert native.SIGNATURES["svs_extract_ordered_dev"][1][2] is C.POINTER(native.BlockOrder)
    for fn, params in ((batch.embed_frames, ("block_key", "first_frame")), (batch.extract_frames, ("block_key", "first_frame")),
                       (batch.embed_device, ("order",)), (batch.extract_device, ("order",)),
                       (FramePipeline.__init__, ("block_key",)), (FramePipeline.submit_embed, ("first_frame",)),
                       (FramePipeline.submit_extract, ("first_frame",))):
        sig = inspect.signature(fn).parameters
        for p in params:
            assert p in sig and sig[p].default in (None, 0), (fn, p)
    lib = native.load()
    for name in ("svs_embed_ordered_dev", "svs_extract_ordered_dev", "svs_embed_ordered", "svs_extract_ordered"):
        assert hasattr(lib, name)


def test_reserved_and_planes_are_checked_without_a_gpu():
    """argument checks come before any device work: reserved != 0 is refused, an empty batch is a no-op"""
    lib = native.load()
    bad = native.BlockOrder(1, 0, 1)
    planes = native.Planes.contiguous(1, 8, 8)
    done = C.c_uint64(7)
    assert lib.svs_embed_ordered_dev(None, None, C.byref(planes), C.byref(bad), 8.0, 3, None, 0, 0, 0, C.byref(done),
                                     None) == native.SVS_ERR_INVALID_ARG
    assert b"reserved" in lib.svs_last_error()
    assert lib.svs_extract_ordered_dev(None, C.byref(planes), C.byref(bad), 8.0, 3, None, 0, 0, None, None) == \
        native.SVS_ERR_INVALID_ARG
    assert lib.svs_embed_ordered(None, None, C.byref(planes), C.byref(bad), 8.0, 3, None, 0, 0, 0, None) == \
        native.SVS_ERR_INVALID_ARG
    assert lib.svs_extract_ordered(None, C.byref(planes), C.byref(bad), 8.0, 3, None, 0, 0, None) == \
        native.SVS_ERR_INVALID_ARG
    empty = native.Planes.contiguous(0, 8, 8)
    good = native.BlockOrder(1, 0, 0)
    assert lib.svs_embed_ordered_dev(None, None, C.byref(empty), C.byref(good), 8.0, 3, None, 0, 0, 0, C.byref(done),
                                     None) == native.SVS_OK
    assert done.value == 0
