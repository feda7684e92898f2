"""Every dispatched kernel instantiation against the oracle: each case of tests/kernel_matrix.py (KERNEL_CASES) runs one C ABI
call - gray embed and extract, read-back, fused colour embed, fused colour extraction - on small structured frames, and its
result is compared with the reference's (oracle/qim_dct_oracle.py): stego pixels, bit counts and extracted bits.
tests/test_kernel_matrix_cpu.py checks that the cases launch all the instantiations in the library and no other."""
import numpy as np
import pytest

import kernel_matrix as km
from oracle import qim_dct_oracle as orc
from readback_lib import content, host_readback
from test_block_order_gpu import cover
from test_gpu_parity import _Dev, d_gray_default
from test_keep_colour_cpu import TABLES, gray_of, keep_colour_rule
from test_keep_colour_gpu import colour_cover
from testlib import experiments_library, structured_covers, using_library
from svsdct import batch, colour, native, order, synth
from svsdct.native import Planes

pytestmark = pytest.mark.gpu
W15 = TABLES["15-bit"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def gray_frames(case, seed):
    """frame 0: noise with flat, clipping and ramp blocks (guard replays, tie settles); frame 1: blocks whose row-0 / column-0
    coefficients cancel exactly and a text-like half; frame 2: natural-like content with a flat panel and letterbox bars.
    Read-back: letterboxed, flat black and natural frames (the reference's stego fails to read back on the first two)."""
    f, h, w = km.SHAPES[case.shape]
    if case.entry == "readback":
        return np.stack([content(k, h, w, seed=seed + i) for i, k in enumerate(("letterbox", "flat0", "natural"))])
    frames = cover(f, h, w, seed)
    sc = structured_covers(h, w, seed)
    half = (w // 16) * 8
    frames[1, :, :half] = sc["outer_product_blocks"][:, :half]
    frames[1, :, half:] = sc["text_4x4_binary"][:, half:]
    frames[2] = sc["natural_like"]
    return frames


def stream_of(case, seed):
    """(the whole stream, the bits the call offers)"""
    bits = synth.synthetic_bits(km.BIT_OFFSET + km.budget(case), seed=seed)
    return bits, bits[km.BIT_OFFSET:]


def oracle_embed(frames, case, payload):
    """the oracle's stego and bit count; keyed: the oracle on block-permuted frames, permuted back"""
    if not case.keyed:
        return orc.batch_embed(frames, case.delta, payload, case.n)
    stego, used = orc.batch_embed(order.permute_blocks(frames, km.KEY, km.FIRST_FRAME), case.delta, payload, case.n)
    return order.unpermute_blocks(stego, km.KEY, km.FIRST_FRAME), used


def oracle_bits(frames, case):
    src = order.permute_blocks(frames, km.KEY, km.FIRST_FRAME) if case.keyed else frames
    return orc.batch_extract_bits(src, case.delta, case.n)


def embed_device(frames, case, stream, readback=False):
    """svs_embed*_dev from one device buffer into another (no copy is skipped as in place) -> (stego, used, counts)"""
    f, h, w = frames.shape
    planes = Planes.contiguous(f, h, w)
    packed = batch.pack_bits(stream)
    d_in, d_out, d_bits, d_counts = _Dev(frames.nbytes), _Dev(frames.nbytes), _Dev(packed.size + 8), _Dev(16)
    d_in.put(frames)
    d_bits.put(np.concatenate([packed, np.zeros(8, np.uint8)]))
    d_counts.put(np.zeros(2, np.uint64))
    o = batch.block_order(km.KEY, km.FIRST_FRAME) if case.keyed else None
    used = batch.embed_device(d_in.ptr.value, d_out.ptr.value, planes, case.delta, case.n, d_bits.ptr.value, km.BIT_OFFSET,
                              km.budget(case), mode=case.mode, order=o, readback=readback,
                              d_counts=d_counts.ptr.value if readback else 0)
    native.check(native.load().svs_stream_synchronize(None), "sync")
    return d_out.get().reshape(frames.shape), used, tuple(int(c) for c in d_counts.get(16, np.uint64))


def replayed_blocks(frames, case, stream, want):
    """the same call through the experiments library with its replay counter: blocks the streaming kernel redid exactly"""
    exp = experiments_library()
    d_cnt = _Dev(8)
    d_cnt.put(np.zeros(1, np.uint64))
    exp.svs_guard_counter_set(d_cnt.ptr)
    try:
        with using_library(exp):
            stego, used, _ = embed_device(frames, case, stream, readback=case.entry == "readback")
    finally:
        exp.svs_guard_counter_set(None)
    assert used == want[1] and np.array_equal(stego, want[0])
    return int(d_cnt.get(8, np.uint64)[0])


def check_extract(frames, case, label):
    packed, n_bits = batch.extract_frames(frames, case.delta, case.n, mode=case.mode,
                                          block_key=km.KEY if case.keyed else None, first_frame=km.FIRST_FRAME)
    want = oracle_bits(frames, case)
    assert n_bits == km.capacity(case) == want.size, (label, n_bits, want.size)
    got = np.unpackbits(packed, count=n_bits)
    assert np.array_equal(got, want), (label, int((got != want).sum()))


def block_view(frames):
    f, h, w = frames.shape
    return frames.reshape(f, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 64)


def failing(frames, case, payload):
    """per block (raster order of the oracle's view): the block carries payload bits that the oracle does not read back"""
    n = km.clamp_n(case.n)
    got = oracle_bits(frames, case)[: payload.size]
    bad = np.zeros(frames.size // 64, bool)
    np.logical_or.at(bad, np.arange(payload.size) // n, got != payload)
    return bad


def permuted(frames, case):
    return order.permute_blocks(frames, km.KEY, km.FIRST_FRAME) if case.keyed else frames


def run_gray(case, seed):
    frames = gray_frames(case, seed)
    stream, payload = stream_of(case, seed + 1)
    want = oracle_embed(frames, case, payload)
    stego, used, _ = embed_device(frames, case, stream)
    assert used == want[1], (used, want[1])
    assert np.array_equal(stego, want[0]), np.argwhere(stego != want[0])[:4]
    if km.plan_embed(case)["path"] == km.STREAMING:
        assert replayed_blocks(frames, case, stream, want) > 0, "no block was redone exactly: the replay path is not tested"
    if km.capacity(case) == 0:
        return
    if km.plan_extract(case)["path"] == km.FAST:
        assert case.delta >= km.FAST_ORACLE_DELTA_MIN
    check_extract(stego, case, "stego")
    check_extract(frames, case, "cover")              # never-embedded frames: ties of c / delta are frequent on covers


def run_readback(case, seed):
    frames = gray_frames(case, seed)
    stream, payload = stream_of(case, seed + 1)
    ref, ref_used = oracle_embed(frames, case, payload)
    out, used, counts = embed_device(frames, case, stream, readback=True)
    assert used == ref_used == payload.size
    # (a) the host build of csrc/svs_readback.hpp over the oracle's stego
    want, want_counts, _ = host_readback(ref, case.delta, case.n, stream, bit_offset=km.BIT_OFFSET, n_bits=payload.size,
                                         block_key=km.KEY if case.keyed else None, first_frame=km.FIRST_FRAME)
    assert np.array_equal(out, want) and counts == want_counts, (counts, want_counts)
    # (b) against the oracle itself: the blocks that differ from its stego are the repaired ones, and each reads back its bits;
    # every other block is the oracle's; the blocks left failing are the unrepaired ones
    changed = (block_view(permuted(out, case)) != block_view(permuted(ref, case))).any(axis=1)
    assert int(changed.sum()) == counts[0]
    bad_after = failing(out, case, payload)
    assert not (bad_after & changed).any()
    assert int(bad_after.sum()) == counts[1]
    assert int(failing(ref, case, payload).sum()) == counts[0] + counts[1]
    if km.plan_embed(case)["path"] == km.STREAMING:
        assert replayed_blocks(frames, case, stream, (out, used)) > 0


def run_bgr(case, seed):
    f, h, w = km.SHAPES[case.shape]
    bgr = colour_cover(f, h, w, seed)
    gray = d_gray_default(bgr)
    stream, payload = stream_of(case, seed + 1)
    want, want_used = orc.batch_embed(gray, case.delta, payload, case.n)
    out, got_gray, used = batch.embed_bgr_frames(bgr, case.delta, case.n, stream, bit_offset=km.BIT_OFFSET,
                                                 n_bits=payload.size, mode=case.mode, keep_colour=case.keep)
    assert used == want_used
    assert np.array_equal(got_gray, gray)
    if case.keep:
        assert np.array_equal(out, keep_colour_rule(bgr, want, W15))
        assert np.array_equal(colour.device_gray(out), want) and np.array_equal(gray_of(out, W15), want)
    else:
        assert np.array_equal(out, np.repeat(want[..., None], 3, axis=3))


def run_bgr_extract(case, seed):
    f, h, w = km.SHAPES[case.shape]
    bgr = colour_cover(f, h, w, seed)
    gray = d_gray_default(bgr)
    _, payload = stream_of(case, seed + 1)
    stego, _ = orc.batch_embed(gray, case.delta, payload, case.n)
    if km.plan_extract(case)["path"] == km.FAST:
        assert case.delta >= km.FAST_ORACLE_DELTA_MIN
    for label, src, src_gray in (("cover", bgr, gray), ("stego", np.repeat(stego[..., None], 3, axis=3), stego)):
        packed, n_bits = batch.extract_bgr_frames(src, case.delta, case.n)
        want = orc.batch_extract_bits(src_gray, case.delta, case.n)
        assert n_bits == km.capacity(case) == want.size
        got = np.unpackbits(packed, count=n_bits)
        assert np.array_equal(got, want), (label, int((got != want).sum()))


RUN = {"gray": run_gray, "readback": run_readback, "bgr": run_bgr, "bgr_extract": run_bgr_extract}


@pytest.mark.parametrize("case", km.KERNEL_CASES, ids=[c.id for c in km.KERNEL_CASES])
def test_kernel_instantiation_equals_the_oracle(case):
    RUN[case.entry](case, seed=km.KERNEL_CASES.index(case) + 1)
