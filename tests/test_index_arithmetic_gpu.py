"""The kernels' index arithmetic on the GPU, at the sizes where it leaves its trivial regime (the expressions themselves:
tests/test_index_arithmetic_cpu.py):

a. the workgroup -> tile maps at grid sizes around their branch points (a frame of 8 rows and 8 B columns has exactly B blocks);
b. pixel offsets past 2^31 and 2^32 bytes in every kernel family: tiny frames whose pitches put them gigabytes apart, in one
   allocation that spans them (tests/index_lib.py SparseFrames) - a truncated offset lands inside it and shows as a mismatch
   or a written sentinel, not as a fault;
c. payload positions (bit_offset) past 2^32 in every payload reader;
d. extract output positions past 2^32 bits.

Every call is a _dev call on device buffers that the test frees on exit; expected values are the oracle's on the tight frames
(a pitched call equals the tight call by definition), or those of the CPU restatements the other test modules use."""
import ctypes as C

import numpy as np
import pytest

import coeff_select_lib as csl
import helper_refs as refs
import kernel_matrix as km
from index_lib import DevBuf, SparseFrames
from oracle import qim_dct_oracle as orc
from readback_lib import host_readback
from test_keep_colour_cpu import TABLES, keep_colour_rule
from svsdct import batch, native, order, synth
from svsdct.native import Planes

pytestmark = pytest.mark.gpu
W15 = TABLES["15-bit"]
KEY, T0 = km.KEY, km.FIRST_FRAME


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def noise(shape, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.uint8)


def bgr_gray(bgr):
    return refs.bgr_to_gray(bgr).astype(np.uint8)


class Payload(DevBuf):
    """a packed payload on the device, 8 zero bytes behind it"""

    def __init__(self, bits):
        packed = batch.pack_bits(bits)
        super().__init__(packed.size + 8)
        self.put(np.concatenate([packed, np.zeros(8, np.uint8)]))


def embed_tight(frames, delta, n, bits, mode, key=None, coeffs=None, prefill=None):
    """svs_embed*_dev of tight frames from one device buffer into another -> (stego, bits embedded)"""
    f, h, w = frames.shape
    with DevBuf(frames.nbytes) as d_in, DevBuf(frames.nbytes) as d_out, Payload(bits) as d_bits:
        d_in.put(frames)
        d_out.put(prefill) if prefill is not None else d_out.memset(0xC3)
        used = batch.embed_device(d_in.addr, d_out.addr, Planes.contiguous(f, h, w), delta, n, d_bits.addr, 0, len(bits), mode=mode,
                                  order=batch.block_order(key, T0) if key is not None else None, coeffs=coeffs)
        return d_out.get().reshape(frames.shape), used


def extract_tight(frames, delta, n, mode, key=None, coeffs=None):
    """svs_extract*_dev of tight frames -> 0/1 bits; the bytes behind the output must stay as they were"""
    f, h, w = frames.shape
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    with DevBuf(frames.nbytes) as d_in, DevBuf(nbytes + 64) as d_out:
        d_in.put(frames)
        d_out.memset(0xA5)
        got = batch.extract_device(d_in.addr, Planes.contiguous(f, h, w), delta, n, d_out.addr, nbytes, mode=mode,
                                   order=batch.block_order(key, T0) if key is not None else None, coeffs=coeffs)
        out = d_out.get()
    assert got == cap and (out[nbytes:] == 0xA5).all()
    return np.unpackbits(out[:nbytes], count=cap)


# ---- a. tile maps -----------------------------------------------------------------------------------------------------
EXTRACT_G = (255, 256, 257, 264, 511, 512, 513, 775, 1025)
EMBED_G = tuple(range(1, 18)) + (63, 64, 65, 255, 257)
THIN_G = (1, 2, 7, 8, 9, 17, 65, 257)


@pytest.mark.parametrize("delta", [8, 7.5])
def test_one_row_extract_tile_map_around_whole_rounds(delta):
    """extract_exact_kernel<1> (tile_of with chunk = 32: runs of 32 tiles per XCD-group in whole rounds of 256 workgroups,
    the identity past them) at B = 256 g and 256 g - 3 blocks, n = 1 and 7, against the oracle's bits.  The oracle runs once
    per g and step, at n = 7 on the 256 g blocks: a block's bits are those of coefficients 1..7 in order, so n = 1 is every
    seventh bit, and the frame of 256 g - 3 blocks is the first columns of the larger one."""
    for g in EXTRACT_G:
        frame = noise((1, 8, 8 * 256 * g), g)
        want7 = orc.batch_extract_bits(frame, delta, 7).reshape(-1, 7)
        for b in (256 * g, 256 * g - 3):
            for n in (1, 7):
                got = extract_tight(np.ascontiguousarray(frame[:, :, :8 * b]), delta, n, "guarded")
                want = want7[:b, :n].reshape(-1)
                assert np.array_equal(got, want), (g, b, n, int((got != want).sum()))


@pytest.mark.parametrize("per_wg,tail", [(256, 5), (512, 6)], ids=["one_block_per_lane", "two_blocks_per_lane"])
def test_one_row_embed_tile_map(per_wg, tail):
    """embed_row1_kernel (kEighth), guarded, n = 3, delta = 8, B = per_wg g - tail blocks: the last tile is partial and, for
    g % 8 != 1, lands on a workgroup in the middle of the grid.  B odd: one block per lane, 256 per workgroup; B even (16-byte
    pitches, hence tail 6, not 5): two per lane, 512 per workgroup.  Payload: the capacity less 2 bits.  Stego byte for byte."""
    for g in EMBED_G:
        b = per_wg * g - tail
        assert (b % 2 == 0) == (per_wg == 512)
        frame = noise((1, 8, 8 * b), 1000 + g)
        frame[0, :, : 8 * (b // 5)] = frame[0, 0, 0]                     # flat blocks: the guard replays them
        bits = synth.synthetic_bits(3 * b - 2, seed=g)
        want, want_used = orc.batch_embed(frame, 8, bits, 3)
        got, used = embed_tight(frame, 8, 3, bits, "guarded")
        assert used == want_used == bits.size
        assert np.array_equal(got, want), (g, b, np.argwhere(got != want)[:3])


def _gray_case(g, n, seed):
    b = 256 * g - 5
    frame = noise((1, 8, 8 * b), seed + g)
    frame[0, :, : 8 * (b // 7)] = 200
    return b, frame, synth.synthetic_bits(n * b - 2, seed=seed + g)


def test_two_row_and_exact_embed_tile_maps():
    """embed_kernel<2> (n = 10, guarded) and embed_exact_kernel (n = 20) at the thinned grid sizes"""
    for g in THIN_G:
        for n, mode in ((10, "guarded"), (20, "guarded")):
            b, frame, bits = _gray_case(g, n, 2000 + n)
            want, want_used = orc.batch_embed(frame, 8, bits, n)
            got, used = embed_tight(frame, 8, n, bits, mode)
            assert used == want_used and np.array_equal(got, want), (g, n, np.argwhere(got != want)[:3])


def test_fast_extract_three_rows_tile_map():
    """extract_kernel<3> (FAST, n = 20) at the thinned grid sizes"""
    for g in THIN_G:
        b, frame, _ = _gray_case(g, 20, 3000)
        got = extract_tight(frame, 8, 20, "fast")
        want = orc.batch_extract_bits(frame, 8, 20)
        assert np.array_equal(got, want), (g, int((got != want).sum()))


def test_copy_path_tile_map():
    """an empty payload: embed_row1_kernel<0> copies every block; the output starts as the complement of the input"""
    for g in THIN_G:
        for b in (256 * g - 5, 512 * g - 6):
            frame = noise((1, 8, 8 * b), 4000 + g)
            got, used = embed_tight(frame, 8, 3, np.zeros(0, np.uint8), "guarded", prefill=~frame)
            assert used == 0 and np.array_equal(got, frame), (g, b)


def bgr_call(bgr, delta, n, bits, mode, keep, readback=False, bit_offset=0, d_bits=None, pitches=None):
    """svs_embed_bgr*_dev -> (BGR out, gray reference, used, counts).  pitches: None (tight buffers) or
    ((in row, in frame), (out row, out frame), (ref row, ref frame)) - SparseFrames, sentinels checked"""
    f, h, w, _ = bgr.shape
    tight = ((3 * w, 3 * w * h), (3 * w, 3 * w * h), (w, w * h))
    (irp, ifp), (orp, ofp), (grp, gfp) = pitches or tight
    own_bits = d_bits is None
    d_bits = Payload(bits) if own_bits else d_bits
    try:
        with SparseFrames(f, h, w, irp, ifp, px=3) as d_in, SparseFrames(f, h, w, orp, ofp, px=3) as d_out, \
                SparseFrames(f, h, w, grp, gfp) as d_ref, DevBuf(16) as d_counts:
            d_in.upload(bgr)
            d_counts.put(np.zeros(2, np.uint64))
            used = batch.embed_bgr_device(d_in.addr, d_out.addr, d_ref.addr, Planes(f, h, w, 0, grp, gfp), delta, n, d_bits.addr,
                                          bit_offset, len(bits), mode=mode, in_pitches=(irp, ifp), out_pitches=(orp, ofp),
                                          keep_colour=keep, readback=readback, d_counts=d_counts.addr if readback else 0)
            out = d_out.download().reshape(bgr.shape)
            ref = d_ref.download().reshape(f, h, w)
            counts = tuple(int(c) for c in d_counts.get(dtype=np.uint64))
            if pitches:
                for d in (d_in, d_out, d_ref):
                    d.check_sentinels()
                assert np.array_equal(d_in.download().reshape(bgr.shape), bgr)
            assert d_out.padding_after_rows() and d_ref.padding_after_rows()
    finally:
        if own_bits:
            d_bits.close()
    return out, ref, used, counts


def bgr_extract(bgr, delta, n, pitches=None):
    f, h, w, _ = bgr.shape
    rp, fp = pitches or (3 * w, 3 * w * h)
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    with SparseFrames(f, h, w, rp, fp, px=3) as d_in, DevBuf(nbytes + 64) as d_out:
        d_in.upload(bgr)
        d_out.memset(0xA5)
        got = batch.extract_bgr_device(d_in.addr, Planes.contiguous(f, h, w), delta, n, d_out.addr, nbytes, pitches=(rp, fp))
        out = d_out.get()
        if pitches:
            d_in.check_sentinels()
    assert got == cap and (out[nbytes:] == 0xA5).all()
    return np.unpackbits(out[:nbytes], count=cap)


def expect_bgr(bgr, stego_gray, keep):
    return keep_colour_rule(bgr, stego_gray, W15) if keep else np.repeat(stego_gray[..., None], 3, axis=-1)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep_colour"])
def test_colour_kernels_tile_maps(keep):
    """embed_bgr_kernel and extract_bgr_kernel (kEighth) at n = 3, thinned grid sizes"""
    for g in THIN_G:
        b = 256 * g - 5
        bgr = noise((1, 8, 8 * b, 3), 5000 + g)
        gray = bgr_gray(bgr)
        bits = synth.synthetic_bits(3 * b - 2, seed=g)
        want, want_used = orc.batch_embed(gray, 8, bits, 3)
        out, ref, used, _ = bgr_call(bgr, 8, 3, bits, "guarded", keep)
        assert used == want_used and np.array_equal(ref, gray)
        assert np.array_equal(out, expect_bgr(bgr, want, keep)), (g, np.argwhere(out != expect_bgr(bgr, want, keep))[:3])
        got = bgr_extract(out, 8, 3)
        assert np.array_equal(got, orc.batch_extract_bits(bgr_gray(out), 8, 3)), g


# ---- b. pixel offsets past 2^31 and 2^32 --------------------------------------------------------------------------------
FAR = (1 << 31) + (1 << 20) + 16
FAR_GEOMETRIES = {                     # name -> (frames, height, width, row pitch, frame pitch)
    "even": (*km.SHAPES["even"], km.SHAPES["even"][2], FAR),          # 16-byte pitches: two blocks per lane stay eligible
    "odd": (*km.SHAPES["odd"], km.SHAPES["odd"][2], FAR + 8),
    "rows": (1, 40, 200, (1 << 27) + 16, 40 * ((1 << 27) + 16)),     # rows from 16 on past 2 GiB, from 32 on past 4 GiB
}


def letterboxed(f, h, w, seed):
    """noise in [16, 240) between black bars one block row high: the reference's stego of a black block clips at 0 and does
    not read back, so the read-back pass repairs it"""
    frames = noise((f, h, w), seed, 16, 240)
    frames[:, :8] = 0
    frames[:, -8:] = 0
    return frames


def far_frames(geom, seed, kind="mixed"):
    f, h, w = FAR_GEOMETRIES[geom][:3]
    if kind == "letterbox":
        return letterboxed(f, h, w, seed)
    frames = noise((f, h, w), seed)
    frames[:, : h // 4, : w // 2] = 77                                    # flat blocks in every frame
    return frames


def far_embed(geom, frames, delta, n, bits, mode, in_place, key=None, coeffs=None, readback=False, bit_offset=0):
    """one embed call on SparseFrames of the geometry -> (stego frames, used, counts); sentinels and padding checked"""
    f, h, w, rp, fp = FAR_GEOMETRIES[geom]
    stream = np.concatenate([synth.synthetic_bits(bit_offset, seed=1), bits]) if bit_offset else bits
    with SparseFrames(f, h, w, rp, fp) as d_in, Payload(stream) as d_bits, DevBuf(16) as d_counts:
        d_in.upload(frames)
        d_out = d_in if in_place else SparseFrames(f, h, w, rp, fp, fill=0x3C)
        try:
            d_counts.put(np.zeros(2, np.uint64))
            used = batch.embed_device(d_in.addr, d_out.addr, Planes(f, h, w, 0, rp, fp), delta, n, d_bits.addr, bit_offset, len(bits),
                                      mode=mode, order=batch.block_order(key, T0) if key is not None else None, coeffs=coeffs,
                                      readback=readback, d_counts=d_counts.addr if readback else 0)
            out = d_out.download()
            d_out.check_sentinels()
            assert d_out.padding_after_rows()
            if not in_place:
                d_in.check_sentinels()
                assert np.array_equal(d_in.download(), frames)
            counts = tuple(int(c) for c in d_counts.get(dtype=np.uint64))
        finally:
            if not in_place:
                d_out.close()
    return out, used, counts


def far_extract(geom, frames, delta, n, mode, key=None, coeffs=None):
    f, h, w, rp, fp = FAR_GEOMETRIES[geom]
    cap = batch.capacity_bits(f, h, w, n)
    nbytes = (cap + 7) // 8
    with SparseFrames(f, h, w, rp, fp) as d_in, DevBuf(nbytes + 64) as d_out:
        d_in.upload(frames)
        d_out.memset(0xA5)
        got = batch.extract_device(d_in.addr, Planes(f, h, w, 0, rp, fp), delta, n, d_out.addr, nbytes, mode=mode,
                                   order=batch.block_order(key, T0) if key is not None else None, coeffs=coeffs)
        out = d_out.get()
        d_in.check_sentinels()
        assert np.array_equal(d_in.download(), frames)
    assert got == cap and (out[nbytes:] == 0xA5).all()
    return np.unpackbits(out[:nbytes], count=cap)


def budget_inside_a_block(geom, n):
    f, h, w = FAR_GEOMETRIES[geom][:3]
    cap = batch.capacity_bits(f, h, w, n)
    nb = cap - (cap // f) // 3 - 1                                        # inside the last frame
    return nb - 1 if n > 1 and nb % n == 0 else nb


def oracle_embed(frames, delta, n, bits, key=None):
    if key is None:
        return orc.batch_embed(frames, delta, bits, n)
    stego, used = orc.batch_embed(order.permute_blocks(frames, key, T0), delta, bits, n)
    return order.unpermute_blocks(stego, key, T0), used


def oracle_bits(frames, delta, n, key=None):
    return orc.batch_extract_bits(order.permute_blocks(frames, key, T0) if key is not None else frames, delta, n)


# (geometry, n, mode): row1 with one and with two blocks per lane, two rows, exact with one, two and eight coefficient rows;
# the single frame with far rows through the three kernel families
FAR_EMBEDS = [("odd", 3, "guarded"), ("even", 3, "guarded"), ("odd", 10, "guarded"), ("even", 3, "exact"), ("odd", 10, "exact"),
              ("even", 20, "exact"), ("rows", 3, "guarded"), ("rows", 10, "fast"), ("rows", 20, "guarded")]


@pytest.mark.parametrize("keyed", [False, True], ids=["raster", "keyed"])
@pytest.mark.parametrize("geom,n,mode", FAR_EMBEDS, ids=[f"{g}-n{n}-{m}" for g, n, m in FAR_EMBEDS])
def test_gray_embed_with_frames_gigabytes_apart(geom, n, mode, keyed):
    key = KEY if keyed else None
    frames = far_frames(geom, 10 + n)
    bits = synth.synthetic_bits(budget_inside_a_block(geom, n), seed=n)
    want, want_used = oracle_embed(frames, 8, n, bits, key)
    for in_place in (False, True):
        got, used, _ = far_embed(geom, frames, 8, n, bits, mode, in_place, key=key)
        assert used == want_used == bits.size
        assert np.array_equal(got, want), (in_place, np.argwhere(got != want)[:3])


@pytest.mark.parametrize("geom", ["odd", "rows"])
def test_readback_embed_with_frames_gigabytes_apart(geom):
    """svs_embed_readback_dev on letterboxed frames (the reference's stego fails to read back there), with counts"""
    frames = far_frames(geom, 21, "letterbox")
    n, delta = 3, 8
    bits = synth.synthetic_bits(budget_inside_a_block(geom, n), seed=5)
    ref, _ = orc.batch_embed(frames, delta, bits, n)
    want, want_counts, _ = host_readback(ref, delta, n, bits, bit_offset=0, n_bits=bits.size)
    assert want_counts[0] > 0, "no block is repaired: the pass's stores are not tested"
    for in_place in (False, True):
        got, used, counts = far_embed(geom, frames, delta, n, bits, "guarded", in_place, readback=True)
        assert used == bits.size and counts == tuple(want_counts), (counts, want_counts)
        assert np.array_equal(got, want), (in_place, np.argwhere(got != want)[:3])


@pytest.mark.parametrize("geom", ["even", "rows"])
def test_select_calls_with_frames_gigabytes_apart(geom):
    """svs_embed_select_dev and svs_extract_select_dev with the zig-zag scan of 10 coefficients"""
    index = csl.zigzag(10)
    frames = far_frames(geom, 31)
    bits = synth.synthetic_bits(budget_inside_a_block(geom, 10), seed=6)
    want, want_used = csl.select_batch_embed(frames, 8, bits, index)
    for in_place in (False, True):
        got, used, _ = far_embed(geom, frames, 8, 10, bits, "guarded", in_place, coeffs=index)
        assert used == want_used and np.array_equal(got, want), (in_place, np.argwhere(got != want)[:3])
    got = far_extract(geom, want, 8, 10, "guarded", coeffs=index)
    assert np.array_equal(got, csl.select_batch_extract(want, 8, index))


FAR_EXTRACTS = [("odd", 3, "fast", False), ("even", 10, "fast", False), ("odd", 20, "fast", False), ("even", 20, "exact", False),
                ("rows", 10, "fast", False), ("rows", 20, "exact", False), ("odd", 3, "guarded", True), ("even", 10, "fast", True),
                ("rows", 20, "fast", True)]


@pytest.mark.parametrize("geom,n,mode,keyed", FAR_EXTRACTS, ids=[f"{g}-n{n}-{m}" + ("-keyed" if k else "") for g, n, m, k in FAR_EXTRACTS])
def test_gray_extract_with_frames_gigabytes_apart(geom, n, mode, keyed):
    """svs_extract_dev (FAST and exact) and svs_extract_ordered_dev"""
    key = KEY if keyed else None
    frames = far_frames(geom, 40 + n)
    got = far_extract(geom, frames, 8, n, mode, key=key)
    want = oracle_bits(frames, 8, n, key)
    assert np.array_equal(got, want), int((got != want).sum())


def far_bgr_pitches(geom):
    f, h, w, rp, fp = FAR_GEOMETRIES[geom]
    if geom == "rows":
        big = (1 << 27) + 16
        return ((big + 8, h * (big + 8)), (big + 24, h * (big + 24)), (rp, fp))
    return ((3 * w, FAR + 24), (3 * w + 8, FAR + 40), (rp, fp))


FAR_BGR = [("odd", 3, "guarded", False), ("even", 10, "fast", True), ("odd", 20, "guarded", True), ("even", 3, "exact", False),
           ("rows", 3, "fast", True), ("rows", 10, "guarded", False)]


@pytest.mark.parametrize("geom,n,mode,keep", FAR_BGR, ids=[f"{g}-n{n}-{m}" + ("-keep" if k else "") for g, n, m, k in FAR_BGR])
def test_colour_embed_and_extract_with_frames_gigabytes_apart(geom, n, mode, keep):
    """svs_embed_bgr_dev (streaming and exact, plain and keep-colour) with large BGR pitches on input and output and a large
    gray-reference pitch; svs_extract_bgr_dev of the result from the far layout"""
    f, h, w = FAR_GEOMETRIES[geom][:3]
    bgr = noise((f, h, w, 3), 50 + n)
    bgr[:, : h // 4, : w // 2] = (10, 200, 90)
    gray = bgr_gray(bgr)
    bits = synth.synthetic_bits(budget_inside_a_block(geom, n), seed=7)
    want, want_used = orc.batch_embed(gray, 8, bits, n)
    out, ref, used, _ = bgr_call(bgr, 8, n, bits, mode, keep, pitches=far_bgr_pitches(geom))
    assert used == want_used and np.array_equal(ref, gray)
    assert np.array_equal(out, expect_bgr(bgr, want, keep)), np.argwhere(out != expect_bgr(bgr, want, keep))[:3]
    got = bgr_extract(out, 8, n, pitches=far_bgr_pitches(geom)[0])
    assert np.array_equal(got, orc.batch_extract_bits(bgr_gray(out), 8, n))


@pytest.mark.parametrize("geom,keep", [("odd", False), ("rows", True)])
def test_colour_readback_with_frames_gigabytes_apart(geom, keep):
    """svs_embed_bgr_readback_dev: the far call gives what the tight call gives, counts included, and repairs blocks"""
    f, h, w = FAR_GEOMETRIES[geom][:3]
    gray = far_frames(geom, 61, "letterbox")
    bgr = np.repeat(gray[..., None], 3, axis=-1)
    bits = synth.synthetic_bits(budget_inside_a_block(geom, 3), seed=8)
    tight = bgr_call(bgr, 8, 3, bits, "guarded", keep, readback=True)
    far = bgr_call(bgr, 8, 3, bits, "guarded", keep, readback=True, pitches=far_bgr_pitches(geom))
    assert tight[3][0] > 0, "no block is repaired: the pass's stores are not tested"
    assert far[2:] == tight[2:] and np.array_equal(far[0], tight[0]) and np.array_equal(far[1], tight[1])


@pytest.mark.parametrize("geom", ["even", "odd", "rows"])
def test_helper_kernels_with_frames_gigabytes_apart(geom):
    """svs_fill_synthetic_dev, svs_frame_sse_dev, svs_frame_ssim_dev (with the data-range pass), svs_bgr_to_gray_dev and
    svs_gray_to_bgr_dev on far layouts, against tests/helper_refs.py and svsdct/synth.py"""
    lib = native.load()
    f, h, w, rp, fp = FAR_GEOMETRIES[geom]
    planes = Planes(f, h, w, 0, rp, fp)
    brp, bfp = far_bgr_pitches(geom)[0]
    with SparseFrames(f, h, w, rp, fp) as d_a, SparseFrames(f, h, w, rp, fp) as d_b, SparseFrames(f, h, w, brp, bfp, px=3) as d_bgr, \
            DevBuf(8 * f) as d_sse, DevBuf(8 * f) as d_ssim, \
            DevBuf(int(lib.svs_ssim_workspace_bytes(C.byref(planes)))) as d_work:
        native.check(lib.svs_fill_synthetic_dev(d_a.ptr, C.byref(planes), 99, 4, 16, 224, None), "fill")
        a = d_a.download()
        assert np.array_equal(a, synth.synthetic_frames(f, h, w, seed=99, first_frame=4))
        b = far_frames(geom, 70)
        d_b.upload(b)
        native.check(lib.svs_frame_sse_dev(d_a.ptr, d_b.ptr, C.byref(planes), d_sse.ptr, None), "sse")
        assert np.array_equal(d_sse.get(dtype=np.uint64).astype(np.int64), refs.frame_sse(a, b))
        # data range NULL: the data-range pass takes max - min of each frame b and leaves it in the workspace behind the partials
        native.check(lib.svs_frame_ssim_dev(d_a.ptr, d_b.ptr, C.byref(planes), None, d_ssim.ptr, d_work.ptr, None), "ssim")
        got = d_ssim.get(dtype=np.float64)
        want = np.array([refs.ssim_exact(a[k], b[k]) for k in range(f)])
        # the bound tests/test_helper_kernels_gpu.py holds the kernel to against the same float64 restatement
        assert np.abs(got - want).max() <= 1e-12, (got, want)
        parts = d_work.nbytes // 8 - 2 * f
        assert np.array_equal(d_work.get(dtype=np.float64)[parts:parts + f], refs.frame_range(b))
        bgr = noise((f, h, w, 3), 71)
        d_bgr.upload(bgr)
        native.check(lib.svs_bgr_to_gray_dev(d_bgr.ptr, brp, bfp, d_a.ptr, C.byref(planes), None, None), "bgr_to_gray")
        assert np.array_equal(d_a.download(), bgr_gray(bgr))
        native.check(lib.svs_gray_to_bgr_dev(d_b.ptr, C.byref(planes), d_bgr.ptr, brp, bfp, None), "gray_to_bgr")
        assert np.array_equal(d_bgr.download().reshape(f, h, w, 3), refs.gray_to_bgr(b))
        for d in (d_a, d_b, d_bgr):
            d.check_sentinels()
            assert d.padding_after_rows()


# ---- c. payload positions past 2^32 ------------------------------------------------------------------------------------
FAR_BIT_OFFSETS = [(1 << 32) - 19, (1 << 32) + 37, (1 << 35) + 5]


class FarPayload(DevBuf):
    """a payload buffer of ceil((off + use) / 32) dwords of which only the window's bytes are written (8 bytes of junk on
    either side); the rest keeps what the allocation held"""

    def __init__(self, bits, bit_offset):
        end = bit_offset + len(bits)
        super().__init__(-(-end // 32) * 4)
        first = bit_offset // 8
        lead = np.random.default_rng(3).integers(0, 2, 64 + bit_offset % 8).astype(np.uint8)       # junk before the window
        tail = np.ones(((-end) % 8) + 64, np.uint8)                                                 # and behind it
        packed = np.packbits(np.concatenate([lead, np.asarray(bits, np.uint8), tail]))
        packed = packed[: min(packed.size, self.nbytes - (first - 8))]
        self.put(packed, first - 8)


# reader: (geometry of km.SHAPES, n, mode, keyed, entry)
READERS = {"row1_one_block": ("odd", 3, "guarded", False, "gray"), "row1_two_blocks": ("even", 3, "guarded", False, "gray"),
           "two_rows_guard_and_replay": ("odd", 10, "guarded", False, "gray"), "exact": ("even", 20, "exact", False, "gray"),
           "keyed_row1": ("even", 3, "guarded", True, "gray"), "keyed_two_rows": ("odd", 10, "fast", True, "gray"),
           "readback": ("odd", 3, "guarded", False, "readback"), "select": ("even", 10, "guarded", False, "select"),
           "colour": ("odd", 3, "guarded", False, "bgr"), "colour_readback": ("odd", 10, "fast", False, "bgr_readback")}


@pytest.mark.parametrize("bit_offset", FAR_BIT_OFFSETS, ids=["2^32-19", "2^32+37", "2^35+5"])
@pytest.mark.parametrize("reader", list(READERS))
def test_payload_read_at_bit_offsets_past_2_to_the_32(reader, bit_offset):
    shape, n, mode, keyed, entry = READERS[reader]
    f, h, w = km.SHAPES[shape]
    key = KEY if keyed else None
    letter = entry in ("readback", "bgr_readback")
    frames = letterboxed(f, h, w, 80) if letter else far_frames(shape, 80 + n)
    cap = batch.capacity_bits(f, h, w, n)
    nb = cap - (cap // f) // 3 - 1
    bits = synth.synthetic_bits(nb - 1 if nb % n == 0 else nb, seed=n)
    planes = Planes.contiguous(f, h, w)
    with FarPayload(bits, bit_offset) as d_bits:
        if entry in ("bgr", "bgr_readback"):
            bgr = np.repeat(frames[..., None], 3, axis=-1)
            out, _, used, counts = bgr_call(bgr, 8, n, bits, mode, False, readback=letter, bit_offset=bit_offset, d_bits=d_bits)
            near = bgr_call(bgr, 8, n, bits, mode, False, readback=letter)
            assert used == bits.size and (used, counts) == near[2:] and np.array_equal(out, near[0])
            if not letter:
                assert np.array_equal(out[..., 0], orc.batch_embed(frames, 8, bits, n)[0])
            return
        with DevBuf(frames.nbytes) as d_in, DevBuf(frames.nbytes) as d_out, DevBuf(16) as d_counts:
            d_in.put(frames)
            d_out.memset(0xC3)
            d_counts.put(np.zeros(2, np.uint64))
            used = batch.embed_device(d_in.addr, d_out.addr, planes, 8, n, d_bits.addr, bit_offset, bits.size, mode=mode,
                                      order=batch.block_order(key, T0) if keyed else None, readback=entry == "readback",
                                      d_counts=d_counts.addr if entry == "readback" else 0,
                                      coeffs=csl.zigzag(10) if entry == "select" else None)
            got = d_out.get().reshape(frames.shape)
            counts = tuple(int(c) for c in d_counts.get(dtype=np.uint64))
    assert used == bits.size
    if entry == "select":
        want = csl.select_batch_embed(frames, 8, bits, csl.zigzag(10))[0]
    elif entry == "readback":
        want, want_counts, _ = host_readback(orc.batch_embed(frames, 8, bits, n)[0], 8, n, bits, bit_offset=0, n_bits=bits.size)
        assert counts == tuple(want_counts) and counts[0] > 0
    else:
        want = oracle_embed(frames, 8, n, bits, key)[0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:3]


def test_payload_arguments_that_overflow_are_refused_before_any_launch():
    """bit_offset + n_bits past 2^64, and a payload of 2^32 dwords and more, are SVS_ERR_INVALID_ARG; the output is untouched"""
    lib = native.load()
    f, h, w = km.SHAPES["odd"]
    frames = far_frames("odd", 90)
    planes = Planes.contiguous(f, h, w)
    cap = batch.capacity_bits(f, h, w, 3)
    # the buffers hold the batch as BGR too, so that the colour call has the gray calls' capacity: no case passes its checks
    with DevBuf(3 * frames.nbytes) as d_in, DevBuf(3 * frames.nbytes) as d_out, DevBuf(64) as d_bits:
        d_in.put(np.repeat(frames[..., None], 3, axis=-1))
        d_out.memset(0x3C)
        done = C.c_uint64(77)
        for off, nb in (((1 << 64) - 8, 16), ((1 << 64) - 1, cap), (1 << 63, 1 << 63), (32 * ((1 << 32) - 1), cap), (1 << 37, cap),
                        ((1 << 37) - cap + 1, cap), ((1 << 64) - 1 - cap, cap)):
            assert off + min(nb, cap) >= 1 << 64 or -(-(off + min(nb, cap)) // 32) >= 1 << 32     # every case must be refused
            for flags in (0, native.SVS_EXACT_POCKETFFT, native.SVS_EXACT_GUARDED):
                rc = lib.svs_embed_dev(d_in.ptr, d_out.ptr, C.byref(planes), 8.0, 3, d_bits.ptr, off, nb, flags, C.byref(done), None)
                assert rc == native.SVS_ERR_INVALID_ARG, (off, nb, flags, rc)
            rc = lib.svs_embed_bgr_dev(d_in.ptr, 3 * w, 3 * w * h, d_out.ptr, 3 * w, 3 * w * h, None, C.byref(planes), None, 8.0, 3,
                                       d_bits.ptr, off, nb, 0, C.byref(done), None)
            assert rc == native.SVS_ERR_INVALID_ARG, (off, nb, rc)
        native.check(lib.svs_stream_synchronize(None), "sync")
        assert (d_out.get() == 0x3C).all()


# ---- d. extract output positions past 2^32 bits -------------------------------------------------------------------------
def test_extract_output_past_2_to_the_32_bits():
    """66 600 frames of 64 x 1024 at n = 63: 68.2 M blocks, 4.36 GB of pixels, 4.30 G bits - 1.3 M bits past 2^32.  Everything is
    device-resident: synthetic noise in [16, 240), synthetic bits, the exact embed at delta = 8, then the exact, the FAST
    (extract_kernel<8>), the select (the row-major coefficients backwards) and the keyed extract (of a select and of a keyed
    embed).  Frame 0, the frames that straddle stream bit 2^32 and the last frame are downloaded and compared with the oracle
    byte for byte, the matching slices of every extract output bit for bit.

    Bit errors against the payload (svs_bit_errors_dev): the oracle reads every bit of the sampled frames back, so zero is
    the condition there.  Over all 4.30 G bits the reference itself loses a bit now and then (a pixel clips or rounds across
    a quantiser cell; measured: 1 bit in the raster run).  The condition for the whole stream is therefore equality with the
    oracle: every frame in which the device counts an error (found by bisection with svs_bit_errors_dev over frame ranges, at
    most 16 of them) is downloaded, and its stego pixels and extracted bits must be the oracle's - so the device's count is
    the oracle's count on those frames, and 0 on every other frame.

    The streaming kernels (n <= 15) cannot reach 2^32 output bits under 16 GiB of pixels; what this test pins is the shared
    emit_wave_bits and or_bits_global, and (c) covers the reading side.  The colour extract is left out for the same reason."""
    lib = native.load()
    f, h, w, n, delta = 66600, 64, 1024, 63, 8
    planes = Planes.contiguous(f, h, w)
    bpf = (h // 8) * (w // 8)
    cap = f * bpf * n
    assert cap > 1 << 32
    nbytes = (cap + 7) // 8
    per_frame = bpf * n                                                  # bits; a multiple of 64: frames start on 8-byte boundaries
    fbytes = per_frame // 8
    straddle = (1 << 32) // per_frame
    sample = [0, straddle - 1, straddle, straddle + 1, f - 1]
    index = csl.reversed_list(63)
    with DevBuf(f * h * w) as d_px, DevBuf(nbytes + 8) as d_bits, DevBuf(nbytes + 64) as d_out, DevBuf(8) as d_err:
        native.check(lib.svs_fill_bits_dev(d_bits.ptr, cap, 7, 0, None), "fill_bits")

        def fill():
            native.check(lib.svs_fill_synthetic_dev(d_px.ptr, C.byref(planes), 7, 0, 16, 224, None), "fill")

        def cover(k):
            return synth.synthetic_frames(1, h, w, seed=7, first_frame=k)

        def payload(k):
            return np.unpackbits(d_bits.get(k * fbytes, fbytes))

        def errors(k0, k1):
            """differing bits of frames [k0, k1) between the extract output and the payload"""
            d_err.put(np.zeros(1, np.uint64))
            native.check(lib.svs_bit_errors_dev(C.c_void_p(d_out.addr + k0 * fbytes), C.c_void_p(d_bits.addr + k0 * fbytes),
                                                (k1 - k0) * per_frame, d_err.ptr, None), "bit_errors")
            return int(d_err.get(dtype=np.uint64)[0])

        def frames_with_errors(k0, k1, count):
            if count == 0:
                return []
            if k1 - k0 == 1:
                return [k0]
            mid = (k0 + k1) // 2
            left = errors(k0, mid)
            return frames_with_errors(k0, mid, left) + frames_with_errors(mid, k1, count - left)

        def check(label, reference, key=None, coeffs=None, mode="exact"):
            """reference(cover, payload, k) -> the oracle's (stego, extracted bits) of frame k"""
            d_out.memset(0xA5)
            got = batch.extract_device(d_px.addr, planes, delta, n, d_out.addr, nbytes, mode=mode,
                                       order=batch.block_order(key, 0) if key is not None else None, coeffs=coeffs)
            assert got == cap, label
            assert (d_out.get(nbytes, 64) == 0xA5).all(), label

            def frame_is_the_oracles(k):
                want, want_bits = reference(cover(k), payload(k), k)
                assert np.array_equal(d_px.get(k * h * w, h * w).reshape(1, h, w), want), (label, k)
                bits = np.unpackbits(d_out.get(k * fbytes, fbytes))
                assert np.array_equal(bits, want_bits), (label, k, int((bits != want_bits).sum()))
                return int((want_bits != payload(k)).sum())

            for k in sample:
                assert frame_is_the_oracles(k) == 0, "the oracle itself loses bits on a sampled frame"
            total = errors(0, f)
            assert total <= 16, (label, total)
            bad = frames_with_errors(0, f, total)
            assert sum(frame_is_the_oracles(k) for k in bad) == total, (label, bad, total)

        def raster(c, p, k):
            want, _ = orc.batch_embed(c, delta, p, n)
            return want, orc.batch_extract_bits(want, delta, n)

        def selected(c, p, k):
            want, _ = csl.select_batch_embed(c, delta, p, index)
            return want, csl.select_batch_extract(want, delta, index)

        def keyed(c, p, k):
            want, _ = orc.batch_embed(order.permute_blocks(c, KEY, k), delta, p, n)
            return order.unpermute_blocks(want, KEY, k), orc.batch_extract_bits(want, delta, n)

        fill()
        assert np.array_equal(d_px.get((f - 1) * h * w, h * w).reshape(1, h, w), cover(f - 1))
        assert batch.embed_device(d_px.addr, d_px.addr, planes, delta, n, d_bits.addr, 0, cap, mode="exact") == cap
        check("exact", raster)
        check("fast", raster, mode="fast")
        fill()
        assert batch.embed_device(d_px.addr, d_px.addr, planes, delta, n, d_bits.addr, 0, cap, mode="exact", coeffs=index) == cap
        check("select", selected, coeffs=index)
        fill()
        assert batch.embed_device(d_px.addr, d_px.addr, planes, delta, n, d_bits.addr, 0, cap, mode="exact",
                                  order=batch.block_order(KEY, 0)) == cap
        check("keyed", keyed, key=KEY)
