"""GPU tier (-m gpu): the helper kernels - SSIM and its data range, SSE, bit errors, the synthetic fills and the colour
conversions - against the plain NumPy references of tests/helper_refs.py, at the shapes, counters and layouts where they
could go wrong: both sides of every tile / band / row-group edge, pitched planes whose padding holds sentinels that would
change the result if read, counters past 2^32, and the argument checks that keep misaligned rows away from the kernels."""
import ctypes as C

import numpy as np
import pytest

import helper_refs as hr
from oracle import metrics_oracle as mo
from svsdct import native, synth
from svsdct.native import Planes
from test_gpu_parity import _Dev

pytestmark = pytest.mark.gpu
U32 = 2 ** 32


@pytest.fixture(scope="module", autouse=True)
def _device():
    native.ensure_device(0)


def _at(d, offset):
    return C.c_void_p(d.ptr.value + offset)


def _pitched_dev(frames, row_pitch, frame_pitch, values=(0, 255)):
    """a device buffer holding `frames` [F, H, W] at the given pitches, every other byte a sentinel; -> (_Dev, host copy)"""
    host = hr.to_pitched(frames, row_pitch, frame_pitch, hr.sentinel_fill(len(frames) * frame_pitch, values))
    d = _Dev(host.nbytes)
    d.put(host)
    return d, host


def _padding_mask(f, h, row_bytes, row_pitch, frame_pitch):
    mask = np.ones(f * frame_pitch, bool)
    for k in range(f):
        for y in range(h):
            mask[k * frame_pitch + y * row_pitch:k * frame_pitch + y * row_pitch + row_bytes] = False
    return mask


# ---- SSIM and the data range -----------------------------------------------------------------------
def _ssim_dev(d_a, d_b, planes, ranges=None):
    """-> (ssim[F], the per-frame data range the call used when `ranges` is None)"""
    lib = native.load()
    f = planes.n_frames
    work, out = _Dev(int(lib.svs_ssim_workspace_bytes(C.byref(planes)))), _Dev(8 * f)
    d_r = None
    if ranges is not None:
        d_r = _Dev(8 * f)
        d_r.put(np.asarray(ranges, np.float64))
    native.check(lib.svs_frame_ssim_dev(d_a.ptr, d_b.ptr, C.byref(planes), d_r.ptr if d_r else None, out.ptr, work.ptr,
                                        None), "svs_frame_ssim_dev")
    ssim = out.get(dtype=np.float64)
    # workspace: the partials, then the per-frame data range (svs_frame_ssim_dev)
    parts = work.nbytes // 8 - 2 * f
    return ssim, (work.get(dtype=np.float64)[parts:parts + f] if ranges is None else None)


def _check_ssim(got, a, b, ranges, what):
    for k in range(len(a)):
        r = None if ranges is None else float(ranges[k])
        with np.errstate(invalid="ignore"):               # skimage's 0 / 0
            exact, sk = hr.ssim_exact(a[k], b[k], r), mo.ssim_skimage(a[k], b[k], r)
        assert np.isnan(got[k]) == np.isnan(exact) == np.isnan(sk), (what, k, got[k], exact, sk)
        if not np.isnan(exact):
            assert abs(got[k] - exact) <= 1e-12, (what, k, got[k], exact, got[k] - exact)
            assert abs(got[k] - sk) <= 1e-9, (what, k, got[k], sk)


def _ssim_pair(f, h, w, seed):
    """a: mixed content; b: a plus noise inside [10, 245], then each frame's only extreme - a 0 or a 255 - in its first
    pixel, its last row or its last column"""
    rng = np.random.default_rng(seed)
    a = synth.synthetic_frames(f, h, w, seed=seed, lo=0, span=256)
    yy, xx = np.mgrid[0:h, 0:w]
    a[1::3] = ((2 * xx + 3 * yy) % 256).astype(np.uint8)
    a[2::3, : h // 2] = 90
    b = np.clip(a.astype(int) + rng.integers(-12, 13, a.shape), 10, 245).astype(np.uint8)
    for k in range(f):
        y, x = [(0, 0), (h - 1, int(rng.integers(w))), (int(rng.integers(h)), w - 1)][(k + seed) % 3]
        b[k, y, x] = 255 * ((k + seed // 3) % 2)
    return a, b


@pytest.mark.parametrize("h", [8, 128, 136, 256, 264])
@pytest.mark.parametrize("w", [8, 256, 264, 512, 520])
def test_ssim_and_data_range_at_tile_band_and_row_group_edges(h, w):
    """output width W-6 on both sides of the 256-column tiles, output height H-6 on both sides of the 126-row bands and the
    16-row min / max groups; contiguous and pitched planes (padding and frame gaps hold 0 / 255 sentinels); the data range
    per frame (1, 255, 1000) and the reference's max(b) - min(b)"""
    f = 2 + (h + w) % 2
    a, b = _ssim_pair(f, h, w, seed=h * 1000 + w)
    for rp, fp in ((w, h * w), (w + 8 * (1 + h % 3), (w + 8 * (1 + h % 3)) * h + 24)):
        planes = Planes(f, h, w, 0, rp, fp)
        d_a, _ = _pitched_dev(a, rp, fp, (0, 255))
        d_b, _ = _pitched_dev(b, rp, fp, (255, 0))
        ssim, used = _ssim_dev(d_a, d_b, planes)
        assert np.array_equal(used, hr.frame_range(b)), (rp, used)
        _check_ssim(ssim, a, b, None, (rp, "max - min"))
        ranges = np.resize([1.0, 255.0, 1000.0], f)[::-1 if h % 16 else 1]
        ssim, _ = _ssim_dev(d_a, d_b, planes, ranges)
        _check_ssim(ssim, a, b, ranges, (rp, "given"))


def test_ssim_many_frames_per_call_with_flat_frames():
    """>= 300 frames per call, flat b frames (data range 0: NaN where skimage has NaN, and only there) among them"""
    f, h, w = 320, 16, 24
    a, b = _ssim_pair(f, h, w, seed=3)
    for i, g in enumerate((0, 1, 128, 255)):
        b[7 + 50 * i] = g                               # against a: a window flat in b only -> 0, not NaN
        b[8 + 50 * i] = a[8 + 50 * i] = g               # identical flat frames -> NaN
        b[9 + 50 * i], a[9 + 50 * i] = g, (g + 77) % 256    # two different flat frames -> NaN
    rp, fp = w + 8, (w + 8) * h + 8
    planes = Planes(f, h, w, 0, rp, fp)
    d_a, _ = _pitched_dev(a, rp, fp, (0, 255))
    d_b, _ = _pitched_dev(b, rp, fp, (255, 0))
    ssim, used = _ssim_dev(d_a, d_b, planes)
    assert np.array_equal(used, hr.frame_range(b))
    _check_ssim(ssim, a, b, None, "many")
    assert np.isnan(ssim[[8, 9, 58, 59, 108, 109, 158, 159]]).all() and not np.isnan(ssim[[57, 157]]).any()
    ranges = np.resize([1.0, 255.0, 1000.0], f)
    _check_ssim(_ssim_dev(d_a, d_b, planes, ranges)[0], a, b, ranges, "many, given")


def test_ssim_flat_frames_give_skimage_nan():
    """a flat frame b at 0, 1, 128 and 255 with data_range = max - min = 0: against itself, against another flat frame
    and against noise, the kernel must give what skimage gives - NaN where its denominator is 0, finite elsewhere"""
    h, w = 64, 72
    noise = synth.synthetic_frames(1, h, w, seed=9, lo=0, span=256)[0]
    a, b = [], []
    for g in (0, 1, 128, 255):
        flat = np.full((h, w), g, np.uint8)
        for x, y in ((flat, flat), (np.full((h, w), (g + 77) % 256, np.uint8), flat), (noise, flat), (flat, noise)):
            a.append(x)
            b.append(y)
    a, b = np.stack(a), np.stack(b)
    planes = Planes.contiguous(len(a), h, w)
    d_a, d_b = _Dev(a.nbytes), _Dev(b.nbytes)
    d_a.put(a)
    d_b.put(b)
    ssim, _ = _ssim_dev(d_a, d_b, planes)
    _check_ssim(ssim, a, b, None, "flat")
    assert np.isnan(ssim[0::4]).all() and np.isnan(ssim[1::4]).all()
    _check_ssim(_ssim_dev(d_a, d_b, planes, np.full(len(a), 255.0))[0], a, b, np.full(len(a), 255.0), "flat, 255")


# ---- SSE ---------------------------------------------------------------------------------------------
def test_frame_sse_past_2_to_the_32():
    lib = native.load()
    f, h, w = 2, 2160, 3840
    planes = Planes.contiguous(f, h, w)
    d_a, d_b, d_sse = _Dev(f * h * w), _Dev(f * h * w), _Dev(8 * f)
    native.check(lib.svs_memset(d_a.ptr, 0, f * h * w, None), "memset")
    native.check(lib.svs_memset(d_b.ptr, 255, f * h * w, None), "memset")
    native.check(lib.svs_frame_sse_dev(d_a.ptr, d_b.ptr, C.byref(planes), d_sse.ptr, None), "sse")
    want = 255 ** 2 * h * w
    assert want > U32 and d_sse.get(dtype=np.uint64).tolist() == [want] * f


@pytest.mark.parametrize("f,h,w,rp,fp", [(1000, 8, 8, 8, 64), (1000, 8, 16, 16, 128), (1000, 8, 8, 16, 136),
                                         (3, 40, 72, 96, 96 * 40 + 64), (2, 264, 520, 536, 536 * 264 + 8)])
def test_frame_sse_many_frames_and_pitched(f, h, w, rp, fp):
    lib = native.load()
    a = synth.synthetic_frames(f, h, w, seed=w + f, lo=0, span=256)
    b = synth.synthetic_frames(f, h, w, seed=w + f + 1, lo=0, span=256)
    b[0] = a[0]
    d_a, _ = _pitched_dev(a, rp, fp, (0, 255))
    d_b, _ = _pitched_dev(b, rp, fp, (255, 0))
    d_sse = _Dev(8 * f)
    native.check(lib.svs_frame_sse_dev(d_a.ptr, d_b.ptr, C.byref(Planes(f, h, w, 0, rp, fp)), d_sse.ptr, None), "sse")
    assert np.array_equal(d_sse.get(dtype=np.uint64).astype(np.int64), hr.frame_sse(a, b))


# ---- bit errors ----------------------------------------------------------------------------------------
def test_bit_errors_lengths_and_tail_masks():
    """n_bits 0..70 and 2^k +- 1 up to 2^20; both streams carry random bits past n_bits, in the last byte and after it;
    every count slot starts stale (non-zero) - n_bits = 0 must overwrite it with 0"""
    lib = native.load()
    ns = sorted(set(range(0, 71)) | {2 ** k + d for k in range(3, 21) for d in (-1, 0, 1)})
    rng = np.random.default_rng(12)
    nbytes = (max(ns) + 7) // 8 + 64
    a, b = rng.integers(0, 256, nbytes, dtype=np.uint8), rng.integers(0, 256, nbytes, dtype=np.uint8)
    d_a, d_b, d_cnt = _Dev(nbytes), _Dev(nbytes), _Dev(8 * len(ns))
    d_a.put(a)
    d_b.put(b)
    d_cnt.put(np.full(len(ns), 0xDEADBEEF, np.uint64))
    for i, n in enumerate(ns):
        native.check(lib.svs_bit_errors_dev(d_a.ptr, d_b.ptr, n, _at(d_cnt, 8 * i), None), "bit_errors")
    got = d_cnt.get(dtype=np.uint64)
    want = [hr.bit_errors(a, b, n) for n in ns]
    assert got.tolist() == want


def test_bit_errors_count_past_2_to_the_32():
    """two 512 MiB streams, all zeros against all ones: the first n_bits = 2^32 + 13 differ, and so does every bit after"""
    lib = native.load()
    n = U32 + 13
    nbytes = (n + 7) // 8 + 6                   # 8-byte multiple; ones past n_bits in the last byte and after it
    d_a, d_b, d_cnt = _Dev(nbytes), _Dev(nbytes), _Dev(16)
    native.check(lib.svs_memset(d_a.ptr, 0x00, nbytes, None), "memset")
    native.check(lib.svs_memset(d_b.ptr, 0xFF, nbytes, None), "memset")
    native.check(lib.svs_memset(d_cnt.ptr, 0x5A, 16, None), "memset")
    native.check(lib.svs_bit_errors_dev(d_a.ptr, d_b.ptr, n, d_cnt.ptr, None), "bit_errors")
    native.check(lib.svs_bit_errors_dev(d_b.ptr, d_a.ptr, n - 18, _at(d_cnt, 8), None), "bit_errors")
    assert d_cnt.get(dtype=np.uint64).tolist() == [n, n - 18]


# ---- the synthetic fills ---------------------------------------------------------------------------------
def test_fill_bits_counters_past_2_to_the_32():
    """first_bit past 2^32 (sharded runs: 1200 x 8K at n = 63 is 3.9e10 bits), seeds 0 and 2^32 - 1: the stream equals
    synth.synthetic_bits, the bits after n_bits up to the dword boundary are 0, the bytes after it untouched"""
    lib = native.load()
    ns = (1, 31, 32, 33, 1_000_003)
    nbytes = ((max(ns) + 31) // 32) * 4 + 64
    sentinel = np.full(nbytes, 0xA5, np.uint8)
    d = _Dev(nbytes)
    for first in (0, 1000, U32 - 77, U32 + 5, 39_191_040_000):
        for n in ns:
            for seed in (0, U32 - 1):
                d.put(sentinel)
                native.check(lib.svs_fill_bits_dev(d.ptr, n, seed, first, None), "fill_bits")
                got = d.get()
                end = ((n + 31) // 32) * 4
                bits = np.unpackbits(got[:end])
                assert np.array_equal(bits[:n], synth.synthetic_bits(n, seed=seed, first_bit=first)), (first, n, seed)
                assert not bits[n:].any(), (first, n, seed)
                assert np.all(got[end:] == 0xA5), (first, n, seed)


@pytest.mark.parametrize("f,h,w,rp,fp", [(2, 2160, 3840, 3840, 3840 * 2160), (3, 40, 72, 88, 88 * 40 + 24),
                                         (5, 16, 8, 24, 24 * 16 + 8)])
def test_fill_synthetic_frames_counters_and_padding(f, h, w, rp, fp):
    """2 x 4K is more than one grid-stride sweep (4096 x 256 threads x 8 pixels); first_frame near 2^32 (the frame counter
    wraps inside the call), seeds 0 and 2^32 - 1, (lo, span) in {(0, 256), (16, 224), (100, 1)}; padding untouched"""
    lib = native.load()
    planes = Planes(f, h, w, 0, rp, fp)
    fill = hr.sentinel_fill(f * fp, (0x3C, 0xC3))
    mask = _padding_mask(f, h, w, rp, fp)
    d = _Dev(f * fp)
    combos = [(0, U32 - 2, 0, 256), (U32 - 1, U32 - 1, 16, 224), (U32 - 1, 7, 100, 1)]
    if h * w <= 4096:
        combos += [(s, ff, lo, span) for s in (0, U32 - 1) for ff in (0, U32 - 2) for lo, span in ((0, 256), (16, 224), (100, 1))]
    for seed, first, lo, span in combos:
        d.put(fill)
        native.check(lib.svs_fill_synthetic_dev(d.ptr, C.byref(planes), seed, first, lo, span, None), "fill_synthetic")
        got = d.get()
        want = synth.synthetic_frames(f, h, w, seed=seed, first_frame=first, lo=lo, span=span)
        assert np.array_equal(hr.from_pitched(got, (f, h, w), rp, fp), want), (seed, first, lo, span)
        assert np.array_equal(got[mask], fill[mask]), (seed, first, lo, span)


# ---- colour ----------------------------------------------------------------------------------------------
TABLES = (hr.OPENCV_15, hr.OPENCV_14, (21845, 21846, 21845, 16), (0, 0, 2, 1))


def _bgr_to_gray_dev(d_bgr, brp, bfp, d_gray, planes, table):
    wt = np.asarray(table, np.uint32)
    native.check(native.load().svs_bgr_to_gray_dev(d_bgr.ptr, brp, bfp, d_gray.ptr, C.byref(planes), wt.ctypes.data, None),
                 "svs_bgr_to_gray_dev")


def _gray_to_bgr_dev(d_gray, planes, d_bgr, brp, bfp):
    native.check(native.load().svs_gray_to_bgr_dev(d_gray.ptr, C.byref(planes), d_bgr.ptr, brp, bfp, None),
                 "svs_gray_to_bgr_dev")


def test_bgr_to_gray_every_colour_under_every_table():
    """one 4096 x 4096 frame holding every (B, G, R) triple once, in a shuffled order; gray -> BGR -> gray is the identity"""
    n = 4096
    idx = np.random.default_rng(0).permutation(1 << 24).astype(np.uint32)
    bgr = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(1, n, n, 3)
    planes = Planes.contiguous(1, n, n)
    d_bgr, d_gray, d_back = _Dev(bgr.nbytes), _Dev(n * n), _Dev(bgr.nbytes)
    d_bgr.put(bgr)
    for table in TABLES:
        _bgr_to_gray_dev(d_bgr, 3 * n, 3 * n * n, d_gray, planes, table)
        gray = d_gray.get().reshape(1, n, n)
        assert np.array_equal(gray, hr.bgr_to_gray(bgr, table)), table
        _gray_to_bgr_dev(d_gray, planes, d_back, 3 * n, 3 * n * n)
        assert np.array_equal(d_back.get().reshape(bgr.shape), hr.gray_to_bgr(gray)), table
        _bgr_to_gray_dev(d_back, 3 * n, 3 * n * n, d_gray, planes, table)
        assert np.array_equal(d_gray.get().reshape(1, n, n), gray), table


@pytest.mark.parametrize("f,h,w", [(33, 16, 8), (13, 24, 40), (5, 24, 200)])
def test_colour_conversions_pitched_with_sentinels(f, h, w):
    """8-byte pitches past the rows of both BGR and gray planes, frame gaps; 1, 5 and 25 blocks per row, so that a wave's 64
    blocks wrap across rows and frames, and 66, 195 and 375 blocks (no multiple of 64).  bgr -> gray writes the gray pixels
    only; gray -> bgr is checked byte for byte over the whole buffer, padding included"""
    brp, grp = 3 * w + 8 * (1 + w % 3), w + 8
    bfp, gfp = brp * h + 8, grp * h + 16
    planes = Planes(f, h, w, 0, grp, gfp)
    bgr = synth.synthetic_frames(f, h, 3 * w, seed=f, lo=0, span=256).reshape(f, h, w, 3)
    d_bgr, bgr_host = _pitched_dev(bgr, brp, bfp, (0, 255))
    gray_fill = hr.sentinel_fill(f * gfp, (0x11, 0xEE))
    d_gray = _Dev(f * gfp)
    gmask = _padding_mask(f, h, w, grp, gfp)
    bgr_fill = hr.sentinel_fill(f * bfp, (0x22, 0xDD))
    d_out = _Dev(f * bfp)
    for table in TABLES:
        d_gray.put(gray_fill)
        _bgr_to_gray_dev(d_bgr, brp, bfp, d_gray, planes, table)
        got = d_gray.get()
        want = hr.bgr_to_gray(bgr, table)
        assert np.array_equal(hr.from_pitched(got, (f, h, w), grp, gfp), want), table
        assert np.array_equal(got[gmask], gray_fill[gmask]), table
        d_out.put(bgr_fill)
        _gray_to_bgr_dev(d_gray, planes, d_out, brp, bfp)
        back = d_out.get()
        assert np.array_equal(back, hr.to_pitched(hr.gray_to_bgr(want), brp, bfp, bgr_fill)), table
        d_gray.put(gray_fill)
        _bgr_to_gray_dev(d_out, brp, bfp, d_gray, planes, table)
        assert np.array_equal(hr.from_pitched(d_gray.get(), (f, h, w), grp, gfp), want), table
    assert np.array_equal(d_bgr.get(), bgr_host)                   # the input is never written


# ---- argument checks -------------------------------------------------------------------------------------
def test_helper_refusals_launch_nothing():
    """every refusal returns SVS_ERR_INVALID_ARG before anything is launched: the output buffers keep their bytes"""
    lib = native.load()
    f, h, w = 2, 16, 16
    planes = Planes.contiguous(f, h, w)
    frames = synth.synthetic_frames(f, h, w, seed=1)
    d_bgr, d_gray, d_out = _Dev(3 * f * h * w + 64), _Dev(f * h * w + 64), _Dev(4096)
    d_bgr.put(np.zeros(d_bgr.nbytes, np.uint8))
    d_gray.put(np.resize(frames.ravel(), d_gray.nbytes))
    sentinel = np.full(4096, 0x77, np.uint8)
    bad_w = np.array([0xFFFFFFFF, 1, 2, 1], np.uint32)                 # sums to 2^1 modulo 2^32
    big_w = np.array([65537, 0, 0xFFFFFFFF, 16], np.uint32)
    rp, fp = 3 * w, 3 * w * h
    calls = {
        "bgr2gray row pitch 4 mod 8": lambda: lib.svs_bgr_to_gray_dev(d_bgr.ptr, rp + 4, (rp + 4) * h, d_out.ptr,
                                                                      C.byref(planes), None, None),
        "bgr2gray frame pitch 4 mod 8": lambda: lib.svs_bgr_to_gray_dev(d_bgr.ptr, rp, fp + 4, d_out.ptr, C.byref(planes),
                                                                        None, None),
        "bgr2gray BGR pointer 4 mod 8": lambda: lib.svs_bgr_to_gray_dev(_at(d_bgr, 4), rp, fp, d_out.ptr, C.byref(planes),
                                                                        None, None),
        "bgr2gray gray pointer 4 mod 8": lambda: lib.svs_bgr_to_gray_dev(d_bgr.ptr, rp, fp, _at(d_out, 4), C.byref(planes),
                                                                         None, None),
        "bgr2gray weights wrap": lambda: lib.svs_bgr_to_gray_dev(d_bgr.ptr, rp, fp, d_out.ptr, C.byref(planes),
                                                                 bad_w.ctypes.data, None),
        "bgr2gray weights wrap, 16 bits": lambda: lib.svs_bgr_to_gray_dev(d_bgr.ptr, rp, fp, d_out.ptr, C.byref(planes),
                                                                          big_w.ctypes.data, None),
        "gray2bgr row pitch 4 mod 8": lambda: lib.svs_gray_to_bgr_dev(d_gray.ptr, C.byref(planes), d_out.ptr, rp + 4,
                                                                      (rp + 4) * h, None),
        "gray2bgr frame pitch 4 mod 8": lambda: lib.svs_gray_to_bgr_dev(d_gray.ptr, C.byref(planes), d_out.ptr, rp, fp + 4,
                                                                        None),
        "gray2bgr BGR pointer 4 mod 8": lambda: lib.svs_gray_to_bgr_dev(d_gray.ptr, C.byref(planes), _at(d_out, 4), rp, fp,
                                                                        None),
        "extract_bgr weights wrap": lambda: lib.svs_extract_bgr_dev(d_bgr.ptr, rp, fp, C.byref(planes), bad_w.ctypes.data,
                                                                    8.0, 3, d_out.ptr, 4096, None, None),
        "embed_bgr weights wrap": lambda: lib.svs_embed_bgr_dev(d_bgr.ptr, rp, fp, d_out.ptr, rp, fp, None, C.byref(planes),
                                                                bad_w.ctypes.data, 8.0, 3, d_gray.ptr, 0, 8, 0, None, None),
        "fill_synthetic lo + span wraps": lambda: lib.svs_fill_synthetic_dev(d_out.ptr, C.byref(planes), 1, 0, 0xFFFFFFFF,
                                                                             2, None),
        "fill_synthetic span > 256": lambda: lib.svs_fill_synthetic_dev(d_out.ptr, C.byref(planes), 1, 0, 0, 257, None),
        "fill_synthetic lo + span > 256": lambda: lib.svs_fill_synthetic_dev(d_out.ptr, C.byref(planes), 1, 0, 200, 57,
                                                                             None),
    }
    work = _Dev(int(lib.svs_ssim_workspace_bytes(C.byref(planes))) + 64)
    d_r = _Dev(64)
    ssim_args = {"ssim a pointer 4 mod 8": (_at(d_gray, 4), d_gray.ptr, None),
                 "ssim b pointer 4 mod 8": (d_gray.ptr, _at(d_gray, 4), None),
                 "ssim data range pointer 4 mod 8": (d_gray.ptr, d_gray.ptr, _at(d_r, 4))}
    for name, (pa, pb, pr) in ssim_args.items():
        calls[name] = lambda pa=pa, pb=pb, pr=pr: lib.svs_frame_ssim_dev(pa, pb, C.byref(planes), pr, d_out.ptr, work.ptr,
                                                                         None)
    for name, call in calls.items():
        d_out.put(sentinel)
        assert call() == native.SVS_ERR_INVALID_ARG, name
        native.check(lib.svs_stream_synchronize(None), "sync")
        assert np.array_equal(d_out.get(), sentinel), name
