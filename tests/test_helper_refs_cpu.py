"""CPU tier: the references of tests/helper_refs.py that the helper-kernel GPU tests compare against.

`ssim_exact` (exact integer window sums) must agree with oracle/metrics_oracle.ssim_skimage (skimage's float filters) to 1e-9,
NaN in exactly the same frames - in particular a flat frame b (data range 0) gives NaN in both, as in skimage."""
import numpy as np
import pytest

import helper_refs as hr
from oracle import metrics_oracle as mo
from svsdct import synth


def _frames():
    """(name, a, b): the content classes where float window sums and exact ones could part ways"""
    rng = np.random.default_rng(41)
    h, w = 64, 72
    yy, xx = np.mgrid[0:h, 0:w]
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    grad = ((3 * xx + 2 * yy) % 256).astype(np.uint8)
    sat = np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)
    out = [("noise", noise, rng.integers(0, 256, (h, w), dtype=np.uint8)),
           ("noise-self", noise, noise.copy()),
           ("gradient", grad, np.clip(grad.astype(int) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)),
           ("saturated", sat, 255 - sat),
           ("saturated-half", sat, np.where(xx < w // 2, sat, 0).astype(np.uint8))]
    for level in (16, 200):
        for rng_w in (1, 2, 3):
            a = (level + rng.integers(0, rng_w + 1, (h, w))).astype(np.uint8)
            b = (level + rng.integers(0, rng_w + 1, (h, w))).astype(np.uint8)
            b[0, 0], b[-1, -1] = level, level + rng_w                      # range exactly rng_w
            out.append((f"near-flat-{level}-{rng_w}", a, b))
    for g in (0, 1, 128, 255):
        flat = np.full((h, w), g, np.uint8)
        out += [(f"flat-{g}-same", flat, flat.copy()),
                (f"flat-{g}-vs-noise", noise, flat),
                (f"flat-{g}-vs-flat", np.full((h, w), (g + 77) % 256, np.uint8), flat),
                (f"noise-vs-flat-{g}", flat, noise)]
    return out


@pytest.mark.parametrize("name,a,b", _frames(), ids=[c[0] for c in _frames()])
@pytest.mark.parametrize("data_range", [None, 255.0, 1.0])
def test_ssim_exact_equals_the_skimage_restatement(name, a, b, data_range):
    with np.errstate(invalid="ignore"):                   # skimage's 0 / 0
        got, want = hr.ssim_exact(a, b, data_range), mo.ssim_skimage(a, b, data_range)
    assert np.isnan(got) == np.isnan(want), (name, got, want)
    if not np.isnan(want):
        assert abs(got - want) <= 1e-9, (name, got, want)


def test_flat_frame_b_gives_nan_as_in_skimage():
    """data range 0 (flat b, the reference's max - min quirk): C1 = C2 = 0 and every window of b has variance exactly 0"""
    for g in (0, 1, 128, 255):
        flat = np.full((16, 24), g, np.uint8)
        with np.errstate(invalid="ignore"):
            assert np.isnan(hr.ssim_exact(flat, flat)) and np.isnan(mo.ssim_skimage(flat, flat))
    # a given data range keeps a flat pair finite: identical frames are 1 exactly
    assert hr.ssim_exact(flat, flat, 255.0) == 1.0


def test_window_sums_equal_brute_force():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, (2, 11, 13))
    got = hr.window_sums(x)
    want = np.array([[[x[f, i:i + 7, j:j + 7].sum() for j in range(7)] for i in range(5)] for f in range(2)])
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_exact_counters_and_conversions():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (3, 8, 16), dtype=np.uint8)
    b = rng.integers(0, 256, (3, 8, 16), dtype=np.uint8)
    assert hr.frame_sse(a, b).tolist() == [sum((int(x) - int(y)) ** 2 for x, y in zip(a[k].ravel(), b[k].ravel()))
                                           for k in range(3)]
    assert hr.frame_range(b).tolist() == [float(int(b[k].max()) - int(b[k].min())) for k in range(3)]
    pa, pb = np.packbits(a.ravel() & 1), np.packbits(b.ravel() & 1)
    for n in (0, 1, 7, 8, 9, 100, 384):
        assert hr.bit_errors(pa, pb, n) == int(((a.ravel() & 1)[:n] != (b.ravel() & 1)[:n]).sum())
    import config_and_setup as cs
    bgr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    assert np.array_equal(hr.bgr_to_gray(bgr), cs._bgr_to_gray(bgr))
    for table in (hr.OPENCV_15, hr.OPENCV_14, (21845, 21846, 21845, 16), (0, 0, 2, 1)):
        g = rng.integers(0, 256, (8, 8), dtype=np.uint8)
        assert np.array_equal(hr.bgr_to_gray(hr.gray_to_bgr(g), table), g)
    assert np.array_equal(hr.bgr_to_gray(bgr, (0, 0, 2, 1)), bgr[..., 2])


def test_pitched_round_trip():
    frames = synth.synthetic_frames(3, 8, 16, seed=1)
    fill = hr.sentinel_fill(3 * (8 * 24 + 8))
    buf = hr.to_pitched(frames, 24, 8 * 24 + 8, fill)
    assert np.array_equal(hr.from_pitched(buf, frames.shape, 24, 8 * 24 + 8), frames)
    assert np.count_nonzero(buf != fill) <= frames.size
