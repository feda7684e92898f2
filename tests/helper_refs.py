"""Plain NumPy references for the helper kernels (SSIM and its data range, SSE, bit errors, the synthetic fills, the colour
conversions), exact wherever the operation is exact, plus the pitched-buffer plumbing the GPU tests share.

TEST INFRASTRUCTURE ONLY.  tests/test_helper_refs_cpu.py pins `ssim_exact` to oracle/metrics_oracle.ssim_skimage;
tests/test_helper_kernels_gpu.py compares the kernels with these functions."""
from __future__ import annotations

import numpy as np

WIN = 7
NP = WIN * WIN
OPENCV_15 = (3735, 19235, 9798, 15)      # OpenCV 4's BGR2GRAY table (svs_bgr_to_gray_dev's default)
OPENCV_14 = (1868, 9617, 4899, 14)       # older OpenCV builds


def window_sums(x: np.ndarray) -> np.ndarray:
    """int64 sums of every 7x7 window lying wholly inside the last two axes (2-D cumulative sums): [..., H-6, W-6]"""
    x = np.asarray(x, np.int64)
    c = np.zeros(x.shape[:-2] + (x.shape[-2] + 1, x.shape[-1] + 1), np.int64)
    c[..., 1:, 1:] = x.cumsum(-2).cumsum(-1)
    return c[..., WIN:, WIN:] - c[..., :-WIN, WIN:] - c[..., WIN:, :-WIN] + c[..., :-WIN, :-WIN]


def ssim_map_exact(a: np.ndarray, b: np.ndarray, data_range=None) -> np.ndarray:
    """skimage's SSIM map (7x7 uniform window, K1 .01, K2 .03, sample covariance, float64) over the (H-6) x (W-6) windows
    inside a 2-D frame, from exact integer window sums: means sum / 49, variances (49 sum(xx) - sum(x)^2) / (49 * 48).
    A flat window has variance exactly 0, so with a data range of 0 its value is 0 / 0 = NaN, as in skimage."""
    if data_range is None:
        data_range = float(b.max()) - float(b.min())          # the reference's choice (evaluation.py:26)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    sa, sb, saa, sbb, sab = (window_sums(x) for x in (a, b, a * a, b * b, a * b))
    ux, uy = sa / float(NP), sb / float(NP)
    d = float(NP * (NP - 1))
    vx, vy, vxy = (NP * saa - sa * sa) / d, (NP * sbb - sb * sb) / d, (NP * sab - sa * sb) / d
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_exact(a: np.ndarray, b: np.ndarray, data_range=None) -> float:
    """mean of ssim_map_exact: NaN when any window is NaN"""
    return float(ssim_map_exact(a, b, data_range).mean(dtype=np.float64))


def frame_sse(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """per-frame sum of squared differences of [F, H, W] uint8 frames, exact (int64)"""
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).reshape(len(a), -1).sum(1)


def frame_range(b: np.ndarray) -> np.ndarray:
    """per-frame max - min of [F, H, W] frames (float64)"""
    flat = b.reshape(len(b), -1)
    return flat.max(1).astype(np.float64) - flat.min(1).astype(np.float64)


def bit_errors(a_packed: np.ndarray, b_packed: np.ndarray, n_bits: int) -> int:
    """differing bits among the first n_bits of two MSB-first packed streams"""
    a = np.unpackbits(np.asarray(a_packed, np.uint8), count=n_bits)
    b = np.unpackbits(np.asarray(b_packed, np.uint8), count=n_bits)
    return int(np.count_nonzero(a != b))


def bgr_to_gray(bgr: np.ndarray, weights=OPENCV_15) -> np.ndarray:
    """OpenCV's fixed-point BGR2GRAY: (B*wb + G*wg + R*wr + 2^(s-1)) >> s, in int64"""
    wb, wg, wr, s = (int(w) for w in weights)
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    return ((b * wb + g * wg + r * wr + (1 << (s - 1))) >> s).astype(np.uint8)


def gray_to_bgr(gray: np.ndarray) -> np.ndarray:
    return np.repeat(gray[..., None], 3, axis=-1)


# ---- pitched buffers -----------------------------------------------------------------------------
def sentinel_fill(nbytes: int, values=(0, 255)) -> np.ndarray:
    """a buffer whose bytes alternate between the sentinel values, so that reading them moves both a sum and a min / max"""
    return np.resize(np.asarray(values, np.uint8), nbytes)


def to_pitched(frames: np.ndarray, row_pitch: int, frame_pitch: int, fill: np.ndarray) -> np.ndarray:
    """frames [F, H, R] (R bytes per row) written into a copy of `fill` at the given byte pitches"""
    out = np.array(fill, np.uint8, copy=True)
    f, h, r = frames.shape[0], frames.shape[1], int(np.prod(frames.shape[2:]))
    for k in range(f):
        out[k * frame_pitch:k * frame_pitch + h * row_pitch].reshape(h, row_pitch)[:, :r] = frames[k].reshape(h, r)
    return out


def from_pitched(buf: np.ndarray, shape, row_pitch: int, frame_pitch: int) -> np.ndarray:
    """the [F, H, ...] frames of a pitched byte buffer"""
    f, h = shape[0], shape[1]
    r = int(np.prod(shape[2:]))
    return np.stack([buf[k * frame_pitch:k * frame_pitch + h * row_pitch].reshape(h, row_pitch)[:, :r]
                     for k in range(f)]).reshape(shape)
