"""The step tables of the requantisation channel (include/svsdct.h, svs_requantise*): what the luminance path of an 8x8 intra
codec does to gray planes.  This module restates svs_quality_steps in integers - the same 64 values for every quality - and
builds the C struct; the channel itself runs on the GPU (svsdct/batch.py requantise_frames / requantise_device).  Its host
model, built from the CPU oracle, lives with the tests (tests/channel_lib.py)."""
from __future__ import annotations

import numpy as np

from .native import Steps

# ITU-T T.81 Annex K, table K.1 (luminance), natural row-major order: entry 8 u + v is vertical frequency u, horizontal v
ANNEX_K_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61,
                         12, 12, 14, 19, 26, 58, 60, 55,
                         14, 13, 16, 24, 40, 57, 69, 56,
                         14, 17, 22, 29, 51, 87, 80, 62,
                         18, 22, 37, 56, 68, 109, 103, 77,
                         24, 35, 55, 64, 81, 104, 113, 92,
                         49, 64, 78, 87, 103, 121, 120, 101,
                         72, 92, 95, 98, 112, 100, 103, 99], np.uint16)
ANNEX_K_LUMA.setflags(write=False)


def quality_steps(quality) -> np.ndarray:
    """The Annex K luminance table scaled as the IJG library scales it, uint16 [64]: s = 5000 // quality below 50, else
    200 - 2 * quality; step = clamp((base * s + 50) // 100, 1, 255).  quality 50 is the table itself, 100 all ones.
    ValueError outside 1..100."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality {quality!r} is not an integer in 1..100")
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((ANNEX_K_LUMA.astype(np.int64) * s + 50) // 100, 1, 255).astype(np.uint16)


def as_steps(steps_or_quality) -> np.ndarray:
    """A quality (an integer 1..100) or a table of 64 steps -> uint16 [64], every entry checked to lie in 1..255."""
    if np.ndim(steps_or_quality) == 0:
        return quality_steps(steps_or_quality)
    steps = np.asarray(steps_or_quality)
    if steps.size != 64 or not np.issubdtype(steps.dtype, np.integer):
        raise ValueError("a step table has 64 integer entries (flat row-major, entry 0 is DC)")
    steps = steps.reshape(64)
    if steps.min() < 1 or steps.max() > 255:
        k = int(np.flatnonzero((steps < 1) | (steps > 255))[0])
        raise ValueError(f"step[{k}] = {int(steps[k])} is not in 1..255")
    return steps.astype(np.uint16)


def steps_struct(steps_or_quality) -> Steps:
    """struct svs_steps of a quality or a table (as_steps)"""
    return Steps((Steps._fields_[0][1])(*(int(v) for v in as_steps(steps_or_quality))))
