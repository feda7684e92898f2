"""Per-coefficient QIM steps (include/svsdct.h, svs_stepped_embed* / svs_stepped_extract*): a table of 64 steps, one per flat
row-major coefficient, in place of a call's single delta.  matched() restates svs_matched_steps in integers - the same values
for every argument - so that a table matched to a codec's quantiser (svsdct/channel.py) needs no GPU; the stepped calls
themselves run on the GPU (svsdct/batch.py, steps=).  Both sides of a link must hold the same table.  The host model of the
stepped quantiser, built from the CPU oracle, lives with the tests (tests/stepped_lib.py)."""
from __future__ import annotations

import os
import re

import numpy as np

from . import channel
from .native import QimSteps

STEP_MAX = 4095


def as_table(table) -> np.ndarray:
    """64 integer steps, flat row-major -> uint16 [64]; entries 1..63 are checked to lie in 1..4095, entry 0 (DC) is not read
    and is stored as given when it fits, else as 0"""
    t = np.asarray(table)
    if t.size != 64 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("a QIM step table has 64 integer entries (flat row-major, entry 0 is DC and is not read)")
    t = t.reshape(64).astype(np.int64)
    bad = np.flatnonzero((t[1:] < 1) | (t[1:] > STEP_MAX))
    if bad.size:
        k = int(bad[0]) + 1
        raise ValueError(f"delta[{k}] = {int(t[k])} is not in 1..{STEP_MAX}")
    if not 0 <= t[0] <= 0xFFFF:
        t[0] = 0
    return t.astype(np.uint16)


def uniform(delta) -> np.ndarray:
    """every step = delta, an integer in 1..4095: the table whose stepped calls give the bytes of the calls with that delta"""
    if isinstance(delta, bool) or int(delta) != delta or not 1 <= int(delta) <= STEP_MAX:
        raise ValueError(f"a uniform step {delta!r} is not an integer in 1..{STEP_MAX}")
    t = np.full(64, int(delta), np.uint16)
    t[0] = 0
    return t


def matched(codec_steps_or_quality, multiple: int = 2, floor: int = 0) -> np.ndarray:
    """delta[k] = step[k] * max(multiple, ceil(floor / step[k])) for k = 1..63, delta[0] = 0 - svs_matched_steps, in integers.
    codec_steps_or_quality: a quality 1..100 (channel.quality_steps) or a codec table of 64 steps in 1..255.  multiple 1..16,
    floor 0..4095; ValueError for a result above 4095.  A lattice point of such a table is a fixed point of the requantiser of
    that codec table; the floor keeps every step above the embed's own truncation disturbance (up to 4.0)."""
    for name, v, lo, hi in (("multiple", multiple, 1, 16), ("floor", floor, 0, STEP_MAX)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} {v!r} is not an integer in {lo}..{hi}")
    s = channel.as_steps(codec_steps_or_quality).astype(np.int64)
    t = s * np.maximum(int(multiple), -(-int(floor) // s))
    t[0] = 0
    if t.max() > STEP_MAX:
        k = int(np.flatnonzero(t > STEP_MAX)[0])
        raise ValueError(f"delta[{k}] = {int(t[k])} exceeds {STEP_MAX}")
    return t.astype(np.uint16)


def steps_struct(table) -> QimSteps:
    """struct svs_qim_steps of a table (as_table)"""
    return QimSteps((QimSteps._fields_[0][1])(*(int(v) for v in as_table(table))))


_SPEC = re.compile(r"q(\d+)x(\d+)(?:f(\d+))?\Z")


def parse(spec: str) -> np.ndarray:
    """`q<quality>x<multiple>` with an optional `f<floor>` (q75x2, q95x2f16: matched()), or 64 comma-separated integers"""
    spec = spec.strip()
    m = _SPEC.match(spec)
    if m:
        return matched(int(m.group(1)), int(m.group(2)), int(m.group(3) or 0))
    try:
        values = [int(v) for v in spec.split(",")]
    except ValueError:
        raise ValueError(f"SVS_STEPS {spec!r} is neither q<quality>x<multiple>[f<floor>] nor 64 comma-separated integers") from None
    return as_table(np.array(values, np.int64))


def from_env(environ=None) -> np.ndarray | None:
    """the table SVS_STEPS names (parse), None when the variable is unset or empty"""
    spec = (os.environ if environ is None else environ).get("SVS_STEPS", "")
    return parse(spec) if spec.strip() else None
