"""Payload coefficient selection (include/svsdct.h, svs_coeffs).

Without a selection the payload of a block goes into flat row-major coefficients 1..n of its 8x8 DCT, the reference's rule: at
n = 3 only the horizontal frequencies (0,1), (0,2), (0,3) carry bits.  A selection is an ordered list of distinct flat
row-major indices in 1..63 (index 8*u + v: vertical frequency u, horizontal v; DC is never selectable): stream bit i of a block
goes to coefficient index[i].  Sender and receiver must agree on it.  A selection that is the prefix 1..n is the call without
one; any other runs the lane-per-block exact kernels, has no colour form, and is read back and repaired by readback_keyed (svs_embed_dithered_readback*).
"""
from __future__ import annotations

import os

import numpy as np

from . import native

MAX_COUNT = 63

# JPEG zig-zag scan as flat row-major indices; position 0 is DC (svs_coeffs_scan of the library holds the same table)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)


def check(indices) -> tuple:
    """-> the selection as a tuple of ints; ValueError unless they are distinct, in 1..63 and at most 63"""
    if isinstance(indices, (str, bytes)):
        raise TypeError("a selection is a sequence of integers (use selection() for a spec string)")
    out = []
    for k in indices:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"coefficient index must be an integer, not {type(k).__name__}")
        out.append(int(k))
    if len(out) > MAX_COUNT:
        raise ValueError(f"a selection holds at most {MAX_COUNT} coefficients, not {len(out)}")
    for k in out:
        if not 1 <= k <= 63:
            raise ValueError(f"coefficient index {k} outside 1 .. 63 (DC is never selectable)")
    if len(set(out)) != len(out):
        raise ValueError("coefficient indices must be distinct")
    return tuple(out)


def scan(name: str, first: int, count: int) -> tuple:
    """scan positions first .. first + count - 1 of "rowmajor" or "zigzag" (first >= 1, first + count <= 64)"""
    first, count = int(first), int(count)
    if name not in ("rowmajor", "zigzag"):
        raise ValueError(f"unknown scan {name!r} (rowmajor, zigzag)")
    if first < 1 or count < 0 or first + count > 64:
        raise ValueError(f"scan positions {first} .. {first + count - 1} are not inside 1 .. 63")
    table = ZIGZAG if name == "zigzag" else tuple(range(64))
    return tuple(table[first:first + count])


def selection(spec, n) -> tuple | None:
    """The selection of a call with n_ac = n (clamped to 0..63 as everywhere): None -> None (no selection); "rowmajor" ->
    1..n; "zigzag" -> the first n zig-zag positions after DC; "zigzag:<first>" -> n positions from scan position <first>
    (a mid-band start); "rowmajor:<first>" likewise; an explicit sequence of indices -> itself, and must have len == n."""
    if spec is None:
        return None
    n = max(0, min(int(n), MAX_COUNT))
    if isinstance(spec, str):
        name, _, first = spec.strip().partition(":")
        try:
            first = int(first) if first else 1
        except ValueError:
            raise ValueError(f"bad coefficient spec {spec!r}: <scan>[:<first position>]") from None
        return scan(name.strip(), first, n)
    sel = check(spec)
    if len(sel) != n:
        raise ValueError(f"the selection lists {len(sel)} coefficients but n_ac is {n}")
    return sel


def from_env(n, environ=None) -> tuple | None:
    """SVS_COEFFS of the drop-in embed / extract loops: unset (or empty) -> None, the reference's row-major prefix; a scan
    spec ("zigzag", "zigzag:6", "rowmajor") or a comma-separated list of indices ("9,2,17"), resolved with n_ac = n."""
    value = (os.environ if environ is None else environ).get("SVS_COEFFS")
    if value is None or value.strip() == "":
        return None
    value = value.strip()
    if value[0].isdigit():
        try:
            return selection([int(v.strip(), 0) for v in value.split(",")], n)
        except ValueError as exc:
            raise ValueError(f"SVS_COEFFS={value!r}: {exc}") from None
    return selection(value, n)


def is_prefix(sel) -> bool:
    return tuple(sel) == tuple(range(1, len(sel) + 1))


def native_coeffs(sel) -> native.Coeffs:
    """the C ABI's svs_coeffs of a checked selection"""
    sel = check(sel)
    c = native.Coeffs()
    c.count = len(sel)
    for i, k in enumerate(sel):
        c.index[i] = k
    return c


def gather(bits63: np.ndarray, sel) -> np.ndarray:
    """The gather identity: from the n_ac = 63 bit stream of some frames (0/1 array, 63 bits per block) the stream a selected
    extraction of the same frames gives - each block's bits taken at index[i] - 1."""
    sel = check(sel)
    b = np.asarray(bits63).reshape(-1, 63)
    return b[:, [k - 1 for k in sel]].reshape(-1)
