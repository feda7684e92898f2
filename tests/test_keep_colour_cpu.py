"""SVS_KEEP_COLOUR, CPU tier: the per-pixel rule of csrc/svs_colour.hpp (the one the fused colour kernel applies), built for
the host by tests/hostemu, checked exhaustively; a NumPy restatement of the rule (used by the GPU
tests as their expected output) against it; the flag and the Python parameters that expose it."""
import inspect
import os
import re
import threading

import numpy as np
import pytest

from testlib import REPO, hostemu
from svsdct import batch, native

TABLES = {"15-bit": (3735, 19235, 9798, 15), "14-bit": (1868, 9617, 4899, 14)}


def keep_colour_rule(bgr, t, weights):
    """NumPy restatement of svs::keep_colour_pixel: bgr uint8 [..., 3] (cover), t uint8 [...] (stego gray) -> uint8 [..., 3].
    P = clamp(c + d) with d = t - gray(c); then, channel by channel in decreasing weight order (ties: B, G, R; weight 0
    skipped), the smallest move toward t that reaches it, limited to [0, 255]."""
    wb, wg, wr, s = (int(x) for x in weights)
    w = np.array([wb, wg, wr], np.int64)
    one, half = 1 << s, 1 << (s - 1)
    c = np.asarray(bgr).astype(np.int64)
    t = np.asarray(t).astype(np.int64)
    d = t - ((c @ w + half) >> s)
    p = np.clip(c + d[..., None], 0, 255)
    for k in sorted(range(3), key=lambda i: -w[i]):          # stable sort: equal weights keep B, G, R order
        if w[k] == 0:
            continue
        acc = p @ w
        y = (acc + half) >> s
        pk = p[..., k]
        up = -(-(t * one - half - acc) // w[k])              # ceil; only used where y < t (positive numerator)
        down = -(-(acc + half + 1 - (t + 1) * one) // w[k])  # ceil; only used where y > t
        pk = np.where(y < t, pk + np.minimum(up, 255 - pk), pk)
        pk = np.where(y > t, pk - np.minimum(down, pk), pk)
        p[..., k] = pk
    return p.astype(np.uint8)


def gray_of(bgr, weights):
    wb, wg, wr, s = (int(x) for x in weights)
    c = np.asarray(bgr).astype(np.int64)
    return ((c[..., 0] * wb + c[..., 1] * wg + c[..., 2] * wr + (1 << (s - 1))) >> s).astype(np.uint8)


@pytest.fixture(scope="module")
def shim():
    return hostemu()


def _check(lib, first, count, stride, radius, weights):
    w = np.array(weights, np.uint32)
    v = np.zeros(4, np.uint64)
    pairs = lib.kc_check(first, count, stride, radius, w.ctypes.data, v.ctypes.data)
    return int(pairs), [int(x) for x in v]


def test_rule_exhaustive_both_tables(shim):
    """All 2^24 colours x every stego gray within 24 of the cover gray, and every stego gray 0..255 for a 2^16-colour
    sample, both weight tables: gray(out) == t, out == c + d wherever c + d stays in [0, 255], d == 0 gives the cover,
    and no channel moves against d.  (The two tables run on two threads: ctypes releases the GIL.)"""
    results = {}

    def run(name):
        near = _check(shim, 0, 1 << 24, 1, 24, TABLES[name])
        every = _check(shim, 12345, 1 << 16, 2654435761 & 0xffffff, 255, TABLES[name])  # odd stride: distinct colours
        results[name] = (near, every)

    threads = [threading.Thread(target=run, args=(n,)) for n in TABLES]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for name, (near, every) in results.items():
        assert near[0] > 49 * (1 << 24) * 0.9, name                # every colour, up to 49 targets each
        assert every[0] == 256 * (1 << 16), name
        for pairs, v in (near, every):
            assert v == [0, 0, 0, 0], (name, pairs, v)
    # the saturated corners of the cube against every target
    w = np.array(TABLES["15-bit"], np.uint32)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    bgr = np.repeat(corners, 256, axis=0)
    t = np.tile(np.arange(256, dtype=np.uint8), 8)
    out = np.empty_like(bgr)
    shim.kc_apply(bgr.ctypes.data, t.ctypes.data, out.ctypes.data, t.size, w.ctypes.data)
    assert np.array_equal(gray_of(out, w), t)


def test_numpy_restatement_equals_the_header(shim):
    """keep_colour_rule (the GPU tests' expectation) equals the compiled header on 2^22 random (colour, target) pairs per
    table - half of them near the cover gray, half anywhere - plus saturated colours, and a table with a zero weight."""
    rng = np.random.default_rng(2024)
    n = 1 << 22
    for weights in list(TABLES.values()) + [(0, 40000, 25536, 16), (8, 4, 4, 4)]:
        bgr = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        bgr[: n // 8] = rng.choice(np.array([0, 255], np.uint8), (n // 8, 3))      # cube corners and edges
        bgr[n // 8: n // 4, 1] = 255
        g0 = gray_of(bgr, weights).astype(np.int64)
        t = rng.integers(0, 256, n)
        t[n // 2:] = np.clip(g0[n // 2:] + rng.integers(-24, 25, n - n // 2), 0, 255)
        t = t.astype(np.uint8)
        w = np.array(weights, np.uint32)
        want = np.empty_like(bgr)
        shim.kc_apply(bgr.ctypes.data, t.ctypes.data, want.ctypes.data, n, w.ctypes.data)
        got = keep_colour_rule(bgr, t, weights)
        assert np.array_equal(got, want), (weights, int((got != want).any(axis=1).sum()))
        assert np.array_equal(gray_of(want, weights), t), weights


def test_flag_and_python_parameters():
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    m = re.search(r"#define SVS_KEEP_COLOUR (0x[0-9a-fA-F]+)u", header)
    assert m and int(m.group(1), 16) == 0x100 == native.SVS_KEEP_COLOUR
    assert native.SVS_KEEP_COLOUR & (native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED) == 0
    for name in ("embed_bgr_frames", "embed_bgr_device"):
        params = inspect.signature(getattr(batch, name)).parameters
        assert params["keep_colour"].default is False, name
        assert params["mode"].default is None, name
    import embed_process
    assert embed_process.KEEP_COLOUR is (os.environ.get("SVS_KEEP_COLOUR", "0") == "1")
