"""Helpers of the tie-corpus tests (tests/test_tie_corpus_cpu.py, tests/test_tie_corpus_gpu.py): the committed corpus of
tests/golden/make_tie_corpus.py, the frames the tests lay its strips out in, the payload that gives every `lattice` block its
recorded bit, and the message that names the class of the first block two results differ in."""
import functools
import json
import os

import numpy as np

import dither_lib as dl
from testlib import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
with open(os.path.join(GOLDEN, "tie_corpus.json")) as _fh:
    META = json.load(_fh)
KEY, FIRST_FRAME = META["key"], META["first_frame"]
ORDER_KEY = 0xC0FFEE1234
FAMILIES = {f: (tuple(v["n_acs"]), tuple(v["ks"])) for f, v in META["families"].items()}
MODES = META["modes"]                                   # "d<delta>" -> pow2 / f32 / double
WIDTHS = (136, 144)                                     # 17 blocks per row: one block per lane; 18: two blocks per lane


def tag(delta):
    return "d" + repr(delta)


def deltas_of(family):
    return tuple(META["deltas"]) + (tuple(META["deltas_row8"]) if family == "row8" else ())


def settings(families=("row1", "row2", "row8")):
    """(family, n_ac, delta) of every frame set"""
    return [(f, n, d) for f in families for n in FAMILIES[f][0] for d in deltas_of(f)]


def setting_id(s):
    return f"{s[0]}-n{s[1]}-{tag(s[2])}"


def one_setting_per_family_and_mode():
    """one (family, n_ac, delta) per family and quantiser mode: the larger n of the family"""
    out = []
    for f in FAMILIES:
        for d in (8, 12.5, 7.3):
            out.append((f, FAMILIES[f][0][1], d))
    return out


@functools.lru_cache(maxsize=None)
def _arrays():
    return np.load(os.path.join(GOLDEN, "tie_corpus.npz"))


def blocks_of(delta):
    """-> (uint8 [K, 8, 8], the K records of the JSON)"""
    strip = _arrays()[tag(delta) + "/strip"]
    return np.ascontiguousarray(strip.reshape(8, -1, 8).transpose(1, 0, 2)), META["blocks"][tag(delta)]


def to_blocks(frames):
    f, h, w = frames.shape
    return frames.reshape(f, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4).reshape(f, -1, 8, 8)


def from_blocks(blocks, h, w):
    f = blocks.shape[0]
    return np.ascontiguousarray(blocks.reshape(f, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(f, h, w))


@functools.lru_cache(maxsize=None)
def frames_for(n, delta, width):
    """Two frames [2, H, width] with every corpus block of `delta` whose k <= n: the dither blocks at their slot (f, i), the
    others spread evenly over the free slots of both frames, noise (dither_lib.noise) everywhere else; at least four block
    rows.  -> (frames (read-only), where): where[(f, p)] = the record of the corpus block at raster block p of frame f."""
    blocks, records = blocks_of(delta)
    use = [j for j, r in enumerate(records) if r["k"] <= n]
    slotted = [j for j in use if records[j]["class"] == "dither_tie"]
    free_blocks = [j for j in use if records[j]["class"] != "dither_tie"]
    bpr = width // 8
    per_frame = -(-len(free_blocks) // 2) + len(slotted)
    rows = max(4, -(-per_frame // bpr))
    h, nblk = 8 * rows, rows * bpr
    grid = to_blocks(dl.noise((2, h, width), seed=int(n * 1000 + width))).copy()
    where = {}
    for j in slotted:
        where[(records[j]["f"], records[j]["i"])] = j
    for f in range(2):
        mine = free_blocks[f::2]
        free = [p for p in range(nblk) if (f, p) not in where]
        for j, at in zip(mine, np.linspace(0, len(free) - 1, len(mine)).astype(int)):
            assert (f, free[at]) not in where
            where[(f, free[at])] = j
    assert len(where) == len(use) and nblk >= 65
    for (f, p), j in where.items():
        grid[f, p] = blocks[j]
    frames = from_blocks(grid, h, width)
    frames.setflags(write=False)
    return frames, {fp: records[j] for fp, j in where.items()}


def payload_for(frames, where, n, index=None, seed=3):
    """random bits for the whole capacity of `frames`; the coefficient k of every `lattice` block carries its recorded bit
    (the one that differs from the parity of its index).  index: None (coefficients 1..n) or a selection."""
    index = list(range(1, n + 1)) if index is None else [int(k) for k in index]
    nblk = (frames.shape[1] // 8) * (frames.shape[2] // 8)
    bits = dl.payload(frames.shape[0] * nblk * len(index), seed=seed)
    for (f, p), r in where.items():
        if r["class"] == "lattice" and r["k"] in index:
            bits[(f * nblk + p) * len(index) + index.index(r["k"])] = r["bit"]
    return bits


def blame(where, got, want, bits_per_block=None, perm=None):
    """names the first corpus block in which two results differ.  Pixels: got / want are frames [2, H, W].  Bits
    (bits_per_block set): 0/1 streams of the two frames.  perm: (optional) per frame, stream slot -> raster block."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes differ: {got.shape} != {want.shape}"
    if bits_per_block is None:
        bad = (to_blocks(got) != to_blocks(want)).reshape(got.shape[0], -1, 64).any(2)
    else:
        bad = (got != want).reshape(2, -1, bits_per_block).any(2)
        if perm is not None:
            raster = np.zeros_like(bad)
            for f in range(2):
                raster[f, perm[f]] = bad[f]
            bad = raster
    cells = np.argwhere(bad)
    if not len(cells):
        return "no difference"
    hits = [(int(f), int(p), where[(int(f), int(p))]) for f, p in cells if (int(f), int(p)) in where]
    if not hits:
        return f"{len(cells)} blocks differ, the first (frame {cells[0][0]}, block {cells[0][1]}) is no corpus block"
    f, p, r = hits[0]
    return (f"{len(cells)} blocks differ; first corpus block: frame {f}, block {p}, class {r['class']}"
            f"{'/' + r['sub'] if 'sub' in r else ''}, k = {r['k']}, delta = {r['delta']}, c = {float.fromhex(r['c'])!r}, "
            f"floor parity {r['floor_parity']}, diverge {r['diverge']}")
