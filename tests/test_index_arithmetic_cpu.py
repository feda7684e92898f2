"""The kernels' index arithmetic (csrc/svs_index.hpp; the payload readers of csrc/svs_block.hpp) against plain Python
integers, through tests/hostemu: the multiply-shift division, the workgroup -> tile maps, the pixel offset of a block with
64-bit pitches, a block's place in the payload stream, and the 64-bit payload windows at stream positions past 2^32.

This arithmetic leaves its trivial regime only at sizes the small GPU tests never reach (a grid of 256 workgroups and more,
2^31 blocks, offsets past 4 GiB); the GPU tier (tests/test_index_arithmetic_gpu.py) runs the kernels there, this tier says
at once which expression is wrong."""
import numpy as np
import pytest

import index_lib as ix
from svsdct import order

K8 = ix.K_EIGHTH
LIMIT = 1 << 31          # dividends and block counts stay below 2^31 (make_geometry refuses more)

# (width / 8, blocks per frame) of the BASELINE.json shapes: 640x480, 1920x1080, 3840x2160, 7680x4320
BASELINE_WB_BPF = [(80, 4800), (240, 32400), (480, 129600), (960, 518400)]


def divisors():
    d = set(range(1, 4097))
    for k in range(31):
        d.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
    d.add(2 ** 31 - 1)
    for wb, bpf in BASELINE_WB_BPF:
        d.update((wb, bpf))
    d.update((129600, 518400))
    return sorted(x for x in d if 1 <= x < LIMIT)


def dividends(d):
    """0, 1, 2^31 - 1 and m d - 1, m d, m d + 1 for 64 multipliers m spread over [1, (2^31 - 1) / d]"""
    top = (LIMIT - 1) // d
    ms = {1, 2, 3, top, max(top - 1, 1)} | {max(1, (top * j) // 59) for j in range(1, 60)}
    ns = {0, 1, LIMIT - 1}
    for m in ms:
        ns.update((m * d - 1, m * d, m * d + 1))
    return np.array(sorted(n for n in ns if 0 <= n < LIMIT), np.uint64)


def test_fast_div_is_exact_below_2_to_the_31():
    for d in divisors():
        mul, shift, div = ix.make_div(d)
        l = (d - 1).bit_length()                       # ceil(log2 d)
        want_mul = -((-1 << (31 + l)) // d)            # ceil(2^shift / d)
        assert (mul, shift, div) == (want_mul, 31 + l, d) and want_mul < 1 << 32, (d, mul, shift, want_mul)
        ns = dividends(d)
        got = ix.fast_div(ns.astype(np.uint32), d)
        bad = np.flatnonzero(got != ns // np.uint64(d))
        assert bad.size == 0, (d, int(ns[bad[0]]), int(got[bad[0]]), int(ns[bad[0]]) // d)


def is_permutation(t):
    return t.size == 0 or (int(t.max()) == t.size - 1 and np.bincount(t, minlength=t.size).max() == 1)


@pytest.mark.parametrize("chunk", [0, 1, 7, 32, K8])
def test_tile_map_is_a_permutation_for_every_grid(chunk):
    """grid 1 .. 4200: the chunk = 32 form's span of 256 workgroups through 16 whole rounds and every remainder"""
    for grid in range(1, 4201):
        t = ix.tile_map(grid, chunk)
        assert is_permutation(t), (chunk, grid)
        if chunk == 0:
            assert np.array_equal(t, np.arange(grid))


# 600 frames of 3840 x 2160: 77 760 000 blocks, one and two per lane
GRIDS_600_4K = [-(-600 * 129600 // 256), -(-600 * 129600 // 512)]


@pytest.mark.parametrize("grid", [(1 << 20) + k for k in range(-3, 4)] + GRIDS_600_4K)
def test_tile_map_at_large_grids(grid):
    for chunk in (1, 7, 32, K8):
        t = ix.tile_map(grid, chunk)
        assert is_permutation(t), (chunk, grid)
    eighth_is_contiguous(grid)
    runs_of_32(grid)


def eighth_is_contiguous(grid):
    """kEighth: the workgroups of XCD-group x (i % 8 == x), in launch order, take consecutive tiles - one run per group,
    the groups' runs in order"""
    t = ix.tile_map(grid, K8).astype(np.int64)
    start = 0
    for x in range(8):
        mine = t[x::8]
        assert np.array_equal(mine, start + np.arange(mine.size)), (grid, x)
        start += mine.size
    assert start == grid


def runs_of_32(grid):
    """chunk = 32: below `full` (whole rounds of 256 workgroups), workgroups i and i + 8 - the same XCD-group, launched one
    after the other - hold adjacent tiles unless i closes a run of 32; a run starts at a multiple of 32; past `full` the
    map is the identity"""
    t = ix.tile_map(grid, 32).astype(np.int64)
    full = grid // 256 * 256
    i = np.arange(max(full - 8, 0))
    inside = (i // 8) % 32 != 31
    assert np.array_equal(t[i + 8][inside], t[i][inside] + 1), grid
    starts = i[(i // 8) % 32 == 0]
    assert (t[starts] % 32 == 0).all(), grid
    assert np.array_equal(t[full:], np.arange(full, grid)), grid
    if full:   # round g holds tiles [256 g, 256 g + 256), XCD-group x of it the 32 tiles from 32 x
        j = np.arange(full)
        assert np.array_equal(t[j] // 256, j // 256) and np.array_equal(t[j] % 256 // 32, j % 8), grid


@pytest.mark.parametrize("grid", [1, 5, 8, 9, 15, 16, 17, 255, 256, 257, 263, 511, 512, 519, 1023, 2049, 4097])
def test_tile_map_intent(grid):
    eighth_is_contiguous(grid)
    runs_of_32(grid)


# (frames, block rows, blocks per row); the last one has 2^31 - 270 848 blocks.  Blocks are sampled: every edge, 4000 others
GEOMETRIES = [(7, 3, 1), (5, 5, 25), (3, 6, 34), (600, 270, 480), (1200, 540, 960), (16568, 135, 960)]
PITCHES = ["tight", "padded", (1 << 31) + (1 << 20) + 16, 1 << 36, 1 << 40]


def sample_blocks(total, bpf, wb, rng):
    edges = {0, 1, wb - 1, wb, bpf - 1, bpf, bpf + 1, total - bpf, total - wb, total - 2, total - 1, total // 2}
    some = rng.integers(0, total, 4000)
    return np.array(sorted({int(b) for b in edges if 0 <= b < total} | {int(b) for b in some}), np.int64)


@pytest.mark.parametrize("bgr", [False, True], ids=["gray", "bgr"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=[f"{f}x{hb}x{wb}" for f, hb, wb in GEOMETRIES])
def test_block_offset_with_64_bit_pitches(geom, bgr):
    f, hb, wb = geom
    bpf, px = hb * wb, 3 if bgr else 1
    total = f * bpf
    assert total < LIMIT
    rng = np.random.default_rng(wb)
    blocks = sample_blocks(total, bpf, wb, rng)
    for kind in PITCHES:
        if kind == "tight":
            rp = 8 * wb * px
            fp = 8 * hb * rp
        elif kind == "padded":
            rp = 8 * wb * px + 40
            fp = 8 * hb * rp + 4096
        elif kind >= 1 << 36:
            rp = 8 * wb * px + 8
            fp = kind                                   # frame pitch alone: f * 2^40 < 2^63
        else:
            rp = (1 << 27) + 16
            fp = max(kind, 8 * hb * rp)
        assert (f - 1) * fp + 8 * hb * rp < 1 << 63
        got = ix.block_offsets(blocks, wb, bpf, rp, fp, bgr)
        for b, o in zip(blocks.tolist(), got.tolist()):
            frame, in_frame = divmod(b, bpf)
            brow, bcol = divmod(in_frame, wb)
            want = frame * fp + 8 * brow * rp + (24 if bgr else 8) * bcol
            assert o == want, (geom, kind, b, o, want)
        last = ix.block_offsets([total - 1], wb, bpf, rp, fp, bgr)[0]
        assert int(last) == (f - 1) * fp + 8 * (hb - 1) * rp + (24 if bgr else 8) * (wb - 1)


def test_block_offset_at_the_limits_of_a_call():
    """the widest frame (svs_planes.width is an int32: at most 2^28 - 1 blocks per row; a colour row stays below 4 GiB, so
    at most (2^32 - 1) // 24 blocks - the colour calls refuse more, the byte column is a 32-bit product) and the most frames
    (2^31 - 1 of one block)"""
    for wb, col in (((1 << 28) - 1, 8), (((1 << 32) - 1) // 24, 24)):
        hb = 7
        total, rp = hb * wb, col * wb + 8
        blocks = np.array([0, 1, wb - 1, wb, total // 2, total - 2, total - 1], np.int64)
        got = ix.block_offsets(blocks, wb, total, rp, 8 * hb * rp, bgr=col == 24)
        assert got.tolist() == [8 * (b // wb) * rp + col * (b % wb) for b in blocks.tolist()]
    total = LIMIT - 1
    blocks = np.array([0, 1, total // 2, total - 2, total - 1], np.int64)
    fp = (1 << 31) + 64
    got = ix.block_offsets(blocks, 1, 1, 8, fp)
    assert got.tolist() == [b * fp for b in blocks.tolist()]


def test_stream_first_raster_and_keyed():
    """a block's first stream bit: gblock * n in 64 bits, and under the keyed order (frame N + slot) * n with the slot of
    svsdct/order.py - at block numbers whose products pass 2^32 and 2^37"""
    for n, bpf, frames in ((3, 129600, 600), (63, 1024, 66600), (63, 32400, 66000), (10, 375, 7)):
        total = frames * bpf
        assert total < LIMIT
        rng = np.random.default_rng(n + bpf)
        blocks = np.unique(np.concatenate([rng.integers(0, total, 300), [0, 1, bpf - 1, bpf, total - 1, (1 << 32) // n,
                                                                         (1 << 32) // n + 1]])).astype(np.int64)
        blocks = blocks[blocks < total]
        got = ix.stream_firsts(blocks, n, bpf)
        assert got.tolist() == [b * n for b in blocks.tolist()]
        key, t0 = 0x0123456789ABCDEF, 5
        even = blocks[(blocks % bpf) < bpf - 1]          # the right neighbour lies in the same frame
        first, second = ix.stream_firsts(even, n, bpf, key=key, first_frame=t0, want_second=True)
        slots = {}
        for b, a, c in zip(even.tolist(), first.tolist(), second.tolist()):
            fr, i = divmod(b, bpf)
            if fr not in slots:
                slots[fr] = order.block_to_slot(key, t0 + fr, bpf)
            assert a == (fr * bpf + int(slots[fr][i])) * n and c == (fr * bpf + int(slots[fr][i + 1])) * n, (n, bpf, b)


def stream_bits(window_bytes, word_base, n_words, s, count):
    """bits [s, s + count) of an MSB-first packed buffer of n_words dwords (zero past its end) as one Python integer; the
    buffer's bytes from 4 word_base on are window_bytes"""
    have = min(len(window_bytes), max(0, 4 * (n_words - word_base)))
    value = int.from_bytes(bytes(window_bytes[:have]), "big") << 128          # zero fill past the end
    width = 8 * have + 128
    rel = s - 32 * word_base
    assert 0 <= rel and rel + count <= width
    return (value >> (width - rel - count)) & ((1 << count) - 1)


BIG_WORDS = (1 << 32) - 1                     # the largest n_words a call takes
POSITIONS = [0, 31, 32, 37, (1 << 32) - 19, 1 << 32, (1 << 32) + 37, (1 << 35) + 5] + \
            [32 * (BIG_WORDS - 2) + k for k in (0, 1, 13, 31)]


@pytest.mark.parametrize("s", POSITIONS)
def test_payload_windows_at_stream_positions_past_2_to_the_32(s):
    """payload_window's 64 bits and payload_qword's (the 64 bits from the dword that holds bit s) against bits sliced from a
    Python integer.  The buffer is a sparse 16 GiB mapping holding the window and, where a position truncated to 32 bits would
    read, its complement (without such a mapping: the window alone, behind a biased pointer).  n_words: far past the window, ending one, two and
    three dwords into it (zero fill), and ending before it."""
    rng = np.random.default_rng(s % 1000003)
    wi = s >> 5
    window = rng.integers(0, 256, 16, dtype=np.uint8)                  # dwords wi .. wi + 3
    window |= 0x11                                                      # no zero byte: zero fill cannot pass by chance
    sparse = ix.sparse_payload()
    decoy = 4 * (wi % (1 << 27))                                        # where a position truncated to 32 bits reads
    if sparse is not None:                                              # the whole buffer, sparse: word base 0
        if decoy != 4 * wi:
            sparse[decoy:decoy + 16] = ~window
        sparse[4 * wi:4 * wi + 16] = window
        words, base = sparse[:4].view("<u4"), 0
    else:
        words, base = window.view("<u4"), wi
    try:
        for n_words in sorted(v for v in {wi + 1000, wi + 3, wi + 2, wi + 1, wi} if v <= BIG_WORDS):
            got = ix.payload_window(words, base, n_words, s)
            assert got == stream_bits(window, wi, n_words, s, 64), (s, n_words, hex(got))
            q = ix.payload_qword(words, base, n_words, s)
            assert q == stream_bits(window, wi, n_words, 32 * wi, 64), (s, n_words, hex(q))
            for sh in (s & 31, (s & 31) + 15):               # a block's window, and its right neighbour's (n <= 15: sh < 47)
                have = min(32, 64 - sh)                      # the qword's bits from sh on, left-aligned; zeros behind them
                assert ix.emu().emu_window32(q, sh) == stream_bits(window, wi, n_words, 32 * wi + sh, have) << (32 - have)
    finally:
        if sparse is not None:
            sparse[4 * wi:4 * wi + 16] = 0
            sparse[decoy:decoy + 16] = 0


def test_window32_shifts():
    q = 0x0123456789ABCDEF
    for sh in range(0, 47):
        assert ix.emu().emu_window32(q, sh) == (q << sh >> 32) & 0xFFFFFFFF
