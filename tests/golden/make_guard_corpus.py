"""Writes tests/golden/guard_corpus.npz / guard_corpus.json: blocks that sit at the boundary of the streaming kernels' guard
(BETA, csrc/svs_block.hpp make_guard) and of FAST extraction's tie margin (make_qim), laid out in frames.

For one block under a setting (n, delta, its payload window), s* is the largest guard scale at which the cheap path keeps
the block and its pixels differ from the exact (pocketfft-identical) arithmetic; 0 for a block whose cheap result is right
at any scale.  t* is the same for extraction and the tie margin.  Both are found by bisection over float32 scales on
hostemu (tests/hostemu: testlib.emu_scales), so that "differs at scale x" is exactly "x <= s*".

Search: random blocks of several content classes and the blocks of testlib.structured_covers, then a hill-climb on +-1
pixel moves that keeps every move not lowering s* (t*).  The best blocks per setting are placed into 544 x 960 frames so
that some waves of 64 blocks (128 in the two-blocks-per-lane form) hold 1, 8, 31, 32, 33, 64 (128) of them; every other
block is filler that the guard decides at scale 1 and whose cheap result is right at any scale.

The file stores what the frames are made of, not the frames: per setting the corpus blocks, their payload bits, positions
and stars, a library of 8 filler blocks and each block's filler index (filler blocks carry all-zero payload bits);
testlib.guard_corpus_case rebuilds frame and payload.

CPU only, seeded, deterministic: `python tests/golden/make_guard_corpus.py` reproduces both files byte for byte.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"), os.path.join(REPO, "tests"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import testlib  # noqa: E402
from oracle import qim_dct_oracle as orc  # noqa: E402

SEED = 20261015
H, W = 544, 960
KEEP = 256            # corpus blocks per setting

# one setting per kernel family of svs_embed_dev (n, delta, width): quantiser mode from delta (pow2 / float32 / double)
EMBED_SETTINGS = [
    ("row1_two_blocks_per_lane", 3, 8.0, 960),
    ("row1_one_block_per_lane", 7, 7.5, 952),      # 119 blocks per row: odd, one block per lane
    ("row1_double", 5, 7.3, 960),
    ("row2_worklist", 9, 8.0, 960),
    ("row2_n10", 10, 8.0, 960),
    ("row2_parked_f32", 12, 12.5, 960),
    ("row2_parked_double", 15, 7.3, 960),
    ("delta_min", 6, 0.25, 960),
    ("delta_max", 11, 4096.0, 960),
]
EXTRACT_SETTINGS = [
    ("extract_n8", 8, 4.0),
    ("extract_n10", 10, 8.0),
    ("extract_n16", 16, 3.5),
    ("extract_n36", 36, 2.0),
    ("extract_n63", 63, 1.5),
]
WAVE_COUNTS = (1, 8, 31, 32, 33, 64)


def _blocks_to_strip(blocks):
    """[K, 8, 8] -> one 8 x 8K frame"""
    return np.ascontiguousarray(blocks.transpose(1, 0, 2).reshape(8, -1))[None]


def _strip_to_blocks(frame):
    return frame[0].reshape(8, -1, 8).transpose(1, 0, 2)


# ---- embed: s* ---------------------------------------------------------------------------------------------------------
def embed_differs(blocks, bits, n, delta, scale):
    """bool per block: the guarded output at `scale` differs from the exact arithmetic (bits: [K, n])"""
    fr = _blocks_to_strip(blocks)
    flat = bits.reshape(-1)
    exact, _ = testlib.emu_embed(fr, delta, n, flat, exact=1)
    with testlib.emu_scales(guard=scale):
        got, _ = testlib.emu_embed(fr, delta, n, flat, exact=4)
    return (_strip_to_blocks(got) != _strip_to_blocks(exact)).reshape(len(blocks), -1).any(1)


def bisect_star(differs_one):
    """largest float32 scale x in [0, 1] with differs_one(x) (differs_one monotone: true below s*, false above); 0 if none"""
    if not differs_one(np.float32(0.0)):
        return 0.0
    assert not differs_one(np.float32(1.0)), "differs at scale 1: the product bound does not hold"
    lo, hi = np.float32(0.0), np.float32(1.0)
    while np.nextafter(lo, np.float32(2)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid <= lo or mid >= hi:
            mid = np.nextafter(lo, np.float32(2))
        if differs_one(mid):
            lo = mid
        else:
            hi = mid
    return float(lo)


def embed_star(block, bits, n, delta):
    return bisect_star(lambda s: bool(embed_differs(block[None], bits[None], n, delta, s)[0]))


def candidate_blocks(rng, count, covers):
    """[count, 8, 8] uint8: content classes in which the guard's margin is thin (smooth and bright blocks: large pixel
    values, small residual) plus uniform noise and blocks of the structured covers"""
    kinds = []
    q = count // 6
    base = rng.integers(20, 250, (q, 1, 1))
    gx = rng.integers(-3, 4, (q, 1, 1)) * np.arange(8)[None, None, :]
    gy = rng.integers(-3, 4, (q, 1, 1)) * np.arange(8)[None, :, None]
    kinds.append(np.clip(base + gx + gy + rng.integers(-2, 3, (q, 8, 8)), 0, 255))                  # smooth
    kinds.append(rng.integers(200, 256, (q, 8, 8)))                                                 # bright noise
    kinds.append(np.clip(rng.integers(150, 256, (q, 1, 1)) + rng.integers(-1, 2, (q, 8, 8)), 0, 255))   # near flat
    kinds.append(rng.integers(0, 256, (q, 8, 8)))                                                   # uniform
    cov = covers[rng.integers(0, len(covers), q)]
    kinds.append(np.clip(cov.astype(np.int64) + rng.integers(-1, 2, (q, 8, 8)) * rng.integers(0, 2, (q, 1, 1)), 0, 255))
    rest = count - 5 * q
    kinds.append(np.clip(rng.integers(100, 256, (rest, 1, 1)) + rng.integers(-6, 7, (rest, 8, 8)), 0, 255))
    return np.concatenate(kinds).astype(np.uint8)


def cover_blocks():
    out = []
    for img in testlib.structured_covers(64, 128, seed=5).values():
        out.append(img.reshape(8, 8, 16, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8))
    return np.concatenate(out)


def hill_climb(rng, blocks, bits, stars, star_fn, differs_fn, rounds, moves):
    """+-1 pixel moves on the given blocks, keeping a move when s* does not drop"""
    blocks, stars = blocks.copy(), stars.copy()
    for _ in range(rounds):
        for i in range(len(blocks)):
            cand = np.repeat(blocks[i][None], moves, 0).astype(np.int64)
            pos = rng.integers(0, 64, moves)
            step = rng.choice([-1, 1], moves)
            cand.reshape(moves, 64)[np.arange(moves), pos] += step
            cand = np.clip(cand, 0, 255).astype(np.uint8)
            d = differs_fn(cand, np.repeat(bits[i][None], moves, 0))
            best = stars[i]
            for j in np.flatnonzero(d):
                s = star_fn(cand[j], bits[i])
                if s >= best:
                    best, blocks[i] = s, cand[j]
            stars[i] = best
    return blocks, stars


def search_embed(rng, n, delta, covers, pool, climb_top, rounds, moves):
    blocks = candidate_blocks(rng, pool, covers)
    bits = rng.integers(0, 2, (pool, n)).astype(np.uint8)
    d = embed_differs(blocks, bits, n, delta, 0.0)
    idx = np.flatnonzero(d)
    stars = np.array([embed_star(blocks[i], bits[i], n, delta) for i in idx])
    blocks, bits = blocks[idx], bits[idx]
    order = np.argsort(-stars, kind="stable")
    blocks, bits, stars = blocks[order], bits[order], stars[order]
    top = slice(0, climb_top)
    blocks[top], stars[top] = hill_climb(rng, blocks[top], bits[top], stars[top],
                                         lambda b, p: embed_star(b, p, n, delta),
                                         lambda b, p: embed_differs(b, p, n, delta, 0.0), rounds, moves)
    return dedupe_best(blocks, bits, stars)


def dedupe_best(blocks, extra, stars):
    order = np.argsort(-np.asarray(stars), kind="stable")
    seen, keep = set(), []
    for i in order:
        key = blocks[i].tobytes() + (extra[i].tobytes() if extra is not None else b"")
        if key not in seen and stars[i] > 0:
            seen.add(key)
            keep.append(i)
        if len(keep) == KEEP:
            break
    keep = np.array(keep, np.int64)
    return blocks[keep], (extra[keep] if extra is not None else None), np.asarray(stars)[keep]


# ---- extraction: t* ----------------------------------------------------------------------------------------------------
def extract_differs(blocks, n, delta, scale):
    fr = _blocks_to_strip(blocks)
    exact = testlib.emu_extract(fr, delta, n, exact=True).reshape(len(blocks), n)
    with testlib.emu_scales(tie=scale):
        got = testlib.emu_extract(fr, delta, n).reshape(len(blocks), n)
    return (got != exact).any(1)


def extract_star(block, n, delta):
    return bisect_star(lambda s: bool(extract_differs(block[None], n, delta, s)[0]))


def search_extract(rng, n, delta, covers, pool, climb_top, rounds, moves):
    blocks = candidate_blocks(rng, pool, covers)
    idx = np.flatnonzero(extract_differs(blocks, n, delta, 0.0))
    stars = np.array([extract_star(blocks[i], n, delta) for i in idx])
    blocks = blocks[idx]
    order = np.argsort(-stars, kind="stable")
    blocks, stars = blocks[order], stars[order]
    top = slice(0, climb_top)
    dummy = np.zeros((len(blocks), 1), np.uint8)
    blocks[top], stars[top] = hill_climb(rng, blocks[top], dummy[top], stars[top],
                                         lambda b, p: extract_star(b, n, delta),
                                         lambda b, p: extract_differs(b, n, delta, 0.0), rounds, moves)
    blocks, _, stars = dedupe_best(blocks, None, stars)
    return blocks, stars


# ---- layout ------------------------------------------------------------------------------------------------------------
def layout_positions(rng, n_corpus, n_blocks, wave):
    """block indices for the corpus: wave k (of `wave` blocks) holds WAVE_COUNTS[k] (and `wave` itself when it is 128)
    corpus blocks at random lanes; the rest one per wave in the waves after those"""
    counts = list(WAVE_COUNTS) + ([128] if wave == 128 else [])
    pos = []
    for k, c in enumerate(counts):
        c = min(c, n_corpus - len(pos))
        pos += sorted((k * wave + rng.choice(wave, c, replace=False)).tolist())
    w = len(counts)
    while len(pos) < n_corpus:
        pos.append(w * wave + int(rng.integers(0, wave)))
        w += 1
    assert max(pos) < n_blocks
    return np.array(pos, np.int64)


def filler_library(rng, count, bad):
    """filler blocks for which bad(blocks) is false (a smooth, low-noise content class)"""
    lib = []
    while len(lib) < count:
        base = rng.integers(30, 200, (64, 1, 1))
        gx = rng.integers(-2, 3, (64, 1, 1)) * np.arange(8)[None, None, :]
        cand = np.clip(base + gx + rng.integers(0, 3, (64, 8, 8)), 0, 255).astype(np.uint8)
        lib += [c for c in cand[~bad(cand)]]
    return np.stack(lib[:count])


def blocks_to_frame(blocks, h, w):
    return np.ascontiguousarray(blocks.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w))


def frame_to_blocks(frame):
    h, w = frame.shape
    return frame.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def test_scale(stars):
    """0.9 x max star, moved off any block's star by at least 0.1 % (the device's sqrt may differ from the host's by an ulp)"""
    x = np.float32(0.9 * max(stars))
    s = np.asarray(stars)
    while np.any(np.abs(s - x) <= 1e-3 * x):
        x = np.float32(x * 0.997)
    return float(x)


FILLER = 8            # filler library blocks per setting; block gb starts as library block gb % FILLER


def stored(arrays, name, meta):
    """the frame (and payload) as tests rebuild them from what goes into the file"""
    return testlib.guard_corpus_case({name + "/" + k: v for k, v in arrays.items()}, meta, name)


def build_embed(rng, name, n, delta, width, covers, quick, floor):
    """`floor`: the search goes on - fresh pools, hill-climbed again, merged with what it has - until the largest s* reaches
    it (half the err / BETA that tools/guard_bound.py samples: tests/test_guard_sensitivity_cpu.py::test_search_is_sharp)"""
    pool, top, rounds, moves = (20000, 8, 1, 16) if quick else (800000, 64, 16, 128)
    corpus, bits, stars = search_embed(rng, n, delta, covers, pool, top, rounds, moves)
    for attempt in range(8):
        if quick or stars.max() >= floor:
            break
        more = search_embed(rng, n, delta, covers, pool, top, rounds, moves)
        corpus, bits, stars = dedupe_best(np.concatenate([corpus, more[0]]), np.concatenate([bits, more[1]]),
                                          np.concatenate([stars, more[2]]))
    else:
        raise RuntimeError(f"{name}: max s* {stars.max()} stays below the floor {floor}")
    wave = 128 if name == "row1_two_blocks_per_lane" else 64
    nblk = (H // 8) * (width // 8)
    positions = layout_positions(rng, len(corpus), nblk, wave)
    zeros = lambda c: np.zeros((len(c), n), np.uint8)          # filler blocks carry all-zero payload bits
    filler = filler_library(rng, FILLER, lambda c: embed_differs(c, zeros(c), n, delta, 0.0))
    index = (np.arange(nblk) % FILLER).astype(np.uint8)
    payload = np.zeros((nblk, n), np.uint8)
    payload[positions] = bits
    corpus_mask = np.zeros(nblk, bool)
    corpus_mask[positions] = True
    # filler the guard leaves undecided at scale 1, or whose cheap result is wrong: another library block until none.  (At
    # the top of the delta range clipping leaves some filler undecided whatever it is: there only the second condition.)
    for it in range(60):
        blocks = filler[index]
        blocks[positions] = corpus
        frame = blocks_to_frame(blocks, H, width)
        replayed = testlib.emu_replay_map(frame, delta, n, payload.reshape(-1))
        wrong0 = embed_differs(blocks, payload, n, delta, 0.0)
        bad = ((replayed if it < 20 else False) | wrong0) & ~corpus_mask
        if not bad.any():
            break
        index[bad] = rng.integers(0, FILLER, int(bad.sum())).astype(np.uint8)
    else:
        raise RuntimeError(name + ": filler does not settle")
    assert replayed[positions].all()          # every corpus block is undecided at scale 1
    # the stars in the frame's context (the payload window of each block) are the searched ones
    for i in range(0, len(positions), 37):
        assert embed_star(blocks[positions[i]], payload[positions[i]], n, delta) == stars[i]
    ref, used = orc.batch_embed(frame[None], delta, payload.reshape(-1), n)
    assert used == payload.size
    emu, _ = testlib.emu_embed(frame, delta, n, payload.reshape(-1), exact=4)
    assert np.array_equal(emu[0], ref[0]), name
    return dict(blocks=corpus, bits=np.packbits(bits.reshape(-1)), positions=positions.astype(np.uint16),
                stars=np.asarray(stars, np.float32), filler=filler, filler_index=index), frame, payload.reshape(-1)


def build_extract(rng, name, n, delta, covers, quick):
    pool, top, rounds, moves = (20000, 8, 1, 16) if quick else (200000, 64, 4, 64)
    corpus, stars = search_extract(rng, n, delta, covers, pool, top, rounds, moves)
    nblk = (H // 8) * (W // 8)
    positions = layout_positions(rng, len(corpus), nblk, 64)
    # filler: never wrong, and never a candidate of step one at scale 1 (hence at any scale below): the kernels take step two
    # for a whole wave when one block is a candidate, which would settle the corpus blocks sharing its wave
    filler = filler_library(rng, FILLER, lambda c: extract_differs(c, n, delta, 0.0) | testlib.emu_tie_candidates(_blocks_to_strip(c), delta, n))
    index = (np.arange(nblk) % FILLER).astype(np.uint8)
    blocks = filler[index]
    blocks[positions] = corpus
    frame = blocks_to_frame(blocks, H, W)
    assert not extract_differs(np.delete(blocks, positions, 0), n, delta, 0.0).any()
    assert np.array_equal(testlib.emu_extract(frame, delta, n), orc.batch_extract_bits(frame[None], delta, n)), name
    return dict(blocks=corpus, positions=positions.astype(np.uint16), stars=np.asarray(stars, np.float32), filler=filler,
                filler_index=index), frame, None


def empirical_err_over_beta(n, delta, count=4000):
    """the largest err / BETA that tools/guard_bound.py measures by random sampling for this row count and delta"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("guard_bound", os.path.join(REPO, "tools", "guard_bound.py"))
    gb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gb)
    gb.CERTIFICATES = np.load(os.path.join(HERE, "guard_certificates.npz"))["log_c2"]
    k = gb.analyse(7 if n <= 7 else 15, verbose=False)
    return max(1.0 / slack for (_, _, _, slack) in gb.empirical(k, count, n, delta))


def main(quick=False):
    rng = np.random.default_rng(SEED)
    covers = cover_blocks()
    arrays, meta = {}, {"seed": SEED, "frame_shape": [H, W], "keep_per_setting": KEEP, "wave_counts": list(WAVE_COUNTS),
                        "embed": {}, "extract": {}}
    for name, n, delta, width in EMBED_SETTINGS:
        empirical = float(empirical_err_over_beta(n, delta))
        r, frame, payload = build_embed(rng, name, n, delta, width, covers, quick, 0.5 * empirical)
        for k, v in r.items():
            arrays[f"{name}/{k}"] = v
        meta["embed"][name] = {"n_ac": n, "delta": delta, "width": width, "blocks": int(len(r["stars"])),
                               "max_s_star": float(r["stars"].max()), "test_scale": test_scale(r["stars"]),
                               "empirical_max_err_over_beta": empirical}
        case = stored(r, name, meta)
        assert np.array_equal(case["frame"], frame) and np.array_equal(case["bits"], payload), name
        print(name, meta["embed"][name], flush=True)
    for name, n, delta in EXTRACT_SETTINGS:
        r, frame, _ = build_extract(rng, name, n, delta, covers, quick)
        for k, v in r.items():
            arrays[f"{name}/{k}"] = v
        meta["extract"][name] = {"n_ac": n, "delta": delta, "blocks": int(len(r["stars"])),
                                 "max_t_star": float(r["stars"].max()), "test_scale": test_scale(r["stars"])}
        assert np.array_equal(stored(r, name, meta)["frame"], frame), name
        print(name, meta["extract"][name], flush=True)
    write_npz(os.path.join(HERE, "guard_corpus.npz"), arrays)
    with open(os.path.join(HERE, "guard_corpus.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    main(quick="--quick" in sys.argv)
