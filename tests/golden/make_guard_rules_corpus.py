"""Writes tests/golden/guard_rules_corpus.npz / guard_rules_corpus.json: the guard-boundary frames of make_guard_corpus.py for
the streaming embed kernels under SVS_NEAREST and SVS_MINMOVE (their own copies of the kernel bodies, their own pooled replay).

Per setting (kernel family x rule) ONE frame of 128 rows, built from two kinds of blocks:

* dense-replay blocks: sampled blocks that the host build of the bodies (tests/hostemu through minmove_lib.host_embed, the library's route and
  rule word, RouteArgs::guard_scale) leaves undecided at guard scale 1.  No search.  Wave k of 64 blocks (128 in the
  two-blocks-per-lane form) holds 1, 8, 31, 32, 33, 64 (128) of them at random lanes, every further wave one: the wave
  worklist and the pooled 8-lane replay run with one entry, full, half full and across the 32 / 33 split under a rule.
* boundary blocks: up to 64 blocks with s* > 0 UNDER THE RULE (s* as in make_guard_corpus.py: the largest guard scale at
  which the cheap path keeps the block and its pixels differ from the exact arithmetic), found by that file's bisection and
  hill-climb on the shim.  They are undecided at scale 1 by construction and sit among the dense-replay blocks.

Every other block is filler: decided at scale 1, cheap result right at scale 0, all-zero payload bits.

The steps of the table are 16 and more: below 6.69 every minimum-move band is 0 and the rule is the nearest one; at 16 and
above a good share of coefficients stays untouched (change exactly 0), the case the guard argument of csrc/svs_block.hpp singles
out.  `left_alone_blocks` counts the undecided blocks of a MINMOVE setting that hold such a coefficient (at least a quarter).
Two more NEAREST settings repeat the committed reference corpus's (n = 3, delta = 8) and (n = 10, delta = 8): a reference-rule
block whose change vector under NEAREST equals its reference change keeps its s* exactly, so those blocks of guard_corpus.npz
start the hill-climb there (and tests/test_guard_rules_cpu.py asserts the carry-over for the whole reference corpus).

The floor of a setting's max s* is HALF the committed max_s_star of the same kernel family in guard_corpus.json - the reference
corpus, not the code under test: the rules move a coefficient by at most delta where BETA's KD term assumes 1.5 delta, so an s*
up to a third lower is expected, the rest is margin for the smaller search (pools of POOL blocks, at most ATTEMPTS of them,
where make_guard_corpus.py takes 800 000 and a long climb).  A setting that stays below is written with what it reached and
`below_floor`: true.

One worker process per setting (--jobs, at most 12); each setting draws from its own child of one SeedSequence, so both files
come out byte for byte whatever the worker count.  Wall times cannot be part of reproducible bytes as measured, so the JSON
carries the times of the run that wrote the committed files (RECORDED_WALL_S below; a run prints its own):
  full run, 8 workers on 8 cores: 15 s in all, 2 to 11 s per setting.

CPU only.  `python tests/golden/make_guard_rules_corpus.py` reproduces both files; `--quick --out DIR` (and `--only NAME,NAME`) is the small run of the
determinism test.
"""
import json
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"), os.path.join(REPO, "tests"), REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_guard_corpus as ref_gen  # noqa: E402
import minmove_lib as ml  # noqa: E402
import nearest_lib as nl  # noqa: E402
from make_guard_corpus import (FILLER, WAVE_COUNTS, bisect_star, blocks_to_frame, candidate_blocks, cover_blocks,  # noqa: E402,F401
                               filler_library, frame_to_blocks, hill_climb, layout_positions, test_scale, write_npz)

SEED = 20261018
H = 128
KEEP = 64             # boundary blocks per setting
POOL, ATTEMPTS, CLIMB_TOP, ROUNDS, MOVES = 200000, 3, 32, 8, 96
QUICK = (4000, 1, 4, 1, 8)
DENSE_BATCH = 8192

# (family, n, delta, width, the committed setting whose max_s_star halves into the floor)
FAMILIES = [
    ("row1_two_blocks_per_lane", 3, 16.0, 960, "row1_two_blocks_per_lane"),
    ("row1_one_block_per_lane", 7, 20.0, 952, "row1_one_block_per_lane"),      # 119 blocks per row
    ("row1_double", 5, 20.3, 960, "row1_double"),
    ("row2_worklist", 9, 16.0, 960, "row2_worklist"),
    ("row2_n10", 10, 20.0, 960, "row2_n10"),
    ("row2_parked", 15, 20.3, 960, "row2_parked_double"),
]
# the committed reference settings repeated under NEAREST: (name, n, delta, width, floor family = carry-over source)
CARRIED = [
    ("row1_two_blocks_per_lane_d8", 3, 8.0, 960, "row1_two_blocks_per_lane"),
    ("row2_n10_d8", 10, 8.0, 960, "row2_n10"),
]
QM_NAMES = {ml.QM_F32: "float32", ml.QM_DOUBLE: "double", ml.QM_POW2: "pow2"}
# setting -> seconds of the run that wrote the committed files (8 workers on 8 cores), and that run's total
RECORDED_WALL_S = {
    "row1_two_blocks_per_lane__nearest": 6,
    "row1_two_blocks_per_lane__minmove": 5,
    "row1_one_block_per_lane__nearest": 8,
    "row1_one_block_per_lane__minmove": 8,
    "row1_double__nearest": 6,
    "row1_double__minmove": 6,
    "row2_worklist__nearest": 10,
    "row2_worklist__minmove": 11,
    "row2_n10__nearest": 9,
    "row2_n10__minmove": 8,
    "row2_parked__nearest": 4,
    "row2_parked__minmove": 4,
    "row1_two_blocks_per_lane_d8__nearest": 2,
    "row2_n10_d8__nearest": 4,
}
RECORDED_TOTAL_WALL_S = 15


def settings():
    """-> list of dict(name, family, rule, n_ac, delta, width, floor_of, carry)"""
    out = []
    for fam, n, delta, width, floor_of in FAMILIES:
        for rule in ("nearest", "minmove"):
            out.append(dict(name=f"{fam}__{rule}", family=fam, rule=rule, n_ac=n, delta=delta, width=width,
                            floor_of=floor_of, carry=None))
    for name, n, delta, width, src in CARRIED:
        out.append(dict(name=name + "__nearest", family=src, rule="nearest", n_ac=n, delta=delta, width=width, floor_of=src,
                        carry=src))
    return out


def rule_kw(rule):
    return dict(minmove=rule == "minmove", nearest=rule == "nearest")


def model(frame, delta, n, bits, rule):
    """the pixel reference: the NumPy model of the rule (nearest_lib / minmove_lib), not the shim"""
    if rule == "minmove":
        return ml.model_batch(frame[None], delta, bits, n)[0][0]
    return nl.model_batch(frame[None], delta, bits, n)[0][0]


# ---- s* under a rule, on the shim ---------------------------------------------------------------------------------------
def rule_differs(blocks, bits, n, delta, rule, scale):
    """bool per block: the streaming body's output at guard `scale` differs from the exact arithmetic under the rule"""
    fr = ref_gen._blocks_to_strip(blocks)
    flat = bits.reshape(-1)
    exact = ml.host_embed(fr, delta, n, flat, pocketfft=True, **rule_kw(rule))[0]
    got = ml.host_embed(fr, delta, n, flat, guard_scale=scale, **rule_kw(rule))[0]
    return (ref_gen._strip_to_blocks(got) != ref_gen._strip_to_blocks(exact)).reshape(len(blocks), -1).any(1)


def rule_star(block, bits, n, delta, rule):
    return bisect_star(lambda s: bool(rule_differs(block[None], bits[None], n, delta, rule, s)[0]))


def undecided(blocks, bits, n, delta, rule):
    """bool per block: the guard hands the block to the exact replay at scale 1"""
    _, _, info = ml.host_embed(ref_gen._blocks_to_strip(blocks), delta, n, bits.reshape(-1), replay_map=True, **rule_kw(rule))
    return info["replay_map"]


def nearest_change_is_reference_change(blocks, bits, n, delta):
    """bool per block: every wrong-parity payload coefficient already moves to the nearer side under the reference rule, so
    the change vector under SVS_NEAREST is the reference's (oracle arithmetic)"""
    from oracle import qim_dct_oracle as orc
    coef = orc._fwd(np.float32(blocks).reshape(1, -1, 8, 8)).reshape(len(blocks), 64)[:, 1:n + 1]
    q = orc._quant_index(coef, delta)
    use = bits.astype(np.int64)
    wrong = (q & 1) != use
    c0 = orc._requantised(q, delta)
    ref_step = np.where(use == 1, 1, -1)
    step = np.where(coef > c0, 1, np.where(coef < c0, -1, ref_step))
    return ~(wrong & (step != ref_step)).any(1)


def reference_corpus_blocks(name):
    """(blocks, bits [K, n], stars) of one embed setting of the committed reference corpus"""
    meta = json.load(open(os.path.join(HERE, "guard_corpus.json")))
    arrays = np.load(os.path.join(HERE, "guard_corpus.npz"))
    n = meta["embed"][name]["n_ac"]
    blocks = arrays[name + "/blocks"]
    bits = np.unpackbits(arrays[name + "/bits"], count=len(blocks) * n).reshape(-1, n)
    return blocks, bits, arrays[name + "/stars"], meta["embed"][name]


def best(blocks, bits, stars, keep=KEEP):
    order = np.argsort(-np.asarray(stars), kind="stable")
    seen, out = set(), []
    for i in order:
        key = blocks[i].tobytes() + bits[i].tobytes()
        if key not in seen and stars[i] > 0:
            seen.add(key)
            out.append(i)
        if len(out) == keep:
            break
    out = np.array(out, np.int64)
    return blocks[out], bits[out], np.asarray(stars, np.float64)[out]


def search(rng, s, covers, pool, top, rounds, moves, start=None):
    n, delta, rule = s["n_ac"], s["delta"], s["rule"]
    blocks = candidate_blocks(rng, pool, covers)
    bits = rng.integers(0, 2, (pool, n)).astype(np.uint8)
    idx = np.flatnonzero(rule_differs(blocks, bits, n, delta, rule, 0.0))
    stars = np.array([rule_star(blocks[i], bits[i], n, delta, rule) for i in idx], np.float64)
    blocks, bits = blocks[idx], bits[idx]
    if start is not None:
        blocks, bits, stars = (np.concatenate([start[0], blocks]), np.concatenate([start[1], bits]), np.concatenate([start[2], stars]))
    order = np.argsort(-stars, kind="stable")
    blocks, bits, stars = blocks[order], bits[order], stars[order]
    if len(blocks):
        t = slice(0, top)
        blocks[t], stars[t] = hill_climb(rng, blocks[t], bits[t], stars[t], lambda b, p: rule_star(b, p, n, delta, rule),
                                         lambda b, p: rule_differs(b, p, n, delta, rule, 0.0), rounds, moves)
    return best(blocks, bits, stars)


def dense_blocks(rng, s, covers, count):
    """`count` sampled blocks (and payload bits) that the shim leaves undecided at scale 1"""
    n, delta, rule = s["n_ac"], s["delta"], s["rule"]
    got_b, got_p, have = [], [], 0
    q = DENSE_BATCH // 6
    low = np.r_[0:q, 2 * q:3 * q, 4 * q:5 * q]      # the smooth, near-flat and structured classes: they compress
    while have < count:
        blocks = candidate_blocks(rng, DENSE_BATCH, covers)[low]
        bits = rng.integers(0, 2, (len(blocks), n)).astype(np.uint8)
        u = undecided(blocks, bits, n, delta, rule)
        got_b.append(blocks[u])
        got_p.append(bits[u])
        have += int(u.sum())
    return np.concatenate(got_b)[:count], np.concatenate(got_p)[:count]


def left_alone(frame, bits, s):
    """bool per block: MINMOVE leaves at least one payload coefficient of the block exactly where it is (model arithmetic)"""
    stats = {}
    ml.model_embed(frame, s["delta"], bits, s["n_ac"], stats=stats)
    same = (stats["new"] == stats["c"]).reshape(-1, s["n_ac"])
    return same.any(1)


def case(arrays, meta, name):
    """one setting as the tests rebuild it -> dict(frame, bits, positions, stars)"""
    m = meta["settings"][name]
    h, w = meta["height"], m["width"]
    blocks = arrays[name + "/filler"][arrays[name + "/filler_index"]]
    positions = arrays[name + "/positions"].astype(np.int64)
    blocks[positions] = arrays[name + "/blocks"]
    n = m["n_ac"]
    bits = np.zeros((blocks.shape[0], n), np.uint8)
    bits[positions] = np.unpackbits(arrays[name + "/bits"], count=len(positions) * n).reshape(-1, n)
    return dict(frame=blocks_to_frame(blocks, h, w), bits=bits.reshape(-1), positions=positions, stars=arrays[name + "/stars"])


def wave_of(s):
    return 128 if s["family"] == "row1_two_blocks_per_lane" else 64


def wave_counts(positions, nblk, wave):
    return np.bincount(positions // wave, minlength=-(-nblk // wave)).tolist()


def build(job):
    s, child, quick = job
    t0 = time.time()
    rng = np.random.default_rng(child)
    n, delta, rule, width = s["n_ac"], s["delta"], s["rule"], s["width"]
    pool, attempts, top, rounds, moves = QUICK if quick else (POOL, ATTEMPTS, CLIMB_TOP, ROUNDS, MOVES)
    covers = cover_blocks()
    committed = json.load(open(os.path.join(HERE, "guard_corpus.json")))["embed"][s["floor_of"]]["max_s_star"]
    floor = 0.5 * committed

    # boundary blocks
    start, carried = None, 0
    if s["carry"]:
        cb, cp, cs, cm = reference_corpus_blocks(s["carry"])
        assert cm["n_ac"] == n and cm["delta"] == delta
        keep = nearest_change_is_reference_change(cb, cp, n, delta)
        start = (cb[keep], cp[keep], cs[keep].astype(np.float64))
        carried = int(keep.sum())
    corpus = (np.zeros((0, 8, 8), np.uint8), np.zeros((0, n), np.uint8), np.zeros(0))
    pools = []
    for attempt in range(attempts):
        more = search(rng, s, covers, pool, top, rounds, moves, start if attempt == 0 else None)
        corpus = best(np.concatenate([corpus[0], more[0]]), np.concatenate([corpus[1], more[1]]), np.concatenate([corpus[2], more[2]]))
        pools.append(pool)
        if len(corpus[2]) and corpus[2].max() >= floor:
            break
    star_blocks, star_bits, stars = corpus

    # layout: every wave of the frame holds undecided blocks
    wave = wave_of(s)
    nblk = (H // 8) * (width // 8)
    counts = list(WAVE_COUNTS) + ([128] if wave == 128 else [])
    total = sum(counts) + (nblk // wave - len(counts))
    positions = layout_positions(rng, total, nblk, wave)
    d_blocks, d_bits = dense_blocks(rng, s, covers, total - len(stars))
    und_blocks = np.concatenate([star_blocks, d_blocks])
    und_bits = np.concatenate([star_bits, d_bits])
    und_stars = np.concatenate([stars, np.zeros(len(d_blocks))])
    wrong0 = np.flatnonzero(rule_differs(d_blocks, d_bits, n, delta, rule, 0.0))       # a sampled block may have a star too
    for i in wrong0:
        und_stars[len(stars) + i] = rule_star(d_blocks[i], d_bits[i], n, delta, rule)
    max_star = float(und_stars.max())
    shuffle = rng.permutation(total)
    und_blocks, und_bits, und_stars = und_blocks[shuffle], und_bits[shuffle], und_stars[shuffle]

    zeros = lambda c: np.zeros((len(c), n), np.uint8)
    filler = filler_library(rng, FILLER, lambda c: rule_differs(c, zeros(c), n, delta, rule, 0.0) | undecided(c, zeros(c), n, delta, rule))
    index = (np.arange(nblk) % FILLER).astype(np.uint8)
    arrays = dict(blocks=und_blocks, bits=np.packbits(und_bits.reshape(-1)), positions=positions.astype(np.uint16),
                  stars=np.asarray(und_stars, np.float32), filler=filler, filler_index=index)

    # what the tests will see
    blocks = filler[index]
    blocks[positions] = und_blocks
    payload = np.zeros((nblk, n), np.uint8)
    payload[positions] = und_bits
    frame, flat = blocks_to_frame(blocks, H, width), payload.reshape(-1)
    want = model(frame, delta, n, flat, rule)
    got, used, info = ml.host_embed(frame, delta, n, flat, replay_map=True, **rule_kw(rule))
    assert used == flat.size and np.array_equal(got[0], want), s["name"]
    mask = np.zeros(nblk, bool)
    mask[positions] = True
    assert np.array_equal(info["replay_map"], mask), s["name"]
    assert not rule_differs(blocks[~mask], payload[~mask], n, delta, rule, 0.0).any(), s["name"]
    assert np.array_equal(np.float32(und_stars).astype(np.float64), und_stars)          # float32 scales from the bisection
    meta = dict(family=s["family"], rule=rule, n_ac=n, delta=delta, width=width, quantiser=QM_NAMES[info["qm"]], wave=wave,
                undecided=int(total), undecided_per_wave=wave_counts(positions, nblk, wave),
                boundary_blocks=int((und_stars > 0).sum()), max_s_star=max_star, floor=floor, floor_of=s["floor_of"],
                below_floor=bool(max_star < floor), test_scale=test_scale(und_stars[und_stars > 0]) if max_star > 0 else None,
                pools=pools, carried_over=carried if s["carry"] else None,
                wall_time_s=None if quick else RECORDED_WALL_S.get(s["name"]))
    if rule == "minmove":
        alone = left_alone(frame, flat, s)[positions]
        meta["left_alone_blocks"] = int(alone.sum())
        assert 4 * meta["left_alone_blocks"] >= total, s["name"]
    return s["name"], arrays, meta, time.time() - t0


def main(quick=False, jobs=None, out=HERE, only=None):
    """only: names of the settings to build (each keeps the seed of its place in the whole list)"""
    t0 = time.time()
    todo = settings()
    children = np.random.SeedSequence(SEED).spawn(len(todo))
    work = [(s, c, quick) for s, c in zip(todo, children) if only is None or s["name"] in only]
    jobs = min(12, len(work), jobs or os.cpu_count() or 1)
    if jobs == 1:
        results = [build(w) for w in work]
    else:
        with multiprocessing.get_context("spawn").Pool(jobs) as p:
            results = p.map(build, work, chunksize=1)
    arrays, meta = {}, {"seed": SEED, "height": H, "keep_per_setting": KEEP, "wave_counts": list(WAVE_COUNTS), "quick": bool(quick),
                        "total_wall_time_s": None if quick else RECORDED_TOTAL_WALL_S, "settings": {}}
    for name, arr, m, wall in results:
        for k, v in arr.items():
            arrays[f"{name}/{k}"] = v
        meta["settings"][name] = m
        print(name, f"{wall:.0f} s", {k: m[k] for k in ("undecided", "boundary_blocks", "max_s_star", "floor", "below_floor", "pools")},
              flush=True)
    os.makedirs(out, exist_ok=True)
    write_npz(os.path.join(out, "guard_rules_corpus.npz"), arrays)
    with open(os.path.join(out, "guard_rules_corpus.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"total {time.time() - t0:.0f} s with {jobs} workers", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(quick="--quick" in a, jobs=int(a[a.index("--jobs") + 1]) if "--jobs" in a else None,
         out=a[a.index("--out") + 1] if "--out" in a else HERE, only=a[a.index("--only") + 1].split(",") if "--only" in a else None)
