"""Writes tests/golden/tie_corpus.npz / tie_corpus.json: uint8 8x8 blocks whose float32 coefficient c = _fwd(block)[k], as the
oracle (pocketfft) computes it, sits where the quantiser q = int(round(c / delta)) has code that runs nowhere else: on a
rounding tie, one float32 next to it, inside the window of the kernels' division fallback, or exactly on a lattice point.
The payload coefficients are the ones with an IRRATIONAL basis (never flat index 4, 32 or 36, whose ties are exact eighths
and which the suite covers by construction): a coefficient reaches a kernel only through pixels, and ordinary content puts
none of these near a tie (tests/test_tie_corpus_cpu.py counts 0 in 4 800 blocks).

Classes, all decided on float32 values (quot = float32(c) / float32(delta), t = c * fl(1 / float32(delta))):
  tie       quot is exactly a half-integer.  Kept balanced over the parity of floor(quot) - half-even rounds down in some
            blocks and up in others - and over the sign of c.
  below     quot is the float32 immediately below a half-integer; `above`: immediately above.
  fallback  (delta not a power of two) | |t - rint(t)| - 1/2 | <= |t| 2^-21: quant_index / qim_change evaluate the IEEE
            division; the block is in none of the classes above.
  lattice   c == fl(q delta) exactly as _requantised forms it, q != 0; `bit` = 1 - (q & 1) is the payload bit the tests
            give that coefficient: the third arm of the nearest rule.
  dither_tie  the block sits at raster position `i` of frame `f` of a two-frame call with dither key KEY and first clip
            frame FIRST_FRAME; cq = fl(c - d(KEY, FIRST_FRAME + f, i, k)) is a tie, below or above (`sub`) of delta.
  diverge   (delta not a power of two) rint(t) != rint(quot): the reciprocal shortcut alone would be wrong.  t is within
            3 ulps of quot, so these are ties and their float32 neighbours (`sub`); a search that reaches ties finds them
            by the dozen.  The JSON counts them per mode (`diverge_found` of `diverge_examined` float32-confirmed
            candidates); nothing is padded.  Blocks of the other classes carry the flag `diverge` as well.

Search.  Per coefficient k one job: base blocks = uniform noise in [16, 240) plus a random multiple of sign(basis_k) - a
strong pattern under the noise makes |c| a few hundred, and the window of a class is an ulp or two of c per period delta -,
and for every base block the 384 variants with ONE pixel changed by +-1, +-2, +-3.  The variants' coefficients are
c + m basis_k(x) in float64, no transform; the ones within TOL of a tie or a lattice point of a delta are built, run through
the oracle and classified on its float32 c.  |basis_k| takes the same value at several pixels, so two variants of one base
block often land on the same float32 c: a job keeps ONE block per (delta, c), whatever its class - a second block with the
same coefficient shows the quantiser nothing new.  A job stops at CHUNKS chunks or when every (delta, class) of its k is full.
Dither blocks: per (delta, k in {1, 10}) DITHER_POOL base blocks through the oracle, against the dither of every slot
(f, i < DITHER_SLOTS); a slot of a delta is given away once.

Stored per delta as one strip uint8 [8, 8 K] (`d<delta>/strip`); the JSON lists the K blocks of each strip in order: class, k,
delta, c as float32 hex, parity of floor(quot), sign, and bit / i, f, sub where they apply.  tests/tie_lib.py
(frames_for) lays the strips of a setting out in frames: a block's class does not depend on where it sits, except for the
dither blocks, which go to their slot.

One worker process per job (--jobs, at most 16); every job draws from its own child of one SeedSequence and the results are
merged in job order, so both files come out byte for byte whatever the worker count.  Wall times cannot be part of
reproducible bytes as measured: the JSON carries the time of the run that wrote the committed files (RECORDED_* below; a
run prints its own).

CPU only; oracle/ and NumPy / SciPy only.  `python tests/golden/make_tie_corpus.py` reproduces both files;
`--only k1,k9 --out DIR` builds the named jobs alone (each keeps the seed of its place in the whole list).
"""
import io
import json
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import qim_dct_oracle as orc  # noqa: E402

SEED = 20261019
KEY = 0x7A11C0DE5EED0001          # the dither key of the tests' dithered calls
FIRST_FRAME = 5                   # clip frame of frame 0 of those calls
DITHER_SLOTS = 68                 # i < 68: four block rows of the narrower test frame (17 blocks per row)
DITHER_KS = (1, 10)
DITHER_POOL = 65536
DITHER_KEEP = 4                   # per (delta, k)
BASES, CHUNKS = 16384, 12         # base blocks per chunk, chunks per job at most
TOL = 3e-4                        # float64 prefilter: |c64 - target|; pocketfft's float32 c is within about 1e-4 of c64
CONFIRM = 8192                    # candidates per (chunk, delta) run through the oracle at most
KEEP = {"tie": 6, "below": 2, "above": 2, "fallback": 2, "diverge": 2, "lattice": 2}
STEPS = (-3, -2, -1, 1, 2, 3)

# family -> (n_ac values of its frames, the tie coefficients); none of 4, 32, 36
FAMILIES = {"row1": ((3, 7), (1, 2, 3, 5, 7)), "row2": ((10, 15), (8, 9, 10, 12, 15)), "row8": ((20, 63), (17, 27, 63))}
DELTAS = (8, 0.25, 20, 12.5, 7.3)             # every family
DELTAS_ROW8 = (0.1,)                           # and the exact route's own double step
MODES = {8: "pow2", 0.25: "pow2", 20: "f32", 12.5: "f32", 7.3: "double", 0.1: "double"}
# seconds of the run that wrote the committed files, and its worker count
RECORDED_TOTAL_WALL_S = 26
RECORDED_WORKERS = 8


def family_of(k):
    return next(f for f, (_, ks) in FAMILIES.items() if k in ks)


def deltas_of(k):
    return DELTAS + (DELTAS_ROW8 if family_of(k) == "row8" else ())


def tag(delta):
    return "d" + repr(delta)


# ---- float32 classes ---------------------------------------------------------------------------------------------------
def _is_half(x):
    return np.isfinite(x) & (np.floor(x) + np.float32(0.5) == x)


def classify(c, delta):
    """c float32 [N] -> dict of arrays: tie, below, above, fallback, diverge, lattice (bool), parity (of floor(quot)), q"""
    c = np.asarray(c, np.float32)
    df = np.float32(delta)
    quot = c / df
    assert quot.dtype == np.float32
    up, down = np.nextafter(quot, np.float32(np.inf)), np.nextafter(quot, np.float32(-np.inf))
    tie, below, above = _is_half(quot), _is_half(up), _is_half(down)
    q = orc._quant_index(c, delta)
    lattice = (orc._requantised(q, delta) == c) & (q != 0)
    if MODES[delta] == "pow2":
        fallback = np.zeros(c.shape, bool)
        diverge = np.zeros(c.shape, bool)
    else:
        t = c * (np.float32(1.0) / df)
        r = np.rint(t)
        miss = np.abs(np.abs(t - r) - np.float32(0.5))
        assert miss.dtype == np.float32
        fallback = (miss <= np.abs(t) * np.float32(2.0 ** -21)) & ~(tie | below | above)
        diverge = r != np.rint(quot)
    return dict(tie=tie, below=below, above=above, fallback=fallback, diverge=diverge, lattice=lattice,
                parity=(np.floor(quot).astype(np.int64) & 1), q=q)


def coefficient(blocks, k):
    """the oracle's float32 c_k of uint8 blocks [N, 8, 8]"""
    return orc._fwd(np.float32(blocks).reshape(1, -1, 8, 8)).reshape(-1, 64)[:, k]


def basis(k):
    """float64 [64]: the orthonormal 8x8 DCT-II basis function of flat index k = 8 u + v over pixels (y, x)"""
    u, v = divmod(k, 8)
    x = np.arange(8)
    a = lambda w: np.sqrt((1.0 if w == 0 else 2.0) / 8.0) * np.cos((2 * x + 1) * w * np.pi / 16.0)   # noqa: E731
    return np.outer(a(u), a(v)).reshape(64)


# ---- the dither, restated (csrc/svs_block.hpp; tests/dither_lib.py holds the product to the same form) -------------------
def _lb(h):
    m = np.uint64(0xFFFFFFFF)
    h = h & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & m
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & m
    return h ^ (h >> np.uint64(16))


def dither(key, t, n_blocks, k, delta):
    """float32 [n_blocks]: d of clip frame t, raster blocks 0 .. n_blocks - 1, flat coefficient k"""
    seed = _lb(_lb(np.uint64((key >> 32) ^ 0x85EBCA6B)) ^ np.uint64(key & 0xFFFFFFFF))
    s_t = _lb(seed ^ np.uint64(t))
    s_b = _lb(s_t + np.arange(n_blocks, dtype=np.uint64) * np.uint64(0x9E3779B1))
    h = _lb(s_b ^ np.uint64((k * 0x632BE5AB) & 0xFFFFFFFF))
    r = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return r * np.float32(delta)


# ---- search ------------------------------------------------------------------------------------------------------------
def base_blocks(rng, count, k):
    """uniform noise in [16, 240) plus amp * sign(basis_k), amp uniform in -100 .. 100 per block, clipped to [4, 251]"""
    noise = rng.integers(16, 240, (count, 64)).astype(np.int16)
    amp = rng.integers(-100, 101, (count, 1)).astype(np.int16)
    return np.clip(noise + amp * np.sign(basis(k)).astype(np.int16), 4, 251).astype(np.uint8)


def record(cls, k, delta, c, info, j, **extra):
    return dict({"class": cls, "k": int(k), "delta": delta, "c": float(c).hex(), "floor_parity": int(info["parity"][j]),
                 "sign": int(np.sign(c)), "diverge": bool(info["diverge"][j])}, **extra)


def search_k(job):
    k, child = job
    t0 = time.time()
    rng = np.random.default_rng(child)
    b = basis(k)
    steps = np.array(STEPS, np.float64)
    shift = (b[:, None] * steps[None, :]).reshape(-1)                 # [384]: pixel x, step m -> m b(x)
    deltas = deltas_of(k)
    found = {d: {cls: [] for cls in KEEP} for d in deltas}            # (block bytes, record)
    seen = set()                                                      # block bytes
    seen_c = set()                                                    # (delta, float32 c): one block per quantiser input
    examined = {d: 0 for d in deltas}
    diverge_seen = {d: 0 for d in deltas}
    chunks = 0

    def full(d, cls):
        have = found[d][cls]
        if cls in ("fallback", "diverge") and MODES[d] == "pow2":
            return True
        if cls == "lattice":
            return len(have) >= 4 * KEEP[cls]                           # a pool to take both payload bits from
        if cls != "tie":
            return len(have) >= KEEP[cls]
        combos = {(r["floor_parity"], r["sign"]) for _, r in have}
        return len(have) >= 4 * KEEP[cls] and len(combos) == 4         # a pool to balance from

    while chunks < CHUNKS and not all(full(d, cls) for d in deltas for cls in KEEP):
        chunks += 1
        bases = base_blocks(rng, BASES, k)
        c64 = bases.astype(np.float64) @ b
        cand = c64[:, None] + shift[None, :]                          # [BASES, 384]
        for d in deltas:
            if all(full(d, cls) for cls in KEEP):
                continue
            tol = min(TOL, float(d) / 8)
            x = cand / float(d)
            near = np.abs(x * 2 - np.rint(x * 2)) * (float(d) / 2) < tol          # within tol of a multiple of delta / 2
            bi, vi = np.nonzero(near)
            bi, vi = bi[:CONFIRM], vi[:CONFIRM]
            blocks = bases[bi].copy()
            px, st = vi // len(STEPS), vi % len(STEPS)
            blocks[np.arange(len(bi)), px] = (blocks[np.arange(len(bi)), px].astype(np.int16) + np.array(STEPS, np.int16)[st]).astype(np.uint8)
            blocks = blocks.reshape(-1, 8, 8)
            c = coefficient(blocks, k)
            info = classify(c, d)
            examined[d] += len(c)
            diverge_seen[d] += int(info["diverge"].sum())
            for cls in KEEP:
                if full(d, cls):
                    continue
                for j in np.flatnonzero(info[cls]):
                    key, key_c = blocks[j].tobytes(), (d, c[j].tobytes())
                    if key in seen or key_c in seen_c or full(d, cls):
                        continue
                    seen.add(key)
                    seen_c.add(key_c)
                    extra = {"bit": int(1 - (info["q"][j] & 1))} if cls == "lattice" else {}
                    if cls == "diverge":
                        extra = {"sub": "tie" if info["tie"][j] else ("below" if info["below"][j] else "above")}
                    found[d][cls].append((blocks[j].copy(), record(cls, k, d, c[j], info, j, **extra)))
    out = {}
    for d in deltas:
        keep = []
        ties = found[d]["tie"]
        combos = sorted({(r["floor_parity"], r["sign"]) for _, r in ties})
        queues = {cb: [e for e in ties if (e[1]["floor_parity"], e[1]["sign"]) == cb] for cb in combos}
        while len(keep) < KEEP["tie"] and any(queues.values()):
            for cb in combos:
                if queues[cb] and len(keep) < KEEP["tie"]:
                    keep.append(queues[cb].pop(0))
        for cls in ("below", "above", "fallback", "diverge"):
            keep += found[d][cls][:KEEP[cls]]
        lat = found[d]["lattice"]
        by_bit = [[e for e in lat if e[1]["bit"] == b] for b in (0, 1)]  # bit 0: the reference direction is -1
        picked = []
        while len(picked) < KEEP["lattice"] and (by_bit[0] or by_bit[1]):
            for q in by_bit:
                if q and len(picked) < KEEP["lattice"]:
                    picked.append(q.pop(0))
        keep += picked
        out[d] = keep
    return k, out, examined, diverge_seen, chunks, time.time() - t0


def search_dither(job):
    """-> list over deltas of (delta, [(block, record)]): the slots (f, i) of one delta are given away once"""
    child, = job
    t0 = time.time()
    rng = np.random.default_rng(child)
    out = []
    for d in DELTAS + DELTAS_ROW8:
        used, keep = set(), []
        for k in DITHER_KS:
            blocks = base_blocks(rng, DITHER_POOL, k).reshape(-1, 8, 8)
            c = coefficient(blocks, k)
            got = 0
            for f in range(2):
                dd = dither(KEY, FIRST_FRAME + f, DITHER_SLOTS, k, d)
                cq = c[:, None] - dd[None, :]
                assert cq.dtype == np.float32
                info = classify(cq.reshape(-1), d)
                hit = (info["tie"] | info["below"] | info["above"]).reshape(cq.shape)
                for j, i in zip(*np.nonzero(hit)):
                    if got >= (DITHER_KEEP + 1) // 2 * (f + 1) or (f, int(i)) in used or ("block", k, int(j)) in used:
                        continue
                    flat = j * DITHER_SLOTS + i
                    sub = "tie" if info["tie"][flat] else ("below" if info["below"][flat] else "above")
                    own = classify(c[j:j + 1], d)
                    if own["tie"][0] or own["below"][0] or own["above"][0] or own["lattice"][0]:
                        continue
                    used.add((f, int(i)))
                    used.add(("block", k, int(j)))
                    got += 1
                    rec = record("dither_tie", k, d, c[j], own, 0, i=int(i), f=int(f), sub=sub, cq=float(cq[j, i]).hex(),
                                 cq_floor_parity=int(info["parity"][flat]))
                    keep.append((blocks[j].copy(), rec))
        out.append((d, keep))
    return out, time.time() - t0


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


def _run(job):
    return search_k(job[1:]) if job[0] == "k" else search_dither(job[1:])


def main(jobs=None, out=HERE, only=None):
    t0 = time.time()
    ks = [k for _, (_, fam_ks) in FAMILIES.items() for k in fam_ks]
    children = np.random.SeedSequence(SEED).spawn(len(ks) + 1)
    names = [f"k{k}" for k in ks] + ["dither"]
    work = [("k", k, c) for k, c in zip(ks, children)] + [("dither", children[-1])]
    work = [w for w, name in zip(work, names) if only is None or name in only]
    jobs = min(16, len(work), jobs or os.cpu_count() or 1)
    if jobs == 1:
        results = [_run(w) for w in work]
    else:
        with multiprocessing.get_context("spawn").Pool(jobs) as p:
            results = p.map(_run, work, chunksize=1)
    per_delta = {d: [] for d in DELTAS + DELTAS_ROW8}
    search = {}
    diverge = {m: {"examined": 0, "found": 0} for m in ("f32", "double")}
    for w, res in zip(work, results):
        if w[0] == "k":
            k, found, examined, diverge_seen, chunks, wall = res
            for d, keep in found.items():
                per_delta[d] += keep
                if MODES[d] != "pow2":
                    diverge[MODES[d]]["examined"] += examined[d]
                    diverge[MODES[d]]["found"] += diverge_seen[d]
            search[f"k{k}"] = dict(chunks=chunks, base_blocks=chunks * BASES, variants_per_base=64 * len(STEPS),
                                   confirmed={tag(d): examined[d] for d in found})
            print(f"k{k}", f"{wall:.0f} s", chunks, "chunks", {tag(d): len(v) for d, v in found.items()}, flush=True)
        else:
            found, wall = res
            for d, keep in found:
                per_delta[d] += keep
            search["dither"] = dict(pool=DITHER_POOL, slots=DITHER_SLOTS, frames=2)
            print("dither", f"{wall:.0f} s", {tag(d): len(v) for d, v in found}, flush=True)
    arrays, blocks_meta = {}, {}
    for d, keep in per_delta.items():
        if keep:
            arrays[tag(d) + "/strip"] = np.concatenate([b for b, _ in keep], axis=1)
            blocks_meta[tag(d)] = [r for _, r in keep]
    mode_of_tag = {tag(d): m for d, m in MODES.items()}
    kept_diverge = {m: sum(r["diverge"] for d, v in blocks_meta.items() for r in v if mode_of_tag[d] == m) for m in ("f32", "double")}
    whole = only is None
    meta = dict(seed=SEED, key=KEY, first_frame=FIRST_FRAME, dither_slots=DITHER_SLOTS, keep=KEEP, dither_keep=DITHER_KEEP, tol=TOL,
                families={f: dict(n_acs=list(n), ks=list(k)) for f, (n, k) in FAMILIES.items()},
                deltas=list(DELTAS), deltas_row8=list(DELTAS_ROW8), modes={tag(d): m for d, m in MODES.items()},
                search=search, diverge_examined={m: v["examined"] for m, v in diverge.items()},
                diverge_found={m: v["found"] for m, v in diverge.items()}, diverge_kept=kept_diverge,
                total_wall_time_s=RECORDED_TOTAL_WALL_S if whole else None, workers=RECORDED_WORKERS if whole else None,
                blocks=blocks_meta)
    os.makedirs(out, exist_ok=True)
    write_npz(os.path.join(out, "tie_corpus.npz"), arrays)
    with open(os.path.join(out, "tie_corpus.json"), "w") as f:
        json.dump(meta, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"total {time.time() - t0:.0f} s with {jobs} workers;", sum(len(v) for v in blocks_meta.values()), "blocks", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(jobs=int(a[a.index("--jobs") + 1]) if "--jobs" in a else None, out=a[a.index("--out") + 1] if "--out" in a else HERE,
         only=a[a.index("--only") + 1].split(",") if "--only" in a else None)
