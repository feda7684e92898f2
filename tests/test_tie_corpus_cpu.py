"""CPU tier of the tie corpus (tests/golden/make_tie_corpus.py; GPU tier: test_tie_corpus_gpu.py): real uint8 blocks whose
payload coefficient - one with an irrational basis, never flat index 4, 32 or 36 - sits on a rounding tie of the quantiser,
one float32 next to it, in the window of the division fallback, where the reciprocal shortcut alone is wrong, or exactly on a
lattice point.

* every block's class is recomputed here from the oracle's float32 coefficient, with scalar float32 arithmetic of its own, and
  the minimums per kernel family and quantiser mode are counted;
* one job of the generator is run again and gives the committed blocks and records;
* on the frames of tie_lib.frames_for the host build of the kernel bodies (tests/hostemu) equals the oracle: embed with
  flags 0 (fast), SVS_EXACT_GUARDED and SVS_EXACT_POCKETFFT, extraction of the COVERS (that is where the ties are) in fast
  mode, per block and per wave - inside the streaming delta range guarded extraction is routed exactly as fast is
  (plan_extract), hostemu has no other guarded extract -, and in exact mode;
* the four scalar forms of the quantiser on the corpus coefficients themselves (hostemu's mismatch counters);
* the SVS_NEAREST, SVS_MINMOVE and dither shims equal their NumPy models, `lattice` and `dither_tie` blocks included;
* the suite's usual noise holds no member of any class at k in {1, 2, 3, 8, 9, 10}: why the corpus exists."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dither_lib as dl
import minmove_lib as ml
import nearest_lib as nl
import tie_lib as tl
from oracle import qim_dct_oracle as orc
from testlib import REPO, emu_embed, emu_extract, hostemu

F32 = np.float32
SETTINGS = tl.settings()
IDS = [tl.setting_id(s) for s in SETTINGS]


# ---- the classes, recomputed with scalars ------------------------------------------------------------------------------
def is_half(x):
    return math.isfinite(x) and float(x) * 2 == math.floor(float(x) * 2) and int(math.floor(float(x) * 2)) % 2 == 1


def classes_of(c, delta):
    """c: numpy float32 scalar -> (set of class names, parity of floor(quot))"""
    assert type(c) is F32
    df = F32(delta)
    quot = c / df
    assert type(quot) is F32
    out = set()
    if is_half(quot):
        out.add("tie")
    if is_half(np.nextafter(quot, F32(np.inf))):
        out.add("below")
    if is_half(np.nextafter(quot, F32(-np.inf))):
        out.add("above")
    if tl.MODES[tl.tag(delta)] != "pow2":
        t = c * (F32(1) / df)
        r = np.rint(t)
        miss = abs(abs(t - r) - F32(0.5))
        assert type(miss) is F32
        if miss <= abs(t) * F32(2.0 ** -21) and not out:
            out.add("fallback")
        if r != np.rint(quot):
            out.add("diverge")
    q = int(np.rint(quot))
    c0 = F32(q * int(delta)) if isinstance(delta, int) else F32(float(q) * float(delta))      # _requantised
    if c0 == c and q != 0:
        out.add("lattice")
    return out, int(math.floor(float(quot))) & 1, q


def corpus():
    """(delta, block uint8 [8, 8], record, the oracle's float32 c of the record's k) of every block"""
    for t, records in tl.META["blocks"].items():
        delta = records[0]["delta"]
        blocks, _ = tl.blocks_of(delta)
        coef = orc._fwd(F32(blocks).reshape(1, -1, 8, 8)).reshape(-1, 64)
        for b, r, row in zip(blocks, records, coef):
            yield delta, b, r, row[r["k"]]


def test_every_block_is_in_its_class_by_the_oracle():
    seen = set()
    for delta, block, r, c in corpus():
        assert r["k"] not in (4, 32, 36) and tl.tag(delta) in tl.MODES
        assert float(c).hex() == r["c"], r
        got, parity, q = classes_of(c, delta)
        assert parity == r["floor_parity"] and ("diverge" in got) == r["diverge"] and r["sign"] == (1 if c > 0 else -1), r
        cls = r["class"]
        if cls == "dither_tie":
            assert r["k"] in (1, 10) and 0 <= r["i"] < tl.META["dither_slots"] and r["f"] in (0, 1)
            d = dl.dither_table(tl.KEY, tl.FIRST_FRAME + r["f"], tl.META["dither_slots"], delta)[r["i"], r["k"]]
            cq = c - d
            assert type(cq) is F32 and float(cq).hex() == r["cq"]
            sub, sub_parity, _ = classes_of(cq, delta)
            assert r["sub"] in sub and sub_parity == r["cq_floor_parity"], r
            assert (delta, r["f"], r["i"]) not in seen, "two dither blocks of one delta in one slot"
            seen.add((delta, r["f"], r["i"]))
        else:
            assert cls in got, (r, got)
            if cls == "fallback":
                assert not got & {"tie", "below", "above"}
            if cls == "diverge":
                assert r["sub"] in got
            if cls == "lattice":
                assert r["bit"] == 1 - (q & 1)
        key = (delta, block.tobytes())
        assert key not in seen, "a block twice in one strip"
        seen.add(key)


def test_minimums_per_family_and_quantiser_mode():
    """Counted by DISTINCT quantiser input: two blocks with the same float32 c (c - d for the dither blocks) at one k and
    delta would count once, whatever their class - the second shows the quantiser nothing the first did not - and the
    corpus holds no such pair."""
    count, inputs = {}, {}

    def add(key, value):
        count.setdefault(key, set()).add(value)

    for delta, _, r, _ in corpus():
        mode = tl.MODES[tl.tag(delta)]
        if r["class"] == "dither_tie":
            add(("dither", mode), (r["k"], delta, r["cq"]))
            continue
        mine = (r["k"], delta, r["c"])
        assert mine not in inputs, ("one coefficient twice", r, inputs[mine])
        inputs[mine] = r
        fam = next(f for f, (_, ks) in tl.FAMILIES.items() if r["k"] in ks)
        assert delta in tl.deltas_of(fam)
        add((fam, mode, "ks"), r["k"])
        add((fam, mode, r["class"]), mine)
        if r["class"] == "tie":
            add((fam, mode, "tie", r["floor_parity"]), mine)
            add((fam, mode, "sign", r["sign"]), mine)
        if r["class"] == "lattice":
            add((fam, mode, "bit", r["bit"]), mine)
        if r["diverge"]:
            add(("diverge", mode), mine)
    n = {key: len(v) for key, v in count.items()}
    for fam in tl.FAMILIES:
        for mode in ("pow2", "f32", "double"):
            cell = {key[2:]: v for key, v in n.items() if key[:2] == (fam, mode)}
            what = (fam, mode, cell)
            assert cell[("ks",)] >= 2, what
            assert cell[("tie",)] >= 16 and cell[("tie", 0)] >= 4 and cell[("tie", 1)] >= 4, what
            assert cell[("sign", 1)] >= 1 and cell[("sign", -1)] >= 1, what
            assert cell[("below",)] >= 8 and cell[("above",)] >= 8 and cell[("lattice",)] >= 8, what
            assert cell[("bit", 0)] >= 1 and cell[("bit", 1)] >= 1, what          # both directions of the nearest rule's third arm
            if mode != "pow2":
                assert cell[("fallback",)] >= 8, what
    for mode in ("pow2", "f32", "double"):
        assert n[("dither", mode)] >= 8, mode
    for mode in ("f32", "double"):
        # the JSON's search record says the same: found > 0 of `examined` candidates, nothing padded
        assert n[("diverge", mode)] >= 4 and tl.META["diverge_found"][mode] >= n[("diverge", mode)], mode
        assert tl.META["diverge_kept"][mode] == n[("diverge", mode)] and tl.META["diverge_examined"][mode] > 0


def test_one_job_of_the_generator_gives_the_committed_blocks(tmp_path):
    k = 63
    subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "make_tie_corpus.py"), "--only", f"k{k}", "--out",
                    str(tmp_path), "--jobs", "1"], check=True, capture_output=True, timeout=600)
    import json
    meta = json.load(open(tmp_path / "tie_corpus.json"))
    arrays = np.load(tmp_path / "tie_corpus.npz")
    assert meta["total_wall_time_s"] is None and meta["search"][f"k{k}"] == tl.META["search"][f"k{k}"]
    n = 0
    for t, records in meta["blocks"].items():
        delta = records[0]["delta"]
        blocks, committed = tl.blocks_of(delta)
        mine = [j for j, r in enumerate(committed) if r["k"] == k and r["class"] != "dither_tie"]
        assert [committed[j] for j in mine] == records, t
        assert arrays[t + "/strip"].tobytes() == np.concatenate(list(blocks[mine]), axis=1).tobytes(), t
        n += len(mine)
    assert n >= 60


# ---- the host build of the kernel bodies on the frames -----------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_hostemu_equals_the_oracle_on_the_tie_frames(setting):
    _, n, delta = setting
    for width in tl.WIDTHS:
        frames, where = tl.frames_for(n, delta, width)
        bits = tl.payload_for(frames, where, n)
        want, used = orc.batch_embed(frames, delta, bits, n)
        assert used == bits.size
        for exact in (0, 4, 1):                                         # flags 0 (fast), SVS_EXACT_GUARDED, SVS_EXACT_POCKETFFT
            got, u = emu_embed(frames, delta, n, bits, exact=exact)
            assert u == used and np.array_equal(got, want), (setting, width, exact, tl.blame(where, got, want))
        want_bits = orc.batch_extract_bits(frames, delta, n)           # of the COVER: its coefficients are the ties
        for kw in (dict(), dict(wave=64), dict(exact=True)):
            got = emu_extract(frames, delta, n, **kw)
            assert np.array_equal(got, want_bits), (setting, width, kw, tl.blame(where, got, want_bits, bits_per_block=n))


def test_scalar_quantiser_forms_on_the_corpus_coefficients():
    """quant_index against the IEEE division and qim_change against force_parity of the division, on every c of the corpus
    (and on c - d of the dither blocks), both payload bits.
    What no embed test can see: the DIRECTION in which qim_change rounds a tie.  Half-even and half-up disagree only when
    the tie lies between 2 j and 2 j + 1, and forcing the low bit to the payload bit (or stepping to the nearer side under
    the other rules) maps both to the same index; extract_block_cheap's own rounding of a tie is not observable either, a
    tie being a candidate for the exact replay by definition.  Replacing t + 1.5 * 2^23 by floorf(t + 0.5f) in those two
    bodies therefore changes no output (tried on the host build: this file passes); a wrong division next to the tie does."""
    lib = hostemu()
    for t, records in tl.META["blocks"].items():
        delta = records[0]["delta"]
        c = np.array([float.fromhex(r["c"]) for r in records] + [float.fromhex(r["cq"]) for r in records if "cq" in r], F32)
        assert c.size >= 8
        assert lib.emu_quant_mismatches(c.ctypes.data, c.size, float(delta)) == 0, t
        if delta >= 0.25:                                                 # qim_change: the streaming bodies' delta range
            for bit in (0, 1):
                b = np.full(c.size, bit, np.uint8)
                assert lib.emu_qim_change_mismatches(c.ctypes.data, b.ctypes.data, c.size, float(delta)) == 0, (t, bit)


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_rule_shims_equal_their_models_on_the_tie_frames(setting):
    """SVS_NEAREST and SVS_MINMOVE: the `lattice` blocks carry the bit that differs from their parity, so the third arm of
    c > c0 ? .. : c < c0 ? .. : 2 bit - 1 decides their direction; the model takes the reference's"""
    _, n, delta = setting
    width = tl.WIDTHS[n % 2]
    frames, where = tl.frames_for(n, delta, width)
    bits = tl.payload_for(frames, where, n)
    lattice = [(f, p) for (f, p), r in where.items() if r["class"] == "lattice"]
    assert len(lattice) >= 2
    want_n, used = nl.model_batch(frames, delta, bits, n)
    want_m, _ = ml.model_batch(frames, delta, bits, n)
    ref, _ = orc.batch_embed(frames, delta, bits, n)
    assert used == bits.size and not np.array_equal(want_n, ref)
    for pocketfft in (False, True):
        got = nl.host_embed(frames, delta, n, bits, pocketfft=pocketfft)[0]
        assert np.array_equal(got, want_n), (setting, pocketfft, tl.blame(where, got, want_n))
        got = ml.host_embed(frames, delta, n, bits, pocketfft=pocketfft, nearest=True, minmove=False)[0]
        assert np.array_equal(got, want_n), (setting, pocketfft, tl.blame(where, got, want_n))
        got = ml.host_embed(frames, delta, n, bits, pocketfft=pocketfft)[0]
        assert np.array_equal(got, want_m), (setting, pocketfft, tl.blame(where, got, want_m))


def test_lattice_blocks_take_the_reference_direction_in_the_model():
    """what the previous test compares against: on a lattice block the nearest rule moves as the reference does, in both
    directions (bit 0: down, bit 1: up) - the stego block of the nearest model is the reference's"""
    seen = set()
    for n, delta in ((7, 8), (15, 20), (63, 7.3)):
        frames, where = tl.frames_for(n, delta, tl.WIDTHS[0])
        for (f, p), r in where.items():
            if r["class"] != "lattice":
                continue
            one = tl.to_blocks(frames)[f, p][None]
            bits = np.zeros(n, np.uint8)
            q = int(orc._quant_index(orc._fwd(F32(one)[None])[0, 0].reshape(64)[r["k"]:r["k"] + 1], delta)[0])
            bits[:] = [int(v) & 1 for v in orc._quant_index(orc._fwd(F32(one)[None])[0, 0].reshape(64)[1:n + 1], delta)]
            bits[r["k"] - 1] = r["bit"]
            assert r["bit"] != (q & 1)
            want, _ = orc.batch_embed(one, delta, bits, n)
            assert np.array_equal(nl.model_batch(one, delta, bits, n)[0], want), r
            seen.add(r["bit"])
    assert seen == {0, 1}


@pytest.mark.parametrize("delta", [8, 0.25, 20, 12.5, 7.3, 0.1])
def test_dither_shim_equals_its_model_on_the_dither_ties(delta):
    for n in (3, 10):
        frames, where = tl.frames_for(n, delta, tl.WIDTHS[n % 2])
        slotted = [r for r in where.values() if r["class"] == "dither_tie"]
        assert len(slotted) >= (8 if n == 10 else 4), (delta, n, len(slotted))
        bits = tl.payload_for(frames, where, n)
        want_cover = dl.model_batch_extract(frames, delta, n, key=tl.KEY, first_frame=tl.FIRST_FRAME)
        got_cover, _ = dl.host_extract(frames, delta, n, tl.KEY, tl.FIRST_FRAME)
        assert np.array_equal(got_cover, want_cover), (delta, n, tl.blame(where, got_cover, want_cover, bits_per_block=n))
        for rule in ("reference", "nearest", "minmove"):
            want, used = dl.model_batch_embed(frames, delta, bits, n, rule, key=tl.KEY, first_frame=tl.FIRST_FRAME)
            got, u, _ = dl.host_embed(frames, delta, n, bits, tl.KEY, tl.FIRST_FRAME, rule=rule)
            assert u == used == bits.size and np.array_equal(got, want), (delta, n, rule, tl.blame(where, got, want))
            back, _ = dl.host_extract(got, delta, n, tl.KEY, tl.FIRST_FRAME)
            assert np.array_equal(back, dl.model_batch_extract(want, delta, n, key=tl.KEY, first_frame=tl.FIRST_FRAME))


def test_ordinary_noise_holds_no_member_of_any_class():
    """4 800 blocks of the suite's usual noise (nearest_lib.content: uniform in [16, 240), 480 x 640): no coefficient of the
    headline kernels' k in {1, 2, 3} and {8, 9, 10} is a tie, next to one, in the fallback window, diverging or on a lattice
    point at delta = 8 and 20 - the kernels' code for these cases does not run on such frames."""
    frame = nl.content("noise")
    blocks = tl.to_blocks(frame[None])[0]
    assert blocks.shape[0] == 4800
    coef = orc._fwd(F32(blocks).reshape(1, -1, 8, 8)).reshape(-1, 64)
    for delta in (8, 20):
        for k in (1, 2, 3, 8, 9, 10):
            members = [(j, classes_of(c, delta)[0]) for j, c in enumerate(coef[:, k]) if classes_of(c, delta)[0]]
            assert members == [], (delta, k, members)
