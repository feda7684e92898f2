"""Writes tests/golden/capi_refusals.json: what every svs_embed* / svs_extract* / svs_soft_* entry point of the C ABI answers to arguments it
refuses - the return code, the full svs_last_error() text and what it left in its out parameters (pre-set to a sentinel) -
and to the empty call (n_frames = 0) it accepts.  tests/test_capi_refusals_cpu.py replays the table against the tree's
library, so the table pins order of checks, status codes and messages of the build that wrote it: it is written from the
build BEFORE a change to csrc/svs_capi.hip that must leave them alone
    SVSDCT_LIB=<that build>/lib/libsvsdct.so python tests/golden/make_capi_refusals.py
and is left alone by that change.  (Committed with the refactor to one options value per gray call, from its parent's build;
the svs_soft_* symbols were added, again from the parent's build, ahead of the refactor to one description of a soft call's
output.  The earlier symbols come first, so their entries and every index they use stay as they were.)

Every argument check of these calls runs before any device work, so the library answers without a GPU, and no case may
reach the device: pointers are fake aligned addresses - but for the tally and the counts of the host vote and histogram
calls, which an empty call zero-fills: those are real arrays pre-set to a sentinel byte, and their contents after the call are
part of the recorded outs (a refusal leaves them untouched) - and a table in which a case returns SVS_ERR_HIP, or SVS_OK for a batch
that is not empty, is not written.

Per symbol: a call that would be accepted (never made; the table's "good" values), every fault the symbol checks before its device work applied to it
alone, every pair of faults of two different checks and arguments (which pins precedence), and the empty call with otherwise
bad pointers, with good and with bad flags.  Host-pointer calls check their device-side arguments (alignment, the
extract calls' unknown flag bits, the colour calls' weights) only after staging: those are not faults here.
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from capi_refusals_lib import SENTINEL, arguments, run_case  # noqa: E402
from svsdct import native  # noqa: E402

OUT = os.path.join(HERE, "capi_refusals.json")
KEY = 0x0123456789ABCDEF

_E, _X = "gray stego planes", "gray planes"
_PAY, _OUT = "bits bit_offset n_bits flags n_embedded", "out cap flags n_bits_out"
_VOTE = "period stream_bit0 tally flags n_bits_out"
_BGR = "bgr_in in_rp in_fp bgr_out out_rp out_fp gray_ref planes weights delta n_ac " + _PAY
PARAMS = {name: names.split() for name, names in {
    "svs_embed_dev": f"{_E} delta n_ac {_PAY} stream",
    "svs_embed": f"{_E} delta n_ac {_PAY}",
    "svs_embed_str": "gray gray_ref stego planes delta n_ac ascii n_bits flags n_embedded",
    "svs_extract_str": f"{_X} delta n_ac {_OUT}",
    "svs_embed_ordered_dev": f"{_E} order delta n_ac {_PAY} stream",
    "svs_extract_ordered_dev": f"{_X} order delta n_ac {_OUT} stream",
    "svs_embed_ordered": f"{_E} order delta n_ac {_PAY}",
    "svs_extract_ordered": f"{_X} order delta n_ac {_OUT}",
    "svs_embed_select_dev": f"{_E} order coeffs delta {_PAY} stream",
    "svs_extract_select_dev": f"{_X} order coeffs delta {_OUT} stream",
    "svs_embed_select": f"{_E} order coeffs delta {_PAY}",
    "svs_extract_select": f"{_X} order coeffs delta {_OUT}",
    "svs_embed_dithered_dev": f"{_E} order coeffs dither delta n_ac {_PAY} stream",
    "svs_extract_dithered_dev": f"{_X} order coeffs dither delta n_ac {_OUT} stream",
    "svs_embed_dithered": f"{_E} order coeffs dither delta n_ac {_PAY}",
    "svs_extract_dithered": f"{_X} order coeffs dither delta n_ac {_OUT}",
    "svs_embed_readback_dev": f"{_E} order delta n_ac {_PAY} d_counts stream",
    "svs_embed_readback": f"{_E} order delta n_ac {_PAY} counts",
    "svs_embed_dithered_readback_dev": f"{_E} order coeffs dither delta n_ac {_PAY} d_counts stream",
    "svs_embed_dithered_readback": f"{_E} order coeffs dither delta n_ac {_PAY} counts",
    "svs_extract_dev": f"{_X} delta n_ac {_OUT} stream",
    "svs_extract": f"{_X} delta n_ac {_OUT}",
    "svs_embed_bgr_dev": f"{_BGR} stream",
    "svs_extract_bgr_dev": "bgr_in in_rp in_fp planes weights delta n_ac out cap n_bits_out stream",
    "svs_embed_bgr": "bgr_in bgr_out gray_ref planes weights delta n_ac " + _PAY,
    "svs_extract_bgr": "bgr_in planes weights delta n_ac out cap n_bits_out",
    "svs_embed_bgr_readback_dev": f"{_BGR} d_counts stream",
    "svs_embed_bgr_readback": "bgr_in bgr_out gray_ref planes weights delta n_ac " + _PAY + " counts",
    "svs_soft_extract_dev": f"{_X} order coeffs dither delta n_ac {_OUT} stream",
    "svs_soft_extract": f"{_X} order coeffs dither delta n_ac {_OUT}",
    "svs_soft_vote_dev": f"{_X} order coeffs dither delta n_ac {_VOTE} stream",
    "svs_soft_vote": f"{_X} order coeffs dither delta n_ac {_VOTE}",
    "svs_soft_histogram_dev": f"{_X} coeffs dither delta n_ac hist flags n_bits_out stream",
    "svs_soft_histogram": f"{_X} coeffs dither delta n_ac hist flags n_bits_out",
}.items()}

# 3 frames of 16 x 24: 18 blocks, 54 bits at n_ac = 3 (7 bytes)
GOOD = {"gray": 0x10000, "stego": 0x20000, "gray_ref": None, "planes": [3, 16, 24, 0, 24, 384], "delta": 8.0, "n_ac": 3,
        "bits": 0x30000, "bit_offset": 37, "n_bits": 100, "flags": native.SVS_EXACT_GUARDED, "n_embedded": SENTINEL, "stream": None,
        "order": [9, 5, 0], "coeffs": [3, 9, 2, 17], "dither": [KEY, 5, 0], "d_counts": 0x40000, "counts": [SENTINEL, SENTINEL - 1],
        "out": 0x60000, "cap": 64, "n_bits_out": SENTINEL, "ascii": "01" * 50, "bgr_in": 0x70000, "bgr_out": 0x80000,
        "in_rp": 72, "in_fp": 1152, "out_rp": 72, "out_fp": 1152, "weights": None}
# the soft calls' own good values (kept out of GOOD, whose line of the table stays as it was): the device forms take fake
# addresses, the host forms real arrays of the output's size, 4 * period and 1024 * n_frames bytes of 0xA5
SOFT_GOOD = {"period": 10, "stream_bit0": 5, "tally": 0x90000, "hist": 0xA0000}
SOFT_HOST = {"tally": {"filled": [40, 0xA5]}, "hist": {"filled": [3072, 0xA5]}}
# the selection of GOOD rules (3 bits a block).  1401856 blocks: 3 bits each are above 1 * 2^22;  1500012900 blocks a frame
# (below 2^31): 3 bytes each are above 2^32 - 1
VOTE_BOUND = {"planes": [1, 9472, 9472, 0, 9472, 9472 * 9472], "period": 1}
HIST_BOUND = {"planes": [1, 309840, 309840, 0, 309840, 309840 * 309840]}
FLAG_BITS = (0x4, native.SVS_KEEP_COLOUR, native.SVS_READBACK, 0x400, native.SVS_NEAREST, native.SVS_MINMOVE, 0x80000000)
EMBED_ONLY = native.SVS_READBACK | native.SVS_NEAREST | native.SVS_MINMOVE
MODES = native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED


def traits(sym):
    t = {"dev": sym.endswith("_dev"), "extract": "extract" in sym or "_soft_" in sym, "soft": "_soft_" in sym,
         "vote": "_vote" in sym, "hist": "_histogram" in sym, "bgr": "_bgr" in sym, "str": sym.endswith("_str"),
         "select": "_select" in sym, "dithered": "_dithered" in sym, "readback": "_readback" in sym}
    t["host"] = not t["dev"]
    return t


def refused_flag_bits(sym):
    """the flag bits the symbol refuses before any device work"""
    t = traits(sym)
    if "flags" not in PARAMS[sym]:
        return ()
    if t["extract"]:
        if t["select"] or t["dithered"] or t["soft"] or t["dev"]:
            return FLAG_BITS                                        # the preamble's mask, or svs_extract_dev's own
        return tuple(b for b in FLAG_BITS if b & EMBED_ONLY)         # the host calls leave unknown bits to the device call
    allowed = MODES | native.SVS_NEAREST | native.SVS_MINMOVE
    if t["bgr"]:
        allowed |= native.SVS_KEEP_COLOUR
    if t["readback"] or not (t["bgr"] or t["select"] or t["dithered"]):
        allowed |= native.SVS_READBACK
    return tuple(b for b in FLAG_BITS if not b & allowed)


def faults(sym):
    """-> [(name, check, {argument or "argument.field": value})]: `check` names the check the fault trips; one fault per check
    (the first listed) stands for it in the pairs"""
    t, names = traits(sym), PARAMS[sym]
    has = lambda a: a in names   # noqa: E731
    out = [("planes NULL", "planes", {"planes": None}),
           ("planes.reserved", "planes.reserved", {"planes.3": 7}),
           ("n_frames < 0", "geometry", {"planes.0": -1}), ("height 0", "geometry", {"planes.1": 0}),
           ("width not a multiple of 8", "multiple of 8", {"planes.2": 20}),
           ("row_pitch < width", "row_pitch", {"planes.4": 16}), ("row_pitch % 8", "row_pitch", {"planes.4": 28}),
           ("frame_pitch too small", "frame_pitch", {"planes.5": 8})]
    if t["bgr"] and t["host"]:
        out.append(("planes not tightly packed", "packed", {"planes.4": 32, "planes.5": 512}))
    if has("order"):
        out.append(("order.reserved", "order.reserved", {"order.2": 1}))
    if has("coeffs"):
        if t["select"]:
            out.append(("coeffs NULL", "coeffs", {"coeffs": None}))
        out += [("coeffs.count 64", "coeffs", {"coeffs": [64] + list(range(1, 64))}),
                ("coeffs.index behind count", "coeffs", {"coeffs": [3, 9, 2, 17, 5]}),
                ("coeffs.index repeated", "coeffs", {"coeffs": [3, 9, 2, 9]}),
                ("coeffs.index DC", "coeffs", {"coeffs": [3, 9, 0, 17]})]
    if has("dither"):
        if not (t["readback"] or t["soft"]):
            out.append(("dither NULL", "dither", {"dither": None}))
        out.append(("dither.reserved", "dither", {"dither.2": 1}))
        if has("order"):
            out.append(("dither.first_frame differs", "dither.first_frame", {"dither.1": 6}))
    for bit in refused_flag_bits(sym):
        kind = "embed flag" if t["extract"] and bit & EMBED_ONLY and not (t["select"] or t["dithered"] or t["soft"]) else "flag"
        out.append((f"flag 0x{bit:x}", kind, {"flags": GOOD["flags"] | bit}))
    first, second = ("bgr_in", "bgr_out") if t["bgr"] else ("gray", "stego")
    second = "tally" if t["vote"] else "hist" if t["hist"] else "out" if t["extract"] else second
    good = {**GOOD, **SOFT_GOOD}
    if t["vote"]:
        out += [("period 0", "period", {"period": 0}), ("period 2^61", "period", {"period": 1 << 61})]
    if t["vote"] or t["hist"]:
        out += [("delta 0", "delta", {"delta": 0.0}), ("delta negative", "delta", {"delta": -8.0})]
    out += [(f"{first} NULL", f"{first} NULL", {first: None}), (f"{second} NULL", f"{second} NULL", {second: None})]
    if t["dev"]:
        out += [(f"{first} misaligned", f"{first} aligned", {first: good[first] + 4}),
                (f"{second} misaligned", f"{second} aligned", {second: good[second] + 2})]
    if t["bgr"] and t["dev"]:
        out += [("BGR row pitch short", "in pitches", {"in_rp": 64}), ("BGR frame pitch % 8", "in pitches", {"in_fp": 1156}),
                ("weights do not sum to 2^shift", "weights", {"weights": {"u32s": [1, 1, 1, 15]}}),
                ("weights shift 17", "weights", {"weights": {"u32s": [1 << 16, 1 << 15, 1 << 15, 17]}})]
        if not t["extract"]:
            out += [("BGR out row pitch short", "out pitches", {"out_rp": 64}),
                    ("gray_ref misaligned", "gray_ref", {"gray_ref": 0x50004})]
    if not t["extract"]:
        if t["str"]:
            out += [("payload NULL", "bits NULL", {"ascii": None}),
                    ("payload character 'x'", "characters", {"ascii": "01" * 10 + "x" + "01" * 40}),
                    ("payload character '2' inside the capacity", "characters", {"ascii": "01" * 26 + "2" + "0" * 47}),
                    ("gray_ref is stego", "gray_ref stego", {"gray_ref": GOOD["stego"]}),
                    ("gray_ref overlaps gray", "gray_ref gray", {"gray_ref": GOOD["gray"] + 8})]
        else:
            out += [("bits NULL", "bits NULL", {"bits": None}),
                    ("bit_offset + n_bits overflows", "overflow", {"bit_offset": (1 << 64) - 50})]
            if t["dev"]:
                out += [("bits misaligned", "bits aligned", {"bits": GOOD["bits"] + 2}),
                        ("payload too large", "too large", {"bit_offset": 1 << 37})]
        if has("d_counts"):
            out.append(("counts misaligned", "counts aligned", {"d_counts": GOOD["d_counts"] + 4}))
    elif t["vote"]:
        out.append(("capacity above period * 2^22", "bound", VOTE_BOUND))
    elif t["hist"]:
        out.append(("a frame above 2^32 - 1 bytes", "bound", HIST_BOUND))
    else:
        out.append(("capacity", "capacity", {"cap": 3}))
    return out


def conflict(a, b):
    """two faults that change the same argument or the same field of a struct"""
    for x, y in itertools.product(a, b):
        (ax, _, fx), (ay, _, fy) = x.partition("."), y.partition(".")
        if ax == ay and (not fx or not fy or fx == fy):
            return True
    return False


def cases_of(sym):
    """-> (the single cases [(name, changes)], the pairs [(i, j)] of them)"""
    fs = faults(sym)
    singles = [(name, ch) for name, _, ch in fs]
    reps = {}
    for i, (_, check, _) in enumerate(fs):
        reps.setdefault(check, i)
    pairs = [(i, j) for i, j in itertools.combinations(reps.values(), 2) if not conflict(fs[i][2], fs[j][2])]
    # the empty call: accepted before any pointer is looked at - unless the symbol checks its flags or structs first
    nothing = {"planes.0": 0, **{p: 4 for p in PARAMS[sym] if p in ("gray", "stego", "bits", "out", "bgr_in", "bgr_out", "d_counts")}}
    singles.append(("empty call, bad pointers", nothing))
    if "flags" in PARAMS[sym]:
        singles.append(("empty call, bad pointers and flags", {**nothing, "flags": 0xFFFFFFFF}))
    return singles, pairs


def main():
    lib = native.load()
    symbols = [s for s in native.SIGNATURES if s.startswith(("svs_embed", "svs_extract"))]
    symbols += [s for s in native.SIGNATURES if s.startswith("svs_soft")]   # behind the others: their indices stay
    assert sorted(symbols) == sorted(PARAMS), sorted(set(symbols) ^ set(PARAMS))
    messages, outs_seen, fault_ids, table, n = {}, {}, {}, {}, 0

    def record(sym, own, name, changes):
        rc, msg, outs = run_case(lib, sym, arguments(PARAMS[sym], {**GOOD, **own}, changes))
        if rc == native.SVS_ERR_HIP or (rc == native.SVS_OK and changes.get("planes.0") != 0):
            raise SystemExit(f"{sym}: '{name}' is not refused before the device work ({rc}: {msg}); nothing written")
        return [rc, messages.setdefault(msg, len(messages)), outs_seen.setdefault(json.dumps(outs), len(outs_seen))]

    for sym in symbols:
        assert len(PARAMS[sym]) == len(native.SIGNATURES[sym][1]), sym
        own = {"gray_ref": 0x50000} if traits(sym)["bgr"] and not traits(sym)["extract"] else {}
        if traits(sym)["soft"]:
            own = {k: v for k, v in {**SOFT_GOOD, **(SOFT_HOST if traits(sym)["host"] else {})}.items() if k in PARAMS[sym]}
        singles, pairs = cases_of(sym)
        table[sym] = {"parameters": PARAMS[sym], "good": own,
                      "cases": [[fault_ids.setdefault(json.dumps([name, ch]), len(fault_ids))] + record(sym, own, name, ch)
                                for name, ch in singles],
                      "pairs": [[i, j] + record(sym, own, f"{singles[i][0]} + {singles[j][0]}", {**singles[i][1], **singles[j][1]})
                                for i, j in pairs]}
        n += len(singles) + len(pairs)
    dumps = lambda x: json.dumps(x, separators=(",", ":"))   # noqa: E731
    lines = ['{', f' "sentinel": {SENTINEL},', f' "good": {json.dumps(GOOD)},',
             ' "messages": [\n  ' + ",\n  ".join(json.dumps(m) for m in messages) + "\n ],",
             f' "outs": {dumps([json.loads(o) for o in outs_seen])},',
             ' "faults": [\n  ' + ",\n  ".join(fault_ids) + "\n ],", ' "symbols": {']
    packed = lambda rows: ",\n    ".join(", ".join(dumps(r) for r in rows[i:i + 8]) for i in range(0, len(rows), 8))   # noqa: E731
    for k, (sym, e) in enumerate(table.items()):
        lines += [f'  "{sym}": {{', f'   "parameters": {json.dumps(e["parameters"])}, "good": {json.dumps(e["good"])},',
                  '   "cases": [\n    ' + packed(e["cases"]) + "\n   ],", '   "pairs": [\n    ' + packed(e["pairs"]) + "\n   ]", "  }" + ("," if k + 1 < len(table) else "")]
    with open(OUT, "w") as f:
        f.write("\n".join(lines + [" }", "}"]) + "\n")
    print(f"{n} cases over {len(symbols)} symbols, {len(messages)} messages -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
