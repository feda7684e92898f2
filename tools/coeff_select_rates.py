"""Cost and effect of the payload coefficient selection (include/svsdct.h svs_coeffs), gray frames of synthetic noise in
[16, 240), full-capacity payload.  One process; each call is timed with a pair of HIP events on the null stream, this build and
the baseline library alternated inside every repetition and the order rotated from one repetition to the next.
  1. calls WITHOUT a selection, this build against the baseline: embed at n = 3, 10 (guarded) and 20, 63 (exact), extract at
     n = 3, 10, 63.  This build's median must lie inside the baseline's own min-max spread.
  2. selected calls (zig-zag from scan position 1) at counts 3, 10, 63: embed and extract, as a ratio to the baseline's
     SVS_EXACT_POCKETFFT call at the same n_ac.
  3. the error / PSNR table of the header: row-major, zig-zag from 1, zig-zag from 6 at (delta 4, n 3), (2, 7), (8, 10) -
     payload bit errors over the batch and PSNR of frame 0 against the cover.
Output: profiles/coeff_select_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc parent      # lib/variants/libsvsdct_parent.so, from git
    python tools/coeff_select_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_parent.so
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd"))

from svsdct import batch, coeffs, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--reps", type=int, default=5, help="alternating repetitions per build")
ap.add_argument("--baseline-lib", required=True, help="libsvsdct.so of the parent commit, timed alternately with this build")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coeff_select_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
base = C.CDLL(os.path.abspath(args.baseline_lib))
for name in ("svs_embed_dev", "svs_extract_dev"):
    getattr(base, name).restype, getattr(base, name).argtypes = native.SIGNATURES[name]
f, h, w = args.frames, args.h, args.w
planes, one = Planes.contiguous(f, h, w), Planes.contiguous(1, h, w)
P = C.byref(planes)
G, X = native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def dev(n):
    p = C.c_void_p()
    native.check(lib.svs_malloc(C.byref(p), n), "svs_malloc")
    return p


def sync():
    native.check(lib.svs_stream_synchronize(None), "sync")


cap_max = batch.capacity_bits(f, h, w, 63)
nbytes = (cap_max + 7) // 8 + 8
d_gray, d_stego, d_bits, d_ext, d_scalar = dev(f * h * w), dev(f * h * w), dev(nbytes), dev(nbytes), dev(8)
native.check(lib.svs_fill_synthetic_dev(d_gray, P, 1, 0, 16, 224, None), "fill")
native.check(lib.svs_fill_bits_dev(d_bits, cap_max, 7, 0, None), "fill_bits")
sync()
torch.cuda.init()
torch.cuda.current_stream()
done = C.c_uint64(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(todo):
    for fn in todo.values():
        timed(fn)
    t = {k: [] for k in todo}
    names = list(todo)
    for r in range(args.reps):
        shift = r % len(names)
        for k in names[shift:] + names[:shift]:
            t[k].append(timed(todo[k]))
    return t


def embed(which, delta, n_ac, flags):
    cap = batch.capacity_bits(f, h, w, n_ac)
    return lambda: native.check(which.svs_embed_dev(d_gray, d_stego, P, float(delta), n_ac, d_bits, 0, cap, flags, C.byref(done), None),
                                "svs_embed_dev")


def extract(which, delta, n_ac, flags):
    return lambda: native.check(which.svs_extract_dev(d_stego, P, float(delta), n_ac, d_ext, nbytes, flags, C.byref(done), None),
                                "svs_extract_dev")


def embed_sel(sel, delta, flags=G):
    cap = batch.capacity_bits(f, h, w, sel.count)
    return lambda: native.check(lib.svs_embed_select_dev(d_gray, d_stego, P, None, C.byref(sel), float(delta), d_bits, 0, cap, flags,
                                                         C.byref(done), None), "svs_embed_select_dev")


def extract_sel(sel, delta, flags=G):
    return lambda: native.check(lib.svs_extract_select_dev(d_stego, P, None, C.byref(sel), float(delta), d_ext, nbytes, flags,
                                                           C.byref(done), None), "svs_extract_select_dev")


def row(k, v):
    return f"    {k:34s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def scalar():
    out = np.zeros(1, np.uint64)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_scalar, 8, None), "d2h")
    sync()
    return int(out[0])


say(f"payload coefficient selection, {f} x {w}x{h} gray noise in [16, 240), full-capacity payload, {args.reps} alternated "
    f"repetitions (order rotated), HIP events; ms per call: median (min .. max)")
say("1. calls without a selection: this build against the baseline (the parent commit's library)")
outside = 0
for what, n_ac, flags in (("embed", 3, G), ("embed", 10, G), ("embed", 20, X), ("embed", 63, X), ("extract", 3, G),
                          ("extract", 10, G), ("extract", 63, G)):
    make = embed if what == "embed" else extract
    embed(lib, 8, n_ac, flags)()                           # the stego the extract calls read
    t = alternate({"baseline": make(base, 8, n_ac, flags), "this build": make(lib, 8, n_ac, flags)})
    b, m = t["baseline"], statistics.median(t["this build"])
    ok = min(b) <= m <= max(b)
    outside += not ok
    say(f"  {what} delta 8 n {n_ac} {'exact' if flags == X else 'guarded'}")
    for k, v in t.items():
        say(row(k, v))
    say(f"    this build's median is {'inside' if ok else ('BELOW (faster than)' if m < min(b) else 'ABOVE (slower than)')} "
        f"the baseline's spread")
say(f"  settings outside the baseline's spread: {outside}")

say("2. selected calls (zig-zag from scan position 1) against the baseline's SVS_EXACT_POCKETFFT call at the same n_ac")
for count in (3, 10, 63):
    sel = coeffs.native_coeffs(coeffs.selection("zigzag", count))
    t = alternate({"baseline exact embed": embed(base, 8, count, X), "selected embed": embed_sel(sel, 8)})
    for k, v in t.items():
        say(row(f"n {count} {k}", v))
    b = t["baseline exact embed"]
    r = statistics.median(t["selected embed"]) / statistics.median(b)
    say(f"    n {count} embed ratio selected / exact = {r:.3f}  (baseline spread {100 * (max(b) - min(b)) / statistics.median(b):.1f} %)")
    t = alternate({"baseline exact extract": extract(base, 8, count, X), "selected extract": extract_sel(sel, 8)})
    for k, v in t.items():
        say(row(f"n {count} {k}", v))
    b = t["baseline exact extract"]
    r = statistics.median(t["selected extract"]) / statistics.median(b)
    say(f"    n {count} extract ratio selected / exact = {r:.3f}  (baseline spread {100 * (max(b) - min(b)) / statistics.median(b):.1f} %)")

say("3. payload bit errors over the batch and PSNR of frame 0 against the cover")
for delta, n_ac in ((4, 3), (2, 7), (8, 10)):
    cap = batch.capacity_bits(f, h, w, n_ac)
    for name, spec in (("row-major", "rowmajor"), ("zig-zag from 1", "zigzag"), ("zig-zag from 6", "zigzag:6")):
        sel = coeffs.native_coeffs(coeffs.selection(spec, n_ac))
        embed_sel(sel, delta)()
        native.check(lib.svs_frame_sse_dev(d_gray, d_stego, C.byref(one), d_scalar, None), "sse")
        sse = scalar()
        psnr = math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 * h * w / sse)
        extract_sel(sel, delta)()
        native.check(lib.svs_bit_errors_dev(d_ext, d_bits, cap, d_scalar, None), "bit_errors")
        say(f"    delta {delta} n {n_ac} {name:15s} {scalar():10d} errors of {cap}   PSNR {psnr:.2f} dB")
for p in (d_gray, d_stego, d_bits, d_ext, d_scalar):
    lib.svs_free(p)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
