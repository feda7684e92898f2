"""Cost of the soft-decision extraction (include/svsdct.h svs_soft_extract_dev), gray frames of synthetic noise in [16, 240)
carrying a full-capacity payload, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the
two sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the soft call against svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac (n = 3, 10, 63): ratio, and the run-to-run
     spread of each side.  The soft call writes eight times the bytes and always runs the eight-row kernel; at n = 3 and 10 the
     hard call runs the one- and two-row instantiations.
  2. the hard eight-row calls - n = 63, a zig-zag selection, a dither -, this build against the baseline library (the parent
     commit's): the soft side shares their four instantiations.  This build's median should lie inside the baseline's own
     min-max spread.
Nobody has measured these times yet, so no ratio is expected: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_extract_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_soft      # lib/variants/libsvsdct_pre_soft.so, from git
    python tools/soft_extract_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_soft.so
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd"))

from svsdct import batch, coeffs, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--reps", type=int, default=5, help="alternating repetitions per side")
ap.add_argument("--baseline-lib", default=None, help="libsvsdct.so of the parent commit (section 2 is skipped without it)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_extract_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
HARD = ("svs_embed_dev", "svs_extract_dev", "svs_extract_select_dev", "svs_extract_dithered_dev")
base = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))
    for name in HARD:
        getattr(base, name).restype, getattr(base, name).argtypes = native.SIGNATURES[name]
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
P = C.byref(planes)
X = native.SVS_EXACT_POCKETFFT
DELTA, KEY = 20.0, 0x0123456789ABCDEF
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
packed_bytes = (cap_max + 7) // 8 + 8
d_gray, d_stego, d_bits, d_ext, d_soft = dev(f * h * w), dev(f * h * w), dev(packed_bytes), dev(packed_bytes), dev(cap_max + 8)
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


def embed(n_ac):
    """the stego the extract calls read: a full payload at n_ac"""
    cap = batch.capacity_bits(f, h, w, n_ac)
    native.check(lib.svs_embed_dev(d_gray, d_stego, P, DELTA, n_ac, d_bits, 0, cap, X, C.byref(done), None), "svs_embed_dev")
    sync()


def hard(which, n_ac):
    return lambda: native.check(which.svs_extract_dev(d_stego, P, DELTA, n_ac, d_ext, packed_bytes, X, C.byref(done), None),
                                "svs_extract_dev")


def hard_select(which, n_ac):
    sel = coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))
    return lambda: native.check(which.svs_extract_select_dev(d_stego, P, None, C.byref(sel), DELTA, d_ext, packed_bytes, X,
                                                             C.byref(done), None), "svs_extract_select_dev")


def hard_dithered(which, n_ac):
    d = native.Dither(KEY, 0, 0)
    return lambda: native.check(which.svs_extract_dithered_dev(d_stego, P, None, None, C.byref(d), DELTA, n_ac, d_ext, packed_bytes, X,
                                                               C.byref(done), None), "svs_extract_dithered_dev")


def soft(n_ac):
    return lambda: native.check(lib.svs_soft_extract_dev(d_stego, P, None, None, None, DELTA, n_ac, d_soft, cap_max, X, C.byref(done),
                                                         None), "svs_soft_extract_dev")


def row(k, v):
    return f"    {k:34s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def spread(v):
    return 100 * (max(v) - min(v)) / statistics.median(v)


say(f"soft-decision extraction, {f} x {w}x{h} gray noise in [16, 240), full-capacity payload, delta = {DELTA:g}, {args.reps} "
    f"alternated repetitions (order rotated), HIP events; ms per call: median (min .. max)")
say("1. the soft call against svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac")
for n_ac in (3, 10, 63):
    embed(n_ac)
    t = alternate({"hard": hard(lib, n_ac), "soft": soft(n_ac)})
    for k, v in t.items():
        say(row(f"n {n_ac} {k}", v))
    say(f"    n {n_ac} ratio soft / hard = {statistics.median(t['soft']) / statistics.median(t['hard']):.3f}  "
        f"(spread hard {spread(t['hard']):.1f} %, soft {spread(t['soft']):.1f} %)")

if base is not None:
    say("2. the hard eight-row extract calls: this build against the baseline (the parent commit's library)")
    outside = 0
    embed(63)
    for what, make, n_ac in (("n 63", hard, 63), ("zig-zag selection of 10", hard_select, 10), ("dither, n 10", hard_dithered, 10)):
        t = alternate({"baseline": make(base, n_ac), "this build": make(lib, n_ac)})
        b, m = t["baseline"], statistics.median(t["this build"])
        ok = min(b) <= m <= max(b)
        outside += not ok
        say(f"  extract {what}")
        for k, v in t.items():
            say(row(k, v))
        say(f"    this build's median is {'inside' if ok else ('BELOW (faster than)' if m < min(b) else 'ABOVE (slower than)')} "
            f"the baseline's spread")
    say(f"  settings outside the baseline's spread: {outside}")

for p in (d_gray, d_stego, d_bits, d_ext, d_soft):
    lib.svs_free(p)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
