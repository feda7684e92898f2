"""Cost and effect of the keyed dither (include/svsdct.h svs_dither), gray frames of synthetic noise in [16, 240), full-capacity
payload, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the two sides of a
comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the dithered embed and extract against the SVS_EXACT_POCKETFFT call at the same n_ac (n = 3, 10, 63): ratio, and the
     run-to-run spread of each side; and the dithered selected call against the selected call (zig-zag, the same counts).
  2. calls WITHOUT a dither, this build against the baseline library (the parent commit's): embed at n = 3, 10 (guarded) and
     10, 63 (exact), extract at n = 3, 10, 63.  This build's median should lie inside the baseline's own min-max spread.
  3. the numbers of the header, from frame 0 of the batch: PSNR against the cover with and without a dither under the three
     rules, the share of recomputed payload coefficients within delta / 4 of a multiple of delta, and the payload bit errors
     over the batch with the right key, another key and no key.
Output: profiles/dither_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_dither      # lib/variants/libsvsdct_pre_dither.so, from git
    python tools/dither_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_dither.so
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
ap.add_argument("--reps", type=int, default=5, help="alternating repetitions per side")
ap.add_argument("--baseline-lib", default=None, help="libsvsdct.so of the parent commit (section 2 is skipped without it)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dither_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
base = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))
    for name in ("svs_embed_dev", "svs_extract_dev"):
        getattr(base, name).restype, getattr(base, name).argtypes = native.SIGNATURES[name]
f, h, w = args.frames, args.h, args.w
planes, one = Planes.contiguous(f, h, w), Planes.contiguous(1, h, w)
P = C.byref(planes)
G, X = native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT
DELTA, KEY, OTHER_KEY = 20.0, 0x0123456789ABCDEF, 0x0123456789ABCDEE
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


def embed_dith(key, delta, n_ac, flags=G):
    cap = batch.capacity_bits(f, h, w, n_ac)
    d = native.Dither(key, 0, 0)
    return lambda: native.check(lib.svs_embed_dithered_dev(d_gray, d_stego, P, None, None, C.byref(d), float(delta), n_ac, d_bits, 0,
                                                           cap, flags, C.byref(done), None), "svs_embed_dithered_dev")


def extract_dith(key, delta, n_ac, flags=G):
    d = native.Dither(key, 0, 0)
    return lambda: native.check(lib.svs_extract_dithered_dev(d_stego, P, None, None, C.byref(d), float(delta), n_ac, d_ext, nbytes,
                                                             flags & 3, C.byref(done), None), "svs_extract_dithered_dev")


def selection(n_ac):
    return coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))


def embed_sel(n_ac, key=None):
    cap = batch.capacity_bits(f, h, w, n_ac)
    sel = selection(n_ac)
    if key is None:
        return lambda: native.check(lib.svs_embed_select_dev(d_gray, d_stego, P, None, C.byref(sel), float(DELTA), d_bits, 0, cap, X,
                                                             C.byref(done), None), "svs_embed_select_dev")
    d = native.Dither(key, 0, 0)
    return lambda: native.check(lib.svs_embed_dithered_dev(d_gray, d_stego, P, None, C.byref(sel), C.byref(d), float(DELTA), 0, d_bits,
                                                           0, cap, X, C.byref(done), None), "svs_embed_dithered_dev")


def extract_sel(n_ac, key=None):
    sel = selection(n_ac)
    if key is None:
        return lambda: native.check(lib.svs_extract_select_dev(d_stego, P, None, C.byref(sel), float(DELTA), d_ext, nbytes, X,
                                                               C.byref(done), None), "svs_extract_select_dev")
    d = native.Dither(key, 0, 0)
    return lambda: native.check(lib.svs_extract_dithered_dev(d_stego, P, None, C.byref(sel), C.byref(d), float(DELTA), 0, d_ext,
                                                             nbytes, X, C.byref(done), None), "svs_extract_dithered_dev")


def row(k, v):
    return f"    {k:34s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def spread(v):
    return 100 * (max(v) - min(v)) / statistics.median(v)


def scalar():
    out = np.zeros(1, np.uint64)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_scalar, 8, None), "d2h")
    sync()
    return int(out[0])


def compare(title, a_name, a, b_name, b):
    t = alternate({a_name: a, b_name: b})
    for k, v in t.items():
        say(row(f"{title} {k}", v))
    r = statistics.median(t[b_name]) / statistics.median(t[a_name])
    say(f"    {title} ratio {b_name} / {a_name} = {r:.3f}  (spread {a_name} {spread(t[a_name]):.1f} %, "
        f"{b_name} {spread(t[b_name]):.1f} %)")


say(f"keyed dither, {f} x {w}x{h} gray noise in [16, 240), full-capacity payload, delta = {DELTA:g}, {args.reps} alternated "
    f"repetitions (order rotated), HIP events; ms per call: median (min .. max)")
say("1. dithered calls against the SVS_EXACT_POCKETFFT call at the same n_ac")
for n_ac in (3, 10, 63):
    compare(f"n {n_ac} embed", "exact", embed(lib, DELTA, n_ac, X), "dithered", embed_dith(KEY, DELTA, n_ac))
    compare(f"n {n_ac} extract", "exact", extract(lib, DELTA, n_ac, X), "dithered", extract_dith(KEY, DELTA, n_ac))
say("1b. dithered selected calls against the selected call (zig-zag scan, the same counts)")
for n_ac in (3, 10, 63):
    compare(f"zigzag {n_ac} embed", "selected", embed_sel(n_ac), "dithered", embed_sel(n_ac, KEY))
    compare(f"zigzag {n_ac} extract", "selected", extract_sel(n_ac), "dithered", extract_sel(n_ac, KEY))

if base is not None:
    say("2. calls without a dither: this build against the baseline (the parent commit's library)")
    outside = 0
    for what, n_ac, flags in (("embed", 3, G), ("embed", 10, G), ("embed", 10, X), ("embed", 63, X), ("extract", 3, G),
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

say("3. frame 0 of the batch, n = 10 (MI355X): PSNR against the cover, the share of recomputed payload coefficients within "
    "delta / 4 of a multiple of delta, payload bit errors over the batch")
from scipy.fftpack import dct  # noqa: E402


def frame0():
    out = np.empty(h * w, np.uint8)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_stego, out.nbytes, None), "d2h")
    sync()
    return out.reshape(h, w)


def comb(stego, n_ac):
    blk = np.float32(stego).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    c = dct(dct(blk, axis=2, norm="ortho"), axis=3, norm="ortho").reshape(-1, 64)[:, 1:n_ac + 1].reshape(-1)
    return float((np.abs(c - DELTA * np.rint(c / DELTA)) < DELTA / 4).mean())


n_ac = 10
cap = batch.capacity_bits(f, h, w, n_ac)
for rule, flag in (("reference", 0), ("SVS_NEAREST", native.SVS_NEAREST), ("SVS_MINMOVE", native.SVS_MINMOVE)):
    res = []
    for name, call in (("no dither", embed(lib, DELTA, n_ac, X | flag)), ("dither", embed_dith(KEY, DELTA, n_ac, flags=X | flag))):
        call()
        native.check(lib.svs_frame_sse_dev(d_gray, d_stego, C.byref(one), d_scalar, None), "sse")
        sse = scalar()
        res.append(f"{name}: PSNR {math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 * h * w / sse):.2f} dB, "
                   f"comb share {comb(frame0(), n_ac):.4f}")
    say(f"    {rule:12s} " + ";  ".join(res))
embed_dith(KEY, DELTA, n_ac)()
for name, call in (("right key", extract_dith(KEY, DELTA, n_ac)), ("another key", extract_dith(OTHER_KEY, DELTA, n_ac)),
                   ("no dither (svs_extract_dev)", extract(lib, DELTA, n_ac, G))):
    call()
    native.check(lib.svs_bit_errors_dev(d_ext, d_bits, cap, d_scalar, None), "bit_errors")
    e = scalar()
    say(f"    dithered stego read with {name:28s} {e:12d} errors of {cap}  (rate {e / cap:.4f})")
for p in (d_gray, d_stego, d_bits, d_ext, d_scalar):
    lib.svs_free(p)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
