"""Cost of the fused per-frame soft histograms (include/svsdct.h svs_soft_histogram_dev), 200 x 3840x2160 gray frames,
delta = 20, n_ac = 3, 10 and 63, on two contents: never-embedded noise in [16, 240), whose rows are flat (every one of the 256
counters of a workgroup's table is hit), and reference-rule full-capacity stego of the same noise, whose rows are peaked (the
case in which LDS atomics of one instruction to one address serialise; how peaked is printed: the stego pixels are rounded, so
the bytes spread over some 64 values, not two).  One process; each call is timed with a pair of HIP events on the null stream,
the sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. svs_soft_histogram_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT) of the same build, per content
     and n_ac.  The histogram call writes no soft byte; what it adds instead is one LDS add per byte and at most 256 global
     atomics per workgroup and frame.  --variant-lib NAME=PATH times the histogram call of another build of the library beside
     it (how the counting was chosen: profiles/soft_histogram_variants.txt).
  2. the calls that existed - the hard eight-row calls (n = 63, a zig-zag selection, a dither), the soft call at n = 10 and 63
     and the vote at period 10^6 -, this build against the baseline library (the parent commit's): the histogram tail shares
     their instantiations.  The yardstick is the baseline's own run-to-run spread in the same process: this build's median
     should lie inside its min-max.
No ratio is asserted: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_histogram_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_hist      # lib/variants/libsvsdct_pre_hist.so, from git
    python tools/soft_histogram_rates.py --reps 15 \\
        --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_hist.so
"""
import argparse
import ctypes as C
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
ap.add_argument("--reps", type=int, default=15, help="alternating repetitions per side")
ap.add_argument("--baseline-lib", default=None, help="libsvsdct.so of the parent commit (section 2 is skipped without it)")
ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH",
                help="another build of this library whose histogram call section 1 times beside this build's")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_histogram_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
EXISTING = ("svs_extract_dev", "svs_extract_select_dev", "svs_extract_dithered_dev", "svs_soft_extract_dev", "svs_soft_vote_dev")


def other(path, names):
    so = C.CDLL(os.path.abspath(path))
    for name in names:
        getattr(so, name).restype, getattr(so, name).argtypes = native.SIGNATURES[name]
    return so


base = other(args.baseline_lib, EXISTING) if args.baseline_lib else None
variants = {v.split("=", 1)[0]: other(v.split("=", 1)[1], ("svs_soft_histogram_dev",)) for v in args.variant_lib}
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
P = C.byref(planes)
X = native.SVS_EXACT_POCKETFFT
DELTA, KEY, N_ACS, PERIOD = 20.0, 0x0123456789ABCDEF, (3, 10, 63), 10 ** 6
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
d_hist, d_tally = dev(1024 * f), dev(4 * PERIOD)
native.check(lib.svs_fill_synthetic_dev(d_gray, P, 1, 0, 16, 224, None), "fill")
native.check(lib.svs_fill_bits_dev(d_bits, cap_max, 7, 0, None), "fill_bits")
native.check(lib.svs_memset(d_tally, 0, 4 * PERIOD, None), "memset")
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
    """the stego the calls read: the reference rule, a full payload at n_ac"""
    native.check(lib.svs_embed_dev(d_gray, d_stego, P, DELTA, n_ac, d_bits, 0, batch.capacity_bits(f, h, w, n_ac), X, C.byref(done),
                                   None), "svs_embed_dev")
    sync()


def hard(which, n_ac, src=None):
    src = src or d_stego
    return lambda: native.check(which.svs_extract_dev(src, P, DELTA, n_ac, d_ext, packed_bytes, X, C.byref(done), None),
                                "svs_extract_dev")


def hard_select(which, n_ac):
    sel = coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))
    return lambda: native.check(which.svs_extract_select_dev(d_stego, P, None, C.byref(sel), DELTA, d_ext, packed_bytes, X,
                                                             C.byref(done), None), "svs_extract_select_dev")


def hard_dithered(which, n_ac):
    d = native.Dither(KEY, 0, 0)
    return lambda: native.check(which.svs_extract_dithered_dev(d_stego, P, None, None, C.byref(d), DELTA, n_ac, d_ext, packed_bytes, X,
                                                               C.byref(done), None), "svs_extract_dithered_dev")


def soft(which, n_ac, src=None):
    src = src or d_stego
    return lambda: native.check(which.svs_soft_extract_dev(src, P, None, None, None, DELTA, n_ac, d_soft, cap_max, X, C.byref(done),
                                                           None), "svs_soft_extract_dev")


def vote(which, n_ac):
    """the tally is added to call after call and never read: a timing, not a decode"""
    return lambda: native.check(which.svs_soft_vote_dev(d_stego, P, None, None, None, DELTA, n_ac, PERIOD, 0, d_tally, 0, C.byref(done),
                                                        None), "svs_soft_vote_dev")


def histogram(which, n_ac, src):
    """the rows are added to call after call: 1 + reps calls of at most 129 600 * 63 bytes a frame stay far inside uint32"""
    return lambda: native.check(which.svs_soft_histogram_dev(src, P, None, None, DELTA, n_ac, d_hist, 0, C.byref(done), None),
                                "svs_soft_histogram_dev")


def row(k, v):
    return f"    {k:34s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def spread(v):
    return 100 * (max(v) - min(v)) / statistics.median(v)


def rows_of(src, n_ac):
    """one histogram call into cleared rows -> [frames, 256]"""
    native.check(lib.svs_memset(d_hist, 0, 1024 * f, None), "memset")
    histogram(lib, n_ac, src)()
    sync()
    out = np.zeros(256 * f, np.uint32)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_hist, out.nbytes, None), "d2h")
    sync()
    return out.reshape(f, 256)


say(f"fused per-frame soft histograms, {f} x {w}x{h} gray, delta = {DELTA:g}, {args.reps} alternated repetitions (order rotated), "
    f"HIP events; ms per call: median (min .. max)")
say("1. svs_soft_histogram_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT) of the same build")
for n_ac in N_ACS:
    embed(n_ac)
    for content, src in (("noise in [16, 240), never embedded", d_gray), ("reference-rule full-capacity stego", d_stego)):
        rows = rows_of(src, n_ac)
        top2 = np.sort(rows, axis=1)[:, -2:].sum() / rows.sum()
        say(f"  n_ac = {n_ac}, {content}: rows sum to {int(rows[0].sum())} a frame, {int((rows[0] != 0).sum())} entries of frame 0 "
            f"are not 0, the two largest entries of a row hold {100 * top2:.1f} % of it")
        todo = {"hard": hard(lib, n_ac, src), "soft": soft(lib, n_ac, src), "histogram": histogram(lib, n_ac, src)}
        for name, so in variants.items():
            todo[f"histogram, {name}"] = histogram(so, n_ac, src)
        t = alternate(todo)
        for k, v in t.items():
            say(row(k, v) + f"  spread {spread(v):.1f} %")
        for k in list(t)[2:]:
            say(f"    {k}: ratio to soft {statistics.median(t[k]) / statistics.median(t['soft']):.3f}, to hard "
                f"{statistics.median(t[k]) / statistics.median(t['hard']):.3f}")

if base is not None:
    say("2. the calls that existed: this build against the baseline (the parent commit's library)")
    outside = 0
    embed(63)
    for what, make, n_ac in (("extract n 63", hard, 63), ("extract, zig-zag selection of 10", hard_select, 10),
                             ("extract, dither, n 10", hard_dithered, 10), ("soft extract n 10", soft, 10), ("soft extract n 63", soft, 63),
                             (f"soft vote n 10, period {PERIOD}", vote, 10)):
        t = alternate({"baseline": make(base, n_ac), "this build": make(lib, n_ac)})
        b, m = t["baseline"], statistics.median(t["this build"])
        ok = min(b) <= m <= max(b)
        outside += not ok
        say(f"  {what}")
        for k, v in t.items():
            say(row(k, v))
        say(f"    this build's median is {'inside' if ok else ('BELOW (faster than)' if m < min(b) else 'ABOVE (slower than)')} "
            f"the baseline's spread")
    say(f"  settings outside the baseline's spread: {outside}")

for p in (d_gray, d_stego, d_bits, d_ext, d_soft, d_hist, d_tally):
    lib.svs_free(p)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
