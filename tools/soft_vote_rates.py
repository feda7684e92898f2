"""Cost of the fused soft vote (include/svsdct.h svs_soft_vote_dev), gray frames of synthetic noise in [16, 240) carrying a
full-capacity payload, n_ac = 10, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the
sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. svs_soft_vote_dev at period = 2 400, 10^6 and capacity / 3 against svs_soft_extract_dev and
     svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac.  The vote writes no soft byte; what it adds instead is one global
     int32 atomic per byte, or per entry a wave touches.  At period = 2 400 every wave of the launch adds into the same 9.6 KB:
     the rate of the atomics there is the open number.  At 10^6 and capacity / 3 the adds spread over megabytes.
  2. the calls that existed - the hard eight-row calls (n = 63, a zig-zag selection, a dither) and the soft call -, this build
     against the baseline library (the parent commit's): the vote tail shares their four instantiations.  The yardstick is the
     baseline's own run-to-run spread in the same process: this build's median should lie inside its min-max.
No ratio is asserted: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_vote_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_vote      # lib/variants/libsvsdct_pre_vote.so, from git
    python tools/soft_vote_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_vote.so
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_vote_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
EXISTING = ("svs_embed_dev", "svs_extract_dev", "svs_extract_select_dev", "svs_extract_dithered_dev", "svs_soft_extract_dev")
base = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))
    for name in EXISTING:
        getattr(base, name).restype, getattr(base, name).argtypes = native.SIGNATURES[name]
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
P = C.byref(planes)
X = native.SVS_EXACT_POCKETFFT
DELTA, KEY, N = 20.0, 0x0123456789ABCDEF, 10
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
cap = batch.capacity_bits(f, h, w, N)
PERIODS = (2400, 10 ** 6, max(1, cap // 3))
packed_bytes = (cap_max + 7) // 8 + 8
d_gray, d_stego, d_bits, d_ext, d_soft = dev(f * h * w), dev(f * h * w), dev(packed_bytes), dev(packed_bytes), dev(cap_max + 8)
d_tally = dev(4 * max(PERIODS))
native.check(lib.svs_fill_synthetic_dev(d_gray, P, 1, 0, 16, 224, None), "fill")
native.check(lib.svs_fill_bits_dev(d_bits, cap_max, 7, 0, None), "fill_bits")
native.check(lib.svs_memset(d_tally, 0, 4 * max(PERIODS), None), "memset")
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
    native.check(lib.svs_embed_dev(d_gray, d_stego, P, DELTA, n_ac, d_bits, 0, batch.capacity_bits(f, h, w, n_ac), X, C.byref(done),
                                   None), "svs_embed_dev")
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


def soft(which, n_ac):
    return lambda: native.check(which.svs_soft_extract_dev(d_stego, P, None, None, None, DELTA, n_ac, d_soft, cap_max, X, C.byref(done),
                                                           None), "svs_soft_extract_dev")


def vote(period, order=None):
    """the tally is added to call after call and never read: a timing, not a decode.  (At the default size a call adds at most
    108 000 copies of 511 to an entry of the smallest period, 5.5e7: the 1 + reps calls stay inside int32 up to 38 of them.)"""
    return lambda: native.check(lib.svs_soft_vote_dev(d_stego, P, order, None, None, DELTA, N, period, 0, d_tally, 0, C.byref(done),
                                                      None), "svs_soft_vote_dev")


def row(k, v):
    return f"    {k:34s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def spread(v):
    return 100 * (max(v) - min(v)) / statistics.median(v)


say(f"fused soft vote, {f} x {w}x{h} gray noise in [16, 240), full-capacity payload, n_ac = {N}, delta = {DELTA:g}, {args.reps} "
    f"alternated repetitions (order rotated), HIP events; ms per call: median (min .. max)")
say("1. svs_soft_vote_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT)")
embed(N)
todo = {"hard": hard(lib, N), "soft": soft(lib, N)}
for period in PERIODS:
    todo[f"vote, period {period}"] = vote(period)
order = batch.block_order(KEY, 0)
todo["vote under an order, period 2400"] = vote(2400, C.byref(order))
native.check(lib.svs_memset(d_tally, 0, 4 * max(PERIODS), None), "memset")
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
                             ("extract, dither, n 10", hard_dithered, 10), ("soft extract n 10", soft, 10), ("soft extract n 63", soft, 63)):
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

for p in (d_gray, d_stego, d_bits, d_ext, d_soft, d_tally):
    lib.svs_free(p)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
