"""Cost and gain of SVS_NEAREST (include/svsdct.h) on the gray embed, guarded mode, full-capacity payload, synthetic noise frames
(the benchmark's content).  One process; each call is timed with a pair of HIP events on the null stream (torch.cuda.Event; the
library's calls with stream NULL are enqueued on the same stream), the builds and the flag alternated inside every repetition
and the order of the three calls rotated from one repetition to the next, so that no call always runs behind the same
neighbour (--fixed-order keeps one order: with --baseline-lib set to a copy of this build's own library it shows what the
position alone is worth):
  baseline, flag clear     --baseline-lib PATH: the library of the commit before the flag (it refuses the flag)
  this build, flag clear   must stay inside the baseline's own min-max spread of the baseline's median
  this build, flag set     reported beside it (no bar)
and, per setting, the PSNR of frame 0 against the cover without and with the flag (svs_frame_sse_dev) and the payload bit errors
of the flagged stego through svs_extract_dev.  The fused colour embed (svs_embed_bgr_dev, --bgr-frames frames) is timed the
same way for the settings of --bgr-configs.  Output: profiles/nearest_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc parent      # lib/variants/libsvsdct_parent.so, from git
    python tools/nearest_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_parent.so
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

from svsdct import batch, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--reps", type=int, default=5, help="alternating repetitions per build")
ap.add_argument("--configs", default="8:3,8:10,20:10,8:20", help="delta:n_ac,...")
ap.add_argument("--bgr-frames", type=int, default=48)
ap.add_argument("--bgr-configs", default="20:10,8:3", help="delta:n_ac,... of the fused colour embed")
ap.add_argument("--fixed-order", action="store_true", help="baseline, flag clear, flag set in every repetition (no rotation)")
ap.add_argument("--baseline-lib", default=None, help="libsvsdct.so of the parent commit, timed alternately with this build")
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
base = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))      # the same swap testlib.using_library makes: another CDLL, same prototypes
    for name in ("svs_embed_dev", "svs_embed_bgr_dev"):
        getattr(base, name).restype, getattr(base, name).argtypes = native.SIGNATURES[name]
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
one = Planes.contiguous(1, h, w)
P = C.byref(planes)
G, NEAREST = native.SVS_EXACT_GUARDED, native.SVS_NEAREST


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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(todo):
    """name -> times over args.reps repetitions of every call in todo, after one warm-up each"""
    for fn in todo.values():
        timed(fn)
    t = {k: [] for k in todo}
    names = list(todo)
    for r in range(args.reps):
        shift = 0 if args.fixed_order else r % len(names)
        for k in names[shift:] + names[:shift]:
            t[k].append(timed(todo[k]))
    return t


def scalar():
    out = np.zeros(1, np.uint64)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_scalar, 8, None), "d2h")
    sync()
    return int(out[0])


def psnr_frame0():
    native.check(lib.svs_frame_sse_dev(d_gray, d_stego, C.byref(one), d_scalar, None), "sse")
    sse = scalar()
    return math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 * h * w / sse)


print(f"SVS_NEAREST cost and gain, {f} x {w}x{h} gray noise in [16, 240), guarded, full-capacity payload, {args.reps} alternated "
      f"repetitions ({'fixed order' if args.fixed_order else 'order rotated'}), HIP events; ms per call: median (min .. max)")
for cfg in args.configs.split(","):
    delta, n_ac = float(cfg.split(":")[0]), int(cfg.split(":")[1])
    cap = batch.capacity_bits(f, h, w, n_ac)
    done = C.c_uint64(0)

    def embed(which, flags):
        return lambda: native.check(which.svs_embed_dev(d_gray, d_stego, P, delta, n_ac, d_bits, 0, cap, flags, C.byref(done), None),
                                    "svs_embed_dev")

    todo = {"this build, flag clear": embed(lib, G), "this build, flag set": embed(lib, G | NEAREST)}
    if base is not None:
        todo = {"baseline,   flag clear": embed(base, G), **todo}
    t = alternate(todo)
    print(f"delta {delta:g} n {n_ac}")
    for k, v in t.items():
        print(f"    {k:24s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})")
    m = {k: statistics.median(v) for k, v in t.items()}
    if base is not None:
        b = t["baseline,   flag clear"]
        spread, over = max(b) - min(b), m["this build, flag clear"] - m["baseline,   flag clear"]
        print(f"    flag clear: this build - baseline = {over:+.3f} ms, baseline spread {spread:.3f} ms: "
              f"{'inside' if over <= spread else 'OUTSIDE'} the noise floor")
        over_set = m["this build, flag set"] - m["baseline,   flag clear"]
        print(f"    flag set:   this build - baseline = {over_set:+.3f} ms ({100 * over_set / m['baseline,   flag clear']:+.1f} %)")
    todo["this build, flag clear"]()
    p_off = psnr_frame0()
    todo["this build, flag set"]()
    p_on = psnr_frame0()
    got = C.c_uint64(0)
    native.check(lib.svs_extract_dev(d_stego, P, delta, n_ac, d_ext, nbytes, G, C.byref(got), None), "extract")
    native.check(lib.svs_bit_errors_dev(d_ext, d_bits, cap, d_scalar, None), "bit_errors")
    print(f"    PSNR frame 0: {p_off:.2f} -> {p_on:.2f} dB ({p_on - p_off:+.2f}); payload bit errors with the flag: {scalar()} of {cap}")

# ---- the fused colour embed (its kernel tests the rule once per block) ----
fb = min(args.bgr_frames, f)
bplanes, wide = Planes.contiguous(fb, h, w), Planes.contiguous(fb, h, 3 * w)
rp, fp = 3 * w, 3 * w * h
d_bgr, d_out = dev(fb * fp), dev(fb * fp)
native.check(lib.svs_fill_synthetic_dev(d_bgr, C.byref(wide), 1, 0, 16, 224, None), "fill")
sync()
print(f"fused colour embed, {fb} x {w}x{h} BGR")
for cfg in [c for c in args.bgr_configs.split(",") if c]:
    delta, n_ac = float(cfg.split(":")[0]), int(cfg.split(":")[1])
    cap = batch.capacity_bits(fb, h, w, n_ac)
    done = C.c_uint64(0)

    def embed_bgr(which, flags):
        return lambda: native.check(which.svs_embed_bgr_dev(d_bgr, rp, fp, d_out, rp, fp, None, C.byref(bplanes), None, delta, n_ac,
                                                            d_bits, 0, cap, flags, C.byref(done), None), "svs_embed_bgr_dev")

    todo = {"this build, flag clear": embed_bgr(lib, G), "this build, flag set": embed_bgr(lib, G | NEAREST)}
    if base is not None:
        todo = {"baseline,   flag clear": embed_bgr(base, G), **todo}
    t = alternate(todo)
    print(f"delta {delta:g} n {n_ac}")
    for k, v in t.items():
        print(f"    {k:24s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})")
    if base is not None:
        b = t["baseline,   flag clear"]
        spread = max(b) - min(b)
        over = statistics.median(t["this build, flag clear"]) - statistics.median(b)
        print(f"    flag clear: this build - baseline = {over:+.3f} ms, baseline spread {spread:.3f} ms: "
              f"{'inside' if over <= spread else 'OUTSIDE'} the noise floor")
for p in (d_gray, d_stego, d_bits, d_ext, d_scalar, d_bgr, d_out):
    lib.svs_free(p)
