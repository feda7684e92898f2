"""Cost and gain of SVS_MINMOVE (include/svsdct.h) on the gray embed, guarded mode, full-capacity payload, synthetic noise frames
(the benchmark's content).  One process; each call is timed with a pair of HIP events on the null stream (torch.cuda.Event; the
library's calls with stream NULL are enqueued on the same stream), the builds and the flags alternated inside every repetition
and the order of the calls rotated from one repetition to the next, so that no call always runs behind the same neighbour
(--fixed-order keeps one order):
  baseline, flag clear     --baseline-lib PATH: the library of the commit before the flag (it refuses the flag)
  baseline, SVS_NEAREST    the parent's nearest-rule time: what the time with the new flag set is compared with
  this build, flag clear   must stay inside the baseline's own min-max spread of the baseline's median
  this build, SVS_NEAREST  likewise against the baseline's nearest time
  this build, SVS_MINMOVE  reported beside them (no bar)
and, per setting, the PSNR of frame 0 against the cover under the three rules (svs_frame_sse_dev) and the payload bit errors of
the minimum-move stego through svs_extract_dev.  The fused colour embed (svs_embed_bgr_dev, --bgr-frames frames) is timed the
same way for the settings of --bgr-configs.  Output: profiles/minmove_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_minmove      # lib/variants/libsvsdct_pre_minmove.so, from git
    python tools/minmove_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_minmove.so
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
ap.add_argument("--configs", default="20:3,20:10,20:20", help="delta:n_ac,...")
ap.add_argument("--bgr-frames", type=int, default=48)
ap.add_argument("--bgr-configs", default="20:10", help="delta:n_ac,... of the fused colour embed")
ap.add_argument("--fixed-order", action="store_true", help="the same order of the calls in every repetition (no rotation)")
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
G, NEAREST, MINMOVE = native.SVS_EXACT_GUARDED, native.SVS_NEAREST, native.SVS_MINMOVE


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


def report(t):
    """medians with their ranges; against a baseline: each of this build's older sides against the baseline's spread, and the
    new flag's time against the baseline's SVS_NEAREST time"""
    for k, v in t.items():
        print(f"    {k:24s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})")
    if base is None:
        return
    m = {k: statistics.median(v) for k, v in t.items()}
    for side in ("flag clear", "SVS_NEAREST"):
        b = t["baseline,   " + side]
        spread, over = max(b) - min(b), m["this build, " + side] - m["baseline,   " + side]
        print(f"    {side}: this build - baseline = {over:+.3f} ms, baseline spread {spread:.3f} ms: "
              f"{'inside' if over <= spread else 'OUTSIDE'} the noise floor")
    over = m["this build, SVS_MINMOVE"] - m["baseline,   SVS_NEAREST"]
    print(f"    SVS_MINMOVE: this build - baseline's SVS_NEAREST = {over:+.3f} ms ({100 * over / m['baseline,   SVS_NEAREST']:+.1f} %)")


print(f"SVS_MINMOVE cost and gain, {f} x {w}x{h} gray noise in [16, 240), guarded, full-capacity payload, {args.reps} alternated "
      f"repetitions ({'fixed order' if args.fixed_order else 'order rotated'}), HIP events; ms per call: median (min .. max)")
for cfg in args.configs.split(","):
    delta, n_ac = float(cfg.split(":")[0]), int(cfg.split(":")[1])
    cap = batch.capacity_bits(f, h, w, n_ac)
    done = C.c_uint64(0)

    def embed(which, flags):
        return lambda: native.check(which.svs_embed_dev(d_gray, d_stego, P, delta, n_ac, d_bits, 0, cap, flags, C.byref(done), None),
                                    "svs_embed_dev")

    todo = {"this build, flag clear": embed(lib, G), "this build, SVS_NEAREST": embed(lib, G | NEAREST),
            "this build, SVS_MINMOVE": embed(lib, G | MINMOVE)}
    if base is not None:
        todo = {"baseline,   flag clear": embed(base, G), "baseline,   SVS_NEAREST": embed(base, G | NEAREST), **todo}
    t = alternate(todo)
    print(f"delta {delta:g} n {n_ac}")
    report(t)
    psnr = []
    for k in ("this build, flag clear", "this build, SVS_NEAREST", "this build, SVS_MINMOVE"):
        todo[k]()
        psnr.append(psnr_frame0())
    got = C.c_uint64(0)
    native.check(lib.svs_extract_dev(d_stego, P, delta, n_ac, d_ext, nbytes, G, C.byref(got), None), "extract")
    native.check(lib.svs_bit_errors_dev(d_ext, d_bits, cap, d_scalar, None), "bit_errors")
    print(f"    PSNR frame 0: reference {psnr[0]:.2f}, SVS_NEAREST {psnr[1]:.2f}, SVS_MINMOVE {psnr[2]:.2f} dB "
          f"({psnr[2] - psnr[0]:+.2f} / {psnr[2] - psnr[1]:+.2f}); payload bit errors with SVS_MINMOVE: {scalar()} of {cap}")

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

    todo = {"this build, flag clear": embed_bgr(lib, G), "this build, SVS_NEAREST": embed_bgr(lib, G | NEAREST),
            "this build, SVS_MINMOVE": embed_bgr(lib, G | MINMOVE)}
    if base is not None:
        todo = {"baseline,   flag clear": embed_bgr(base, G), "baseline,   SVS_NEAREST": embed_bgr(base, G | NEAREST), **todo}
    t = alternate(todo)
    print(f"delta {delta:g} n {n_ac}")
    report(t)
for p in (d_gray, d_stego, d_bits, d_ext, d_scalar, d_bgr, d_out):
    lib.svs_free(p)
