"""Cost of SVS_READBACK: svs_embed_readback_dev (embed, then the read-back pass over the stego) against svs_embed_dev, the same
call without the flag, on noise and on letterboxed frames (noise with black bars over a third of the rows), full-capacity
payload, guarded mode.  The two calls alternate in the same rounds; each call is timed on the host around the launch and a
stream synchronisation.  Output: profiles/readback_rates.txt.

    python tools/readback_rates.py [--frames 600 --h 2160 --w 3840 --rounds 10]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd"))

from svsdct import batch, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--configs", default="8:3,20:10", help="delta:n_ac,...")
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
nbytes = f * h * w


def dev(n):
    p = C.c_void_p()
    native.check(lib.svs_malloc(C.byref(p), n), "svs_malloc")
    return p


def sync():
    native.check(lib.svs_stream_synchronize(None), "sync")


d_gray, d_stego, d_counts = dev(nbytes), dev(nbytes), dev(16)
cap = batch.capacity_bits(f, h, w, 63)
d_bits = dev((cap + 7) // 8 + 8)
native.check(lib.svs_fill_bits_dev(d_bits, cap, 7, 0, None), "fill_bits")
flags = native.SVS_EXACT_GUARDED
bar = (h // 6) // 8 * 8


def content(kind):
    native.check(lib.svs_fill_synthetic_dev(d_gray, C.byref(planes), 1, 0, 0, 256, None), "fill")
    if kind == "letterbox":
        for k in range(f):
            base = d_gray.value + k * h * w
            native.check(lib.svs_memset(C.c_void_p(base), 0, bar * w, None), "memset")
            native.check(lib.svs_memset(C.c_void_p(base + (h - bar) * w), 0, bar * w, None), "memset")
    sync()


def run(flagged, delta, n_ac):
    done = C.c_uint64(0)
    sync()
    t0 = time.perf_counter()
    if flagged:
        rc = lib.svs_embed_readback_dev(d_gray, d_stego, C.byref(planes), None, float(delta), n_ac, d_bits, 0, cap, flags,
                                        C.byref(done), d_counts, None)
    else:
        rc = lib.svs_embed_dev(d_gray, d_stego, C.byref(planes), float(delta), n_ac, d_bits, 0, cap, flags, C.byref(done), None)
    native.check(rc, "embed")
    sync()
    return 1e3 * (time.perf_counter() - t0)


print(f"SVS_READBACK cost, {f} x {w}x{h}, guarded, full-capacity payload, {args.rounds} rounds (median / min ms per call)")
for cfg in args.configs.split(","):
    delta, n_ac = float(cfg.split(":")[0]), int(cfg.split(":")[1])
    for kind in ("noise", "letterbox"):
        content(kind)
        for flagged in (False, True):   # warm-up
            run(flagged, delta, n_ac)
        native.check(lib.svs_memset(d_counts, 0, 16, None), "memset")
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for flagged in (False, True):
                t[flagged].append(run(flagged, delta, n_ac))
        counts = (C.c_uint64 * 2)()
        native.check(lib.svs_memcpy_d2h(counts, d_counts, 16, None), "d2h")
        sync()
        blocks = f * (h // 8) * (w // 8)
        a, b = statistics.median(t[False]), statistics.median(t[True])
        print(f"delta {delta:g} n {n_ac:2d} {kind:9s}  embed {a:8.3f} / {min(t[False]):8.3f}   embed+readback {b:8.3f} / "
              f"{min(t[True]):8.3f}   read-back pass {b - a:8.3f} ms   x{b / a:.2f}   per call: repaired "
              f"{counts[0] // args.rounds} unrepaired {counts[1] // args.rounds} of {blocks} blocks")
for p in (d_gray, d_stego, d_counts, d_bits):
    lib.svs_free(p)
