"""Cost of the colour read-back pass (svs_embed_bgr_readback_dev) on colour noise and on letterboxed colour noise, full-capacity
payload, guarded mode.  Alternated in the same rounds of one process, each call timed with a pair of HIP events on the null
stream (torch.cuda.Event; the library's calls are enqueued on the same stream):
  embed_bgr                      the fused colour embed alone (plain and keep-colour)
  embed_bgr_readback             the same with the pass: pass = the difference
  extract_bgr                    an extraction pass over the same BGR frames
  bgr_to_gray -> embed_readback -> gray_to_bgr   the three-launch composition the plain form replaces
  embed / embed_readback         the gray calls on the frames' gray: the gray pass of this build, and - when
                                 lib/variants/libsvsdct_pre_colour.so exists (`make -C csrc pre_colour`) - of the build before the
                                 colour form, twice each ("a" / "b": the difference between two runs of the same library is the
                                 spread the comparison has to be read against)
Output: profiles/colour_readback_rates.txt.

    python tools/colour_readback_rates.py [--frames 200 --h 2160 --w 3840 --rounds 7]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time  # noqa: F401

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd"))

from svsdct import batch, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--configs", default="8:3,20:10,7.5:20", help="delta:n_ac,... (7.5:20: eight coefficient rows, no power of two)")
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
f, h, w = args.frames, args.h, args.w
planes = Planes.contiguous(f, h, w)
wide = Planes.contiguous(f, h, 3 * w)          # the BGR frames seen as planes of 3 w bytes per row, to fill them
rp, fp = 3 * w, 3 * w * h


def dev(n):
    p = C.c_void_p()
    native.check(lib.svs_malloc(C.byref(p), n), "svs_malloc")
    return p


def sync():
    native.check(lib.svs_stream_synchronize(None), "sync")


d_bgr, d_out, d_gray, d_stego, d_counts = dev(f * fp), dev(f * fp), dev(f * h * w), dev(f * h * w), dev(16)
cap63 = batch.capacity_bits(f, h, w, 63)
d_bits, d_ext = dev((cap63 + 7) // 8 + 8), dev((cap63 + 7) // 8 + 8)
native.check(lib.svs_fill_bits_dev(d_bits, cap63, 7, 0, None), "fill_bits")
G = native.SVS_EXACT_GUARDED
bar = (h // 6) // 8 * 8


def content(kind):
    native.check(lib.svs_fill_synthetic_dev(d_bgr, C.byref(wide), 1, 0, 0, 256, None), "fill")
    if kind == "letterbox":
        for k in range(f):
            base = d_bgr.value + k * fp
            native.check(lib.svs_memset(C.c_void_p(base), 0, bar * rp, None), "memset")
            native.check(lib.svs_memset(C.c_void_p(base + (h - bar) * rp), 0, bar * rp, None), "memset")
    native.check(lib.svs_bgr_to_gray_dev(d_bgr, rp, fp, d_gray, C.byref(planes), None, None), "gray")
    sync()


torch.cuda.init()
torch.cuda.current_stream()          # the default (null) stream: the one the library's calls with stream NULL use
PRE = os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd", "lib", "variants", "libsvsdct_pre_colour.so")
old = None
if os.path.exists(PRE):
    old = C.CDLL(PRE)
    for name in ("svs_embed_dev", "svs_embed_readback_dev"):
        getattr(old, name).restype, getattr(old, name).argtypes = native.SIGNATURES[name]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calls(delta, n_ac):
    cap = batch.capacity_bits(f, h, w, n_ac)
    done, P = C.c_uint64(0), C.byref(planes)
    ck = native.check
    d = float(delta)

    def bgr(keep, rb):
        flags = G | (native.SVS_KEEP_COLOUR if keep else 0)
        if rb:
            return lambda: ck(lib.svs_embed_bgr_readback_dev(d_bgr, rp, fp, d_out, rp, fp, None, P, None, d, n_ac, d_bits, 0, cap,
                                                             flags, C.byref(done), d_counts, None), "bgr_rb")
        return lambda: ck(lib.svs_embed_bgr_dev(d_bgr, rp, fp, d_out, rp, fp, None, P, None, d, n_ac, d_bits, 0, cap, flags,
                                                C.byref(done), None), "bgr")

    def three():
        ck(lib.svs_bgr_to_gray_dev(d_bgr, rp, fp, d_stego, P, None, None), "to_gray")
        ck(lib.svs_embed_readback_dev(d_stego, d_stego, P, None, d, n_ac, d_bits, 0, cap, G, C.byref(done), d_counts, None), "rb")
        ck(lib.svs_gray_to_bgr_dev(d_stego, P, d_out, rp, fp, None), "to_bgr")

    def gray(which, rb):
        if rb:
            return lambda: ck(which.svs_embed_readback_dev(d_gray, d_stego, P, None, d, n_ac, d_bits, 0, cap, G, C.byref(done),
                                                           d_counts, None), "embed_rb")
        return lambda: ck(which.svs_embed_dev(d_gray, d_stego, P, d, n_ac, d_bits, 0, cap, G, C.byref(done), None), "embed")

    extra = {}
    if old is not None:
        for tag in ("a", "b"):
            extra[f"embed_readback gray, this {tag}"] = gray(lib, True)
            extra[f"embed_readback gray, before {tag}"] = gray(old, True)
            extra[f"embed gray, this {tag}"] = gray(lib, False)
            extra[f"embed gray, before {tag}"] = gray(old, False)
    return {
        "embed_bgr plain": bgr(False, False), "embed_bgr_readback plain": bgr(False, True),
        "embed_bgr keep": bgr(True, False), "embed_bgr_readback keep": bgr(True, True),
        "extract_bgr": lambda: ck(lib.svs_extract_bgr_dev(d_out, rp, fp, P, None, d, n_ac, d_ext, (cap63 + 7) // 8 + 8,
                                                          C.byref(done), None), "extract_bgr"),
        "three launches": three,
        "embed gray": lambda: ck(lib.svs_embed_dev(d_gray, d_stego, P, d, n_ac, d_bits, 0, cap, G, C.byref(done), None), "embed"),
        "embed_readback gray": lambda: ck(lib.svs_embed_readback_dev(d_gray, d_stego, P, None, d, n_ac, d_bits, 0, cap, G,
                                                                     C.byref(done), d_counts, None), "embed_rb"),
        **extra,
    }


print(f"colour read-back cost, {f} x {w}x{h} BGR, guarded, full-capacity payload, {args.rounds} alternated rounds, "
      f"HIP events; median / min ms per call")
for cfg in args.configs.split(","):
    delta, n_ac = float(cfg.split(":")[0]), int(cfg.split(":")[1])
    for kind in ("noise", "letterbox"):
        content(kind)
        todo = calls(delta, n_ac)
        for fn in todo.values():
            timed(fn)
        t = {k: [] for k in todo}
        for _ in range(args.rounds):
            for k, fn in todo.items():
                t[k].append(timed(fn))
        print(f"delta {delta:g} n {n_ac} {kind}")
        for k, v in t.items():
            print(f"    {k:34s} {statistics.median(v):8.3f} / {min(v):8.3f}   spread {max(v) - min(v):6.3f}")
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"    colour pass plain {m['embed_bgr_readback plain'] - m['embed_bgr plain']:.3f}  keep "
              f"{m['embed_bgr_readback keep'] - m['embed_bgr keep']:.3f}  gray pass {m['embed_readback gray'] - m['embed gray']:.3f}  "
              f"extract_bgr {m['extract_bgr']:.3f}  plain fused {m['embed_bgr_readback plain']:.3f} vs three launches "
              f"{m['three launches']:.3f}")
        if old is not None:
            p = {k: m[f"embed_readback gray, {k}"] - m[f"embed gray, {k}"] for k in ("this a", "this b", "before a", "before b")}
            print(f"    gray pass: this build {p['this a']:.3f} / {p['this b']:.3f}   build before {p['before a']:.3f} / "
                  f"{p['before b']:.3f}   (two runs of each: their difference is the spread)")
for p in (d_bgr, d_out, d_gray, d_stego, d_counts, d_bits, d_ext):
    lib.svs_free(p)
