"""Cost of the keyed read-back pass (svs_embed_dithered_readback_dev) and what its presence costs the two read-back calls that
were there before, at n = 10, delta = 20, full-capacity payload.  Everything is alternated in the same rounds of one process,
each call timed with a pair of HIP events on the null stream (torch.cuda.Event; the library's calls are enqueued on it):
  embed_dithered / embed_dithered_readback       a keyed dither with the zig-zag selection of 10, on noise and on letterboxed
                                                 noise; pass = the difference; the counts of one call
  embed_select / embed_dithered_readback         the same without the dither (dither NULL)
  embed_readback, embed_bgr_readback             this build against --baseline-lib (the parent commit's library:
                                                 `make -C csrc pre_keyed_readback`), twice each ("a" / "b": the difference between
                                                 two runs of the same library is the spread the comparison is read against)
Output: profiles/keyed_readback_rates.txt (--out).

    python tools/keyed_readback_rates.py [--frames 200 --h 2160 --w 3840 --rounds 7 --baseline-lib PATH]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd")
sys.path.insert(0, PKG)

from svsdct import batch, coeffs, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--delta", type=float, default=20.0)
ap.add_argument("--n-ac", type=int, default=10)
ap.add_argument("--baseline-lib", default=os.path.join(PKG, "lib", "variants", "libsvsdct_pre_keyed_readback.so"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_readback_rates.txt"))
args = ap.parse_args()

native.ensure_device(0)
lib = native.load()
f, h, w, n_ac, delta = args.frames, args.h, args.w, args.n_ac, float(args.delta)
planes = Planes.contiguous(f, h, w)
wide = Planes.contiguous(f, h, 3 * w)          # the BGR frames seen as planes of 3 w bytes per row, to fill them
rp, fp = 3 * w, 3 * w * h
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def dev(n):
    p = C.c_void_p()
    native.check(lib.svs_malloc(C.byref(p), n), "svs_malloc")
    return p


def sync():
    native.check(lib.svs_stream_synchronize(None), "sync")


d_bgr, d_out, d_gray, d_stego, d_counts = dev(f * fp), dev(f * fp), dev(f * h * w), dev(f * h * w), dev(16)
cap = batch.capacity_bits(f, h, w, n_ac)
d_bits = dev((cap + 7) // 8 + 8)
native.check(lib.svs_fill_bits_dev(d_bits, cap, 7, 0, None), "fill_bits")
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
old = None
if os.path.exists(args.baseline_lib):
    old = C.CDLL(args.baseline_lib)
    for name in ("svs_embed_readback_dev", "svs_embed_bgr_readback_dev"):
        getattr(old, name).restype, getattr(old, name).argtypes = native.SIGNATURES[name]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def counts_of(fn):
    native.check(lib.svs_memset(d_counts, 0, 16, None), "memset")
    fn()
    sync()
    out = np.zeros(2, np.uint64)
    native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_counts, 16, None), "d2h")
    sync()
    return int(out[0]), int(out[1])


done, P, ck = C.c_uint64(0), C.byref(planes), native.check
sel = coeffs.native_coeffs(coeffs.scan("zigzag", 1, n_ac))
dith = native.Dither(0x0123456789ABCDEF, 0, 0)
S, D = C.byref(sel), C.byref(dith)


def keyed_calls():
    return {
        "embed_dithered": lambda: ck(lib.svs_embed_dithered_dev(d_gray, d_stego, P, None, S, D, delta, n_ac, d_bits, 0, cap, G,
                                                                C.byref(done), None), "dithered"),
        "embed_dithered_readback": lambda: ck(lib.svs_embed_dithered_readback_dev(d_gray, d_stego, P, None, S, D, delta, n_ac, d_bits,
                                                                                  0, cap, G, C.byref(done), d_counts, None), "dithered_rb"),
        "embed_select": lambda: ck(lib.svs_embed_select_dev(d_gray, d_stego, P, None, S, delta, d_bits, 0, cap, G, C.byref(done), None),
                                   "select"),
        "embed_dithered_readback, no dither": lambda: ck(lib.svs_embed_dithered_readback_dev(d_gray, d_stego, P, None, S, None, delta,
                                                                                             n_ac, d_bits, 0, cap, G, C.byref(done),
                                                                                             d_counts, None), "select_rb"),
    }


def old_calls():
    def gray(which):
        return lambda: ck(which.svs_embed_readback_dev(d_gray, d_stego, P, None, delta, n_ac, d_bits, 0, cap, G, C.byref(done),
                                                       d_counts, None), "embed_rb")

    def bgr(which):
        return lambda: ck(which.svs_embed_bgr_readback_dev(d_bgr, rp, fp, d_out, rp, fp, None, P, None, delta, n_ac, d_bits, 0, cap, G,
                                                           C.byref(done), d_counts, None), "bgr_rb")
    out = {}
    for tag in ("a", "b"):
        out[f"embed_readback, this {tag}"] = gray(lib)
        out[f"embed_bgr_readback, this {tag}"] = bgr(lib)
        if old is not None:
            out[f"embed_readback, parent {tag}"] = gray(old)
            out[f"embed_bgr_readback, parent {tag}"] = bgr(old)
    return out


def measure(todo):
    for fn in todo.values():
        timed(fn)
    t = {k: [] for k in todo}
    for _ in range(args.rounds):
        for k, fn in todo.items():
            t[k].append(timed(fn))
    for k, v in t.items():
        say(f"    {k:38s} {statistics.median(v):8.3f} / {min(v):8.3f}   spread {max(v) - min(v):6.3f}")
    return {k: statistics.median(v) for k, v in t.items()}


say(f"keyed read-back cost, {f} x {w}x{h}, delta {delta:g}, n {n_ac} (zig-zag selection), guarded flags, full-capacity payload, "
    f"{args.rounds} alternated rounds, HIP events; median / min ms per call")
if old is None:
    say(f"(no baseline library at {os.path.relpath(args.baseline_lib, ROOT)}: this build only)")
for kind in ("noise", "letterbox"):
    content(kind)
    say(f"{kind}")
    todo = keyed_calls()
    m = measure(todo)
    c1 = counts_of(todo["embed_dithered_readback"])
    c2 = counts_of(todo["embed_dithered_readback, no dither"])
    blocks = f * (h // 8) * (w // 8)
    say(f"    pass with the dither {m['embed_dithered_readback'] - m['embed_dithered']:.3f} ms "
        f"({m['embed_dithered_readback'] / m['embed_dithered']:.2f} x the call without it); counts (repaired, unrepaired) {c1} of "
        f"{blocks} blocks")
    say(f"    pass without a dither {m['embed_dithered_readback, no dither'] - m['embed_select']:.3f} ms "
        f"({m['embed_dithered_readback, no dither'] / m['embed_select']:.2f} x); counts {c2}")
    m = measure(old_calls())
    for name in ("embed_readback", "embed_bgr_readback"):
        text = f"    {name}: this build {m[name + ', this a']:.3f} / {m[name + ', this b']:.3f}"
        if old is not None:
            text += f"   parent {m[name + ', parent a']:.3f} / {m[name + ', parent b']:.3f}"
        say(text + "   (two runs of each: their difference is the spread)")
for p in (d_bgr, d_out, d_gray, d_stego, d_counts, d_bits):
    lib.svs_free(p)
with open(args.out, "w") as out:
    out.write("\n".join(lines) + "\n")
