"""The harness of the feature rate scripts (tools/*_rates.py): the common options, a session on device 0 (libraries, tracked
buffers, fills, read-back of small results, the report), event timing with alternated sides, the report rows and the one
verdict rule, and the call builders more than one script uses.  Importing it needs neither torch nor a GPU; torch is imported
where the session starts.

The verdict rule: a build is inside the baseline's spread if and only if min(baseline) <= median(this build) <= max(baseline),
the baseline's times taken alternately in the same process; otherwise it is BELOW (faster than) or ABOVE (slower than) it.
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "secure-video-steganography-using-ecc-and-dct_amd")
sys.path.insert(0, PKG)

from svsdct import batch, coeffs, native  # noqa: E402
from svsdct.native import Planes  # noqa: E402

G, X = native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT
KEY = 0x0123456789ABCDEF


def variant_path(name):
    return os.path.join(PKG, "lib", "variants", f"libsvsdct_{name}.so")


def parser(out, frames=200, reps=5, rounds=False, baseline=None):
    """the options every rate script takes.  rounds: --rounds stays an alias of --reps.  baseline: None (the script compares no
    builds), "required" or "optional" (what a script does without one: Session.baseline)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=frames)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--reps", *(["--rounds"] if rounds else []), type=int, default=reps, help="alternating repetitions per side")
    ap.add_argument("--fixed-order", action="store_true", help="the same order of the calls in every repetition (no rotation)")
    if baseline:
        ap.add_argument("--baseline-lib", required=baseline == "required", default=None,
                        help="the library of the parent commit, timed alternately with this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    return ap


def configs(text):
    """"delta:n_ac,..." -> [(delta, n_ac)]"""
    return [(float(c.split(":")[0]), int(c.split(":")[1])) for c in text.split(",") if c]


def load_build(path):
    """another build of the library, with the prototype of every entry point it has (a library of an earlier commit lacks
    the newer ones).  The same swap testlib.using_library makes: another CDLL, same prototypes"""
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in native.SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    return lib


def sync():
    native.check(native.load().svs_stream_synchronize(None), "sync")


_torch = None      # imported by the session, which a script makes before it times anything


def timed(fn):
    """ms of one call between a pair of HIP events on the null stream (torch.cuda.Event; the library's calls with stream NULL
    are enqueued on the same stream).  A call that works in place carries its own `prepare`, run before the first event"""
    a, b = _torch.cuda.Event(enable_timing=True), _torch.cuda.Event(enable_timing=True)
    getattr(fn, "prepare", lambda: None)()
    sync()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(todo, reps, rotate=True, timed=timed):
    """name -> times over reps repetitions of every call in todo, after one warm-up each; the starting side advances by one
    per repetition, so that no call always runs behind the same neighbour, unless the order is fixed"""
    for fn in todo.values():
        timed(fn)
    t = {k: [] for k in todo}
    names = list(todo)
    for r in range(reps):
        shift = r % len(names) if rotate else 0
        for k in names[shift:] + names[:shift]:
            t[k].append(timed(todo[k]))
    return t


def row(k, v, width=34):
    return f"    {k:{width}s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"


def spread(v):
    return 100 * (max(v) - min(v)) / statistics.median(v)


def verdict(baseline_times, this_times):
    """(inside, the report's sentence) by the rule of the module docstring"""
    lo, hi, m = min(baseline_times), max(baseline_times), statistics.median(this_times)
    where = "inside" if lo <= m <= hi else "BELOW (faster than)" if m < lo else "ABOVE (slower than)"
    return where == "inside", f"    this build's median is {where} the baseline's spread"


class Session:
    """Device 0, this build's library, the gray buffers every script uses (cover, stego, a full payload at n_ac = 63, room for
    its extraction), every other buffer the script asks for, and the report."""

    def __init__(self, args):
        # torch, for the events, comes before the library touches the device: it brings a HIP runtime of its own, and imported
        # after svs_init it finds no GPU
        global _torch
        import torch as _torch
        native.ensure_device(0)
        self.lib = native.load()
        _torch.cuda.init()
        _torch.cuda.current_stream()          # the default (null) stream: the one the library's calls with stream NULL use
        self.args = args
        self.f, self.h, self.w = f, h, w = args.frames, args.h, args.w
        self.planes, self.one = Planes.contiguous(f, h, w), Planes.contiguous(1, h, w)
        self.P = C.byref(self.planes)
        self.done = C.c_uint64(0)
        self.lines, self.buffers = [], []
        self.cap_max = self.capacity(63)
        self.packed_bytes = (self.cap_max + 7) // 8 + 8
        self.gray, self.stego = self.dev(f * h * w), self.dev(f * h * w)
        self.bits, self.ext = self.dev(self.packed_bytes), self.dev(self.packed_bytes)
        self.small = self.dev(16)                  # a uint64 result, or the two counts of a read-back call
        native.check(self.lib.svs_fill_bits_dev(self.bits, self.cap_max, 7, 0, None), "fill_bits")
        sync()

    def baseline(self, default=None):
        """the --baseline-lib build; without the option, the build at the default path if that file exists, or None"""
        path = self.args.baseline_lib or (default if default and os.path.exists(default) else None)
        return load_build(path) if path else None

    def order_text(self):
        return "fixed order" if self.args.fixed_order else "order rotated"

    def capacity(self, n_ac, frames=None):
        return batch.capacity_bits(frames or self.f, self.h, self.w, n_ac)

    def dev(self, n):
        p = C.c_void_p()
        native.check(self.lib.svs_malloc(C.byref(p), n), "svs_malloc")
        self.buffers.append(p)
        return p

    def bgr_buffers(self, frames):
        """BGR input and output frames; `wide` sees them as planes of 3 w bytes per row, to fill them"""
        self.rp, self.fp = 3 * self.w, 3 * self.w * self.h
        self.bplanes, self.wide = Planes.contiguous(frames, self.h, self.w), Planes.contiguous(frames, self.h, 3 * self.w)
        self.bgr, self.bgr_out = self.dev(frames * self.fp), self.dev(frames * self.fp)

    def say(self, text=""):
        print(text, flush=True)
        self.lines.append(text)

    def close(self):
        """frees the buffers and writes the report"""
        for p in self.buffers:
            self.lib.svs_free(p)
        with open(self.args.out, "w") as fh:
            fh.write("\n".join(self.lines) + "\n")

    # ---- contents ----
    def noise(self, bgr=False, lo=16, span=224):
        buf, planes = (self.bgr, self.wide) if bgr else (self.gray, self.planes)
        native.check(self.lib.svs_fill_synthetic_dev(buf, C.byref(planes), 1, 0, lo, span, None), "fill")
        sync()

    def content(self, kind, bgr=False):
        """noise in [0, 256); "letterbox": with black bars over a third of the rows.  bgr: the BGR frames, and their gray"""
        self.noise(bgr, 0, 256)
        buf, rp = (self.bgr, 3 * self.w) if bgr else (self.gray, self.w)
        bar = (self.h // 6) // 8 * 8
        if kind == "letterbox":
            for k in range(self.f):
                base = buf.value + k * self.h * rp
                native.check(self.lib.svs_memset(C.c_void_p(base), 0, bar * rp, None), "memset")
                native.check(self.lib.svs_memset(C.c_void_p(base + (self.h - bar) * rp), 0, bar * rp, None), "memset")
        if bgr:
            native.check(self.lib.svs_bgr_to_gray_dev(self.bgr, self.rp, self.fp, self.gray, self.P, None, None), "gray")
        sync()

    # ---- small results ----
    def counts(self):
        out = (C.c_uint64 * 2)()
        native.check(self.lib.svs_memcpy_d2h(out, self.small, 16, None), "d2h")
        sync()
        return int(out[0]), int(out[1])

    def scalar(self):
        return self.counts()[0]

    def counts_of(self, fn):
        """(repaired, unrepaired) of one read-back call"""
        native.check(self.lib.svs_memset(self.small, 0, 16, None), "memset")
        fn()
        return self.counts()

    def psnr_frame0(self):
        native.check(self.lib.svs_frame_sse_dev(self.gray, self.stego, C.byref(self.one), self.small, None), "sse")
        sse = self.scalar()
        return math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 * self.h * self.w / sse)

    def bit_errors(self, cap):
        """of the extracted bits against the payload"""
        native.check(self.lib.svs_bit_errors_dev(self.ext, self.bits, cap, self.small, None), "bit_errors")
        return self.scalar()

    # ---- timing and reporting ----
    def measure(self, todo):
        return alternate(todo, self.args.reps, not self.args.fixed_order)

    def report_rows(self, t, prefix="", width=34):
        for k, v in t.items():
            self.say(row(prefix + k, v, width))

    def against_baseline(self, cases):
        """cases: (title, the baseline's call, this build's call), made one at a time; each pair alternated, reported with the
        verdict, and the settings outside the baseline's spread counted"""
        outside = 0
        for title, old, new in cases:
            t = self.measure({"baseline": old, "this build": new})
            inside, sentence = verdict(t["baseline"], t["this build"])
            outside += not inside
            self.say(f"  {title}")
            self.report_rows(t)
            self.say(sentence)
        self.say(f"  settings outside the baseline's spread: {outside}")

    # ---- call builders: each returns the call of `lib` (this build's library or another build) as a function of nothing ----
    def embed(self, lib, delta, n_ac, flags):
        cap = self.capacity(n_ac)
        return lambda: native.check(lib.svs_embed_dev(self.gray, self.stego, self.P, float(delta), n_ac, self.bits, 0, cap, flags,
                                                      C.byref(self.done), None), "svs_embed_dev")

    def extract(self, lib, delta, n_ac, flags, src=None):
        src = src or self.stego
        return lambda: native.check(lib.svs_extract_dev(src, self.P, float(delta), n_ac, self.ext, self.packed_bytes, flags,
                                                        C.byref(self.done), None), "svs_extract_dev")

    def embed_select(self, lib, sel, delta, flags):
        cap = self.capacity(sel.count)
        return lambda: native.check(lib.svs_embed_select_dev(self.gray, self.stego, self.P, None, C.byref(sel), float(delta), self.bits,
                                                             0, cap, flags, C.byref(self.done), None), "svs_embed_select_dev")

    def extract_select(self, lib, sel, delta, flags):
        return lambda: native.check(lib.svs_extract_select_dev(self.stego, self.P, None, C.byref(sel), float(delta), self.ext,
                                                               self.packed_bytes, flags, C.byref(self.done), None),
                                    "svs_extract_select_dev")

    def embed_dithered(self, lib, key, delta, n_ac, flags, sel=None):
        cap = self.capacity(n_ac if sel is None else sel.count)
        d, S = native.Dither(key, 0, 0), None if sel is None else C.byref(sel)
        return lambda: native.check(lib.svs_embed_dithered_dev(self.gray, self.stego, self.P, None, S, C.byref(d), float(delta), n_ac,
                                                               self.bits, 0, cap, flags, C.byref(self.done), None),
                                    "svs_embed_dithered_dev")

    def extract_dithered(self, lib, key, delta, n_ac, flags, sel=None):
        d, S = native.Dither(key, 0, 0), None if sel is None else C.byref(sel)
        return lambda: native.check(lib.svs_extract_dithered_dev(self.stego, self.P, None, S, C.byref(d), float(delta), n_ac, self.ext,
                                                                 self.packed_bytes, flags, C.byref(self.done), None),
                                    "svs_extract_dithered_dev")

    def soft(self, lib, delta, n_ac, d_soft, src=None):
        src = src or self.stego
        return lambda: native.check(lib.svs_soft_extract_dev(src, self.P, None, None, None, float(delta), n_ac, d_soft, self.cap_max, X,
                                                             C.byref(self.done), None), "svs_soft_extract_dev")

    def vote(self, lib, delta, n_ac, period, d_tally, order=None):
        """the tally is added to call after call and never read: a timing, not a decode"""
        return lambda: native.check(lib.svs_soft_vote_dev(self.stego, self.P, order, None, None, float(delta), n_ac, period, 0, d_tally,
                                                          0, C.byref(self.done), None), "svs_soft_vote_dev")

    def eight_row_calls(self, delta, d_soft):
        """(title, library -> call) of the extract calls whose eight-row instantiations the soft tails share, on stego of n = 63"""
        sel = coeffs.native_coeffs(coeffs.selection("zigzag", 10))
        return [("extract n 63", lambda so: self.extract(so, delta, 63, X)),
                ("extract, zig-zag selection of 10", lambda so: self.extract_select(so, sel, delta, X)),
                ("extract, dither, n 10", lambda so: self.extract_dithered(so, KEY, delta, 10, X)),
                ("soft extract n 10", lambda so: self.soft(so, delta, 10, d_soft)),
                ("soft extract n 63", lambda so: self.soft(so, delta, 63, d_soft))]

    def embed_readback(self, lib, delta, n_ac, flags):
        cap = self.capacity(n_ac)
        return lambda: native.check(lib.svs_embed_readback_dev(self.gray, self.stego, self.P, None, float(delta), n_ac, self.bits, 0, cap,
                                                               flags, C.byref(self.done), self.small, None), "svs_embed_readback_dev")

    def embed_bgr(self, lib, delta, n_ac, flags):
        cap, rp, fp = self.capacity(n_ac, self.bplanes.n_frames), self.rp, self.fp
        return lambda: native.check(lib.svs_embed_bgr_dev(self.bgr, rp, fp, self.bgr_out, rp, fp, None, C.byref(self.bplanes), None,
                                                          float(delta), n_ac, self.bits, 0, cap, flags, C.byref(self.done), None),
                                    "svs_embed_bgr_dev")

    def embed_bgr_readback(self, lib, delta, n_ac, flags):
        cap, rp, fp = self.capacity(n_ac, self.bplanes.n_frames), self.rp, self.fp
        return lambda: native.check(lib.svs_embed_bgr_readback_dev(self.bgr, rp, fp, self.bgr_out, rp, fp, None, C.byref(self.bplanes),
                                                                   None, float(delta), n_ac, self.bits, 0, cap, flags,
                                                                   C.byref(self.done), self.small, None), "svs_embed_bgr_readback_dev")
