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
import ctypes as C
import os
import statistics

import ratelib
from ratelib import G, KEY, coeffs, native


def main():
    ap = ratelib.parser("keyed_readback_rates.txt", reps=7, rounds=True, baseline="optional")
    ap.add_argument("--delta", type=float, default=20.0)
    ap.add_argument("--n-ac", type=int, default=10)
    args = ap.parse_args()
    s = ratelib.Session(args)
    s.bgr_buffers(s.f)
    default = ratelib.variant_path("pre_keyed_readback")
    lib, old, n_ac, delta = s.lib, s.baseline(default), args.n_ac, args.delta
    sel = coeffs.native_coeffs(coeffs.scan("zigzag", 1, n_ac))
    dith = native.Dither(KEY, 0, 0)
    cap, blocks = s.capacity(n_ac), s.f * (s.h // 8) * (s.w // 8)

    def keyed_readback(dither):
        return lambda: native.check(lib.svs_embed_dithered_readback_dev(
            s.gray, s.stego, s.P, None, C.byref(sel), dither, delta, n_ac, s.bits, 0, cap, G, C.byref(s.done), s.small, None),
            "svs_embed_dithered_readback_dev")

    def keyed_calls():
        return {"embed_dithered": s.embed_dithered(lib, KEY, delta, n_ac, G, sel),
                "embed_dithered_readback": keyed_readback(C.byref(dith)),
                "embed_select": s.embed_select(lib, sel, delta, G),
                "embed_dithered_readback, no dither": keyed_readback(None)}

    def old_calls():
        out = {}
        for tag in ("a", "b"):
            out[f"embed_readback, this {tag}"] = s.embed_readback(lib, delta, n_ac, G)
            out[f"embed_bgr_readback, this {tag}"] = s.embed_bgr_readback(lib, delta, n_ac, G)
            if old is not None:
                out[f"embed_readback, parent {tag}"] = s.embed_readback(old, delta, n_ac, G)
                out[f"embed_bgr_readback, parent {tag}"] = s.embed_bgr_readback(old, delta, n_ac, G)
        return out

    def measure(todo):
        t = s.measure(todo)
        s.report_rows(t, width=38)
        return t, {k: statistics.median(v) for k, v in t.items()}

    s.say(f"keyed read-back cost, {s.f} x {s.w}x{s.h}, delta {delta:g}, n {n_ac} (zig-zag selection), guarded flags, full-capacity "
          f"payload, {args.reps} alternated rounds ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    if old is None:
        s.say(f"(no baseline library at {os.path.relpath(default, ratelib.ROOT)}: this build only)")
    for kind in ("noise", "letterbox"):
        s.content(kind, bgr=True)
        s.say(f"{kind}")
        todo = keyed_calls()
        _, m = measure(todo)
        c1 = s.counts_of(todo["embed_dithered_readback"])
        c2 = s.counts_of(todo["embed_dithered_readback, no dither"])
        s.say(f"    pass with the dither {m['embed_dithered_readback'] - m['embed_dithered']:.3f} ms "
              f"({m['embed_dithered_readback'] / m['embed_dithered']:.2f} x the call without it); counts (repaired, unrepaired) {c1} of "
              f"{blocks} blocks")
        s.say(f"    pass without a dither {m['embed_dithered_readback, no dither'] - m['embed_select']:.3f} ms "
              f"({m['embed_dithered_readback, no dither'] / m['embed_select']:.2f} x); counts {c2}")
        t, m = measure(old_calls())
        for name in ("embed_readback", "embed_bgr_readback"):
            text = f"    {name}: this build {m[name + ', this a']:.3f} / {m[name + ', this b']:.3f}"
            if old is not None:
                text += f"   parent {m[name + ', parent a']:.3f} / {m[name + ', parent b']:.3f}"
            s.say(text + "   (two runs of each: their difference is the spread)")
            if old is not None:        # both runs of each side together
                parent, this = (t[f"{name}, {side} a"] + t[f"{name}, {side} b"] for side in ("parent", "this"))
                s.say(ratelib.verdict(parent, this)[1])
    s.close()


if __name__ == "__main__":
    main()
