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
import ctypes as C
import statistics

import ratelib
from ratelib import G, native


def main():
    ap = ratelib.parser("colour_readback_rates.txt", reps=7, rounds=True, baseline="optional")
    ap.add_argument("--configs", default="8:3,20:10,7.5:20", help="delta:n_ac,... (7.5:20: eight coefficient rows, no power of two)")
    args = ap.parse_args()
    s = ratelib.Session(args)
    s.bgr_buffers(s.f)
    lib, old, ck = s.lib, s.baseline(ratelib.variant_path("pre_colour")), native.check
    rp, fp, P = s.rp, s.fp, s.P

    def calls(delta, n_ac):
        cap = s.capacity(n_ac)

        def three():
            ck(lib.svs_bgr_to_gray_dev(s.bgr, rp, fp, s.stego, P, None, None), "to_gray")
            ck(lib.svs_embed_readback_dev(s.stego, s.stego, P, None, delta, n_ac, s.bits, 0, cap, G, C.byref(s.done), s.small, None), "rb")
            ck(lib.svs_gray_to_bgr_dev(s.stego, P, s.bgr_out, rp, fp, None), "to_bgr")

        todo = {
            "embed_bgr plain": s.embed_bgr(lib, delta, n_ac, G), "embed_bgr_readback plain": s.embed_bgr_readback(lib, delta, n_ac, G),
            "embed_bgr keep": s.embed_bgr(lib, delta, n_ac, G | native.SVS_KEEP_COLOUR),
            "embed_bgr_readback keep": s.embed_bgr_readback(lib, delta, n_ac, G | native.SVS_KEEP_COLOUR),
            "extract_bgr": lambda: ck(lib.svs_extract_bgr_dev(s.bgr_out, rp, fp, P, None, delta, n_ac, s.ext, s.packed_bytes,
                                                              C.byref(s.done), None), "extract_bgr"),
            "three launches": three,
            "embed gray": s.embed(lib, delta, n_ac, G), "embed_readback gray": s.embed_readback(lib, delta, n_ac, G),
        }
        if old is not None:
            for tag in ("a", "b"):
                todo[f"embed_readback gray, this {tag}"] = s.embed_readback(lib, delta, n_ac, G)
                todo[f"embed_readback gray, before {tag}"] = s.embed_readback(old, delta, n_ac, G)
                todo[f"embed gray, this {tag}"] = s.embed(lib, delta, n_ac, G)
                todo[f"embed gray, before {tag}"] = s.embed(old, delta, n_ac, G)
        return todo

    s.say(f"colour read-back cost, {s.f} x {s.w}x{s.h} BGR, guarded, full-capacity payload, {args.reps} alternated rounds "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")
    for delta, n_ac in ratelib.configs(args.configs):
        for kind in ("noise", "letterbox"):
            s.content(kind, bgr=True)
            t = s.measure(calls(delta, n_ac))
            s.say(f"delta {delta:g} n {n_ac} {kind}")
            s.report_rows(t)
            m = {k: statistics.median(v) for k, v in t.items()}
            s.say(f"    colour pass plain {m['embed_bgr_readback plain'] - m['embed_bgr plain']:.3f}  keep "
                  f"{m['embed_bgr_readback keep'] - m['embed_bgr keep']:.3f}  gray pass {m['embed_readback gray'] - m['embed gray']:.3f}  "
                  f"extract_bgr {m['extract_bgr']:.3f}  plain fused {m['embed_bgr_readback plain']:.3f} vs three launches "
                  f"{m['three launches']:.3f}")
            if old is not None:
                p = {k: m[f"embed_readback gray, {k}"] - m[f"embed gray, {k}"] for k in ("this a", "this b", "before a", "before b")}
                s.say(f"    gray pass: this build {p['this a']:.3f} / {p['this b']:.3f}   build before {p['before a']:.3f} / "
                      f"{p['before b']:.3f}   (two runs of each: their difference is the spread)")
    s.close()


if __name__ == "__main__":
    main()
