"""Cost of the per-coefficient QIM steps (include/svsdct.h svs_stepped_embed_dev / svs_stepped_extract_dev), 200 x 3840x2160 gray
frames of noise in [16, 240).  One process; each call is timed with a pair of HIP events on the null stream, the sides of a
comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the calls that existed, this build against the baseline library (the parent commit's): the two delta = 7.3 exact embeds
     (n_ac = 20 and 63) and the channel, which run the embed instantiations that now also hold the stepped side; the hard
     eight-row extracts at delta = 8 (the QM_POW2 instantiations, which hold it too) and 20, n_ac = 10 (a zig-zag selection) and
     63; and the soft call.  The yardstick is the baseline's own run-to-run spread in the same process (ratelib.verdict); a
     call outside it is reported as a cost, with both medians.
  2. svs_stepped_embed_dev / svs_stepped_extract_dev with a uniform table of 20 against svs_embed_select_dev /
     svs_extract_select_dev at delta = 20 and the same selection (the zig-zag scan from position 6: never a prefix), counts 3, 10
     and 63, in this build.  The stepped side divides in IEEE float32 per payload coefficient where the existing side multiplies
     by 1 / delta and divides only near a tie.  No threshold: the medians and ratios are the result.
Output: profiles/stepped_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc baseline REV=<parent commit> NAME=pre_stepped
    python tools/stepped_rates.py --reps 15 \\
        --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_stepped.so
"""
import ctypes as C
import statistics

import ratelib
from ratelib import X, coeffs, native
from svsdct import channel, steps

DELTA = 20.0
COUNTS = (3, 10, 63)


def selection(count):
    """`count` coefficients along the zig-zag scan from position 6 (63: the whole scan from position 1) - no prefix"""
    return coeffs.native_coeffs(coeffs.selection("zigzag:6" if count < 58 else "zigzag", count))


def main():
    args = ratelib.parser("stepped_rates.txt", reps=15, baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline(ratelib.variant_path("pre_stepped"))
    s.noise()
    table = steps.steps_struct(steps.uniform(int(DELTA)))
    q75 = channel.steps_struct(75)

    def stepped_embed(sel):
        cap = s.capacity(sel.count)
        return lambda: native.check(lib.svs_stepped_embed_dev(s.gray, s.stego, s.P, None, C.byref(sel), None, C.byref(table), 0, s.bits,
                                                              0, cap, X, C.byref(s.done), None), "svs_stepped_embed_dev")

    def stepped_extract(sel):
        return lambda: native.check(lib.svs_stepped_extract_dev(s.stego, s.P, None, C.byref(sel), None, C.byref(table), 0, s.ext,
                                                                s.packed_bytes, X, C.byref(s.done), None), "svs_stepped_extract_dev")

    def requantise(so):
        return lambda: native.check(so.svs_requantise_dev(s.gray, s.stego, s.P, C.byref(q75), 0, None), "svs_requantise_dev")

    s.say(f"per-coefficient QIM steps, {s.f} x {s.w}x{s.h} gray, noise in [16, 240), {args.reps} alternated repetitions "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")
    if base is not None:
        s.say("1. the calls that existed: this build against the baseline (the parent commit's library)")
        d_soft = s.dev(s.cap_max)
        zz10 = coeffs.native_coeffs(coeffs.selection("zigzag", 10))
        cases = [(f"exact embed n {n}, delta 7.3", lambda so, n=n: s.embed(so, 7.3, n, X)) for n in (20, 63)]
        cases.append(("channel, quality 75", requantise))
        for d in (8.0, DELTA):
            cases.append((f"extract, zig-zag selection of 10, delta {d:g}", lambda so, d=d: s.extract_select(so, zz10, d, X)))
            cases.append((f"extract n 63, delta {d:g}", lambda so, d=d: s.extract(so, d, 63, X)))
        cases.append(("soft extract n 10, delta 20", lambda so: s.soft(so, DELTA, 10, d_soft)))
        s.against_baseline((what, make(base), make(lib)) for what, make in cases)
    else:
        s.say("1. no baseline library: the calls that existed were not compared")

    s.say("2. stepped calls with a uniform table of 20 against the select calls at delta = 20, the same selection, this build")
    s.noise()
    for count in COUNTS:
        sel = selection(count)
        for what, old, new in ((f"embed, {count} coefficients", s.embed_select(lib, sel, DELTA, X), stepped_embed(sel)),
                               (f"extract, {count} coefficients", s.extract_select(lib, sel, DELTA, X), stepped_extract(sel))):
            t = s.measure({"select call": old, "stepped call": new})
            s.say(f"  {what}")
            s.report_rows(t)
            s.say(f"    ratio stepped / select {statistics.median(t['stepped call']) / statistics.median(t['select call']):.3f}")
    s.close()


if __name__ == "__main__":
    main()
