"""Cost of the soft-decision extraction (include/svsdct.h svs_soft_extract_dev), gray frames of synthetic noise in [16, 240)
carrying a full-capacity payload, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the
two sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the soft call against svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac (n = 3, 10, 63): ratio, and the run-to-run
     spread of each side.  The soft call writes eight times the bytes and always runs the eight-row kernel; at n = 3 and 10 the
     hard call runs the one- and two-row instantiations.
  2. the hard eight-row calls - n = 63, a zig-zag selection, a dither -, this build against the baseline library (the parent
     commit's): the soft side shares their four instantiations.  This build's median should lie inside the baseline's own
     min-max spread.
Nobody has measured these times yet, so no ratio is expected: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_extract_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_soft      # lib/variants/libsvsdct_pre_soft.so, from git
    python tools/soft_extract_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_soft.so
"""
import statistics

import ratelib
from ratelib import KEY, X, coeffs

DELTA = 20.0


def main():
    args = ratelib.parser("soft_extract_rates.txt", baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline()
    d_soft = s.dev(s.cap_max + 8)
    s.noise()
    s.say(f"soft-decision extraction, {s.f} x {s.w}x{s.h} gray noise in [16, 240), full-capacity payload, delta = {DELTA:g}, "
          f"{args.reps} alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.say("1. the soft call against svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac")
    for n_ac in (3, 10, 63):
        s.embed(lib, DELTA, n_ac, X)()                 # the stego the extract calls read: a full payload at n_ac
        t = s.measure({"hard": s.extract(lib, DELTA, n_ac, X), "soft": s.soft(lib, DELTA, n_ac, d_soft)})
        s.report_rows(t, f"n {n_ac} ")
        s.say(f"    n {n_ac} ratio soft / hard = {statistics.median(t['soft']) / statistics.median(t['hard']):.3f}  "
              f"(spread hard {ratelib.spread(t['hard']):.1f} %, soft {ratelib.spread(t['soft']):.1f} %)")

    if base is not None:
        s.say("2. the hard eight-row extract calls: this build against the baseline (the parent commit's library)")
        s.embed(lib, DELTA, 63, X)()
        sel = coeffs.native_coeffs(coeffs.selection("zigzag", 10))
        s.against_baseline((f"extract {what}", make(base), make(lib)) for what, make in (
            ("n 63", lambda so: s.extract(so, DELTA, 63, X)),
            ("zig-zag selection of 10", lambda so: s.extract_select(so, sel, DELTA, X)),
            ("dither, n 10", lambda so: s.extract_dithered(so, KEY, DELTA, 10, X))))
    s.close()


if __name__ == "__main__":
    main()
