"""Cost of the soft, vote and histogram calls under per-coefficient steps (include/svsdct.h svs_stepped_soft_*_dev), 200 x
3840x2160 gray frames of noise in [16, 240).  One process; each call is timed with a pair of HIP events on the null stream, the
sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the calls that existed, this build against the baseline library (the parent commit's): the hard eight-row extracts at
     delta = 8 (the QM_POW2 instantiations, which now also hold the stepped soft side) and delta = 20, at n_ac = 63 and with a
     zig-zag selection of 10; svs_stepped_extract_dev with a uniform table of 20; svs_soft_extract_dev at n_ac = 10 for delta = 8
     and 20; the vote at period 10^6 and the histogram at n_ac = 10, delta = 8 and 20.  The yardstick is the baseline's own
     run-to-run spread in the same process (ratelib.verdict); a call outside it is reported as a cost, with both medians.
  2. svs_stepped_soft_extract_dev / _vote_dev / _histogram_dev with a uniform table of 20 against svs_soft_extract_dev /
     svs_soft_vote_dev / svs_soft_histogram_dev at delta = 20 and the same selection (the zig-zag scan from position 6: never a
     prefix), counts 3, 10 and 63, the vote at periods 10^6 and 2 400, in this build.  The stepped side divides twice in IEEE
     float32 per payload coefficient where the existing side multiplies.  No threshold: the medians and ratios are the result.
Output: profiles/stepped_soft_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc baseline REV=<parent commit> NAME=pre_stepped_soft
    python tools/stepped_soft_rates.py --reps 15 \\
        --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_stepped_soft.so
"""
import ctypes as C
import statistics

import ratelib
from ratelib import X, coeffs, native
from svsdct import steps

DELTA = 20.0
COUNTS = (3, 10, 63)
PERIODS = (1_000_000, 2_400)


def selection(count):
    """`count` coefficients along the zig-zag scan from position 6 (63: the whole scan from position 1) - no prefix"""
    return coeffs.native_coeffs(coeffs.selection("zigzag:6" if count < 58 else "zigzag", count))


def main():
    args = ratelib.parser("stepped_soft_rates.txt", reps=15, baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline(ratelib.variant_path("pre_stepped_soft"))
    s.noise()
    table = steps.steps_struct(steps.uniform(int(DELTA)))
    d_soft = s.dev(s.cap_max)
    d_tally = s.dev(4 * max(PERIODS))
    d_hist = s.dev(1024 * s.f)
    native.check(lib.svs_memset(d_tally, 0, 4 * max(PERIODS), None), "memset")
    native.check(lib.svs_memset(d_hist, 0, 1024 * s.f, None), "memset")
    ratelib.sync()
    T = C.byref(table)

    # the tally and the rows are added to call after call and never read: timings, not decodes
    def soft(so, sel, delta=DELTA, n_ac=0):
        S = None if sel is None else C.byref(sel)
        return lambda: native.check(so.svs_soft_extract_dev(s.stego, s.P, None, S, None, float(delta), n_ac, d_soft, s.cap_max, X,
                                                            C.byref(s.done), None), "svs_soft_extract_dev")

    def vote(so, sel, period, delta=DELTA, n_ac=0):
        S = None if sel is None else C.byref(sel)
        return lambda: native.check(so.svs_soft_vote_dev(s.stego, s.P, None, S, None, float(delta), n_ac, period, 0, d_tally, 0,
                                                         C.byref(s.done), None), "svs_soft_vote_dev")

    def hist(so, sel, delta=DELTA, n_ac=0):
        S = None if sel is None else C.byref(sel)
        return lambda: native.check(so.svs_soft_histogram_dev(s.stego, s.P, S, None, float(delta), n_ac, d_hist, 0, C.byref(s.done), None),
                                    "svs_soft_histogram_dev")

    def stepped_extract(so, sel):
        return lambda: native.check(so.svs_stepped_extract_dev(s.stego, s.P, None, C.byref(sel), None, T, 0, s.ext, s.packed_bytes, X,
                                                               C.byref(s.done), None), "svs_stepped_extract_dev")

    def stepped_soft(sel):
        return lambda: native.check(lib.svs_stepped_soft_extract_dev(s.stego, s.P, None, C.byref(sel), None, T, 0, d_soft, s.cap_max, X,
                                                                     C.byref(s.done), None), "svs_stepped_soft_extract_dev")

    def stepped_vote(sel, period):
        return lambda: native.check(lib.svs_stepped_soft_vote_dev(s.stego, s.P, None, C.byref(sel), None, T, 0, period, 0, d_tally, 0,
                                                                  C.byref(s.done), None), "svs_stepped_soft_vote_dev")

    def stepped_hist(sel):
        return lambda: native.check(lib.svs_stepped_soft_histogram_dev(s.stego, s.P, C.byref(sel), None, T, 0, d_hist, 0,
                                                                       C.byref(s.done), None), "svs_stepped_soft_histogram_dev")

    s.say(f"soft, vote and histogram under per-coefficient QIM steps, {s.f} x {s.w}x{s.h} gray, noise in [16, 240), {args.reps} "
          f"alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.embed(lib, DELTA, 63, X)()      # the stego every call reads: delta = 20, n_ac = 63
    ratelib.sync()
    if base is not None:
        s.say("1. the calls that existed: this build against the baseline (the parent commit's library)")
        zz10 = coeffs.native_coeffs(coeffs.selection("zigzag", 10))
        zz6 = selection(10)
        cases = []
        for d in (8.0, DELTA):
            cases.append((f"extract, zig-zag selection of 10, delta {d:g}", lambda so, d=d: s.extract_select(so, zz10, d, X)))
            cases.append((f"extract n 63, delta {d:g}", lambda so, d=d: s.extract(so, d, 63, X)))
        cases.append(("stepped extract, uniform 20, 10 coefficients", lambda so: stepped_extract(so, zz6)))
        for d in (8.0, DELTA):
            cases.append((f"soft extract n 10, delta {d:g}", lambda so, d=d: soft(so, None, d, 10)))
        for d in (8.0, DELTA):
            cases.append((f"soft vote n 10, period 1000000, delta {d:g}", lambda so, d=d: vote(so, None, PERIODS[0], d, 10)))
        for d in (8.0, DELTA):
            cases.append((f"soft histogram n 10, delta {d:g}", lambda so, d=d: hist(so, None, d, 10)))
        s.against_baseline((what, make(base), make(lib)) for what, make in cases)
    else:
        s.say("1. no baseline library: the calls that existed were not compared")

    s.say("2. stepped soft calls with a uniform table of 20 against the soft calls at delta = 20, the same selection, this build")
    for count in COUNTS:
        sel = selection(count)
        pairs = [(f"soft extract, {count} coefficients", soft(lib, sel), stepped_soft(sel))]
        pairs += [(f"soft vote, {count} coefficients, period {p}", vote(lib, sel, p), stepped_vote(sel, p)) for p in PERIODS]
        pairs.append((f"soft histogram, {count} coefficients", hist(lib, sel), stepped_hist(sel)))
        for what, old, new in pairs:
            t = s.measure({"soft call": old, "stepped soft call": new})
            s.say(f"  {what}")
            s.report_rows(t)
            s.say(f"    ratio stepped / soft {statistics.median(t['stepped soft call']) / statistics.median(t['soft call']):.3f}")
    s.close()


if __name__ == "__main__":
    main()
