"""Cost of the fused per-frame soft histograms (include/svsdct.h svs_soft_histogram_dev), 200 x 3840x2160 gray frames,
delta = 20, n_ac = 3, 10 and 63, on two contents: never-embedded noise in [16, 240), whose rows are flat (every one of the 256
counters of a workgroup's table is hit), and reference-rule full-capacity stego of the same noise, whose rows are peaked (the
case in which LDS atomics of one instruction to one address serialise; how peaked is printed: the stego pixels are rounded, so
the bytes spread over some 64 values, not two).  One process; each call is timed with a pair of HIP events on the null stream,
the sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. svs_soft_histogram_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT) of the same build, per content
     and n_ac.  The histogram call writes no soft byte; what it adds instead is one LDS add per byte and at most 256 global
     atomics per workgroup and frame.  --variant-lib NAME=PATH times the histogram call of another build of the library beside
     it (how the counting was chosen: profiles/soft_histogram_variants.txt).
  2. the calls that existed - the hard eight-row calls (n = 63, a zig-zag selection, a dither), the soft call at n = 10 and 63
     and the vote at period 10^6 -, this build against the baseline library (the parent commit's): the histogram tail shares
     their instantiations.  The yardstick is the baseline's own run-to-run spread in the same process: this build's median
     should lie inside its min-max.
No ratio is asserted: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_histogram_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_hist      # lib/variants/libsvsdct_pre_hist.so, from git
    python tools/soft_histogram_rates.py --reps 15 \\
        --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_hist.so
"""
import ctypes as C
import statistics

import numpy as np

import ratelib
from ratelib import X, native

DELTA, N_ACS, PERIOD = 20.0, (3, 10, 63), 10 ** 6


def main():
    ap = ratelib.parser("soft_histogram_rates.txt", reps=15, baseline="optional")
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH",
                    help="another build of this library whose histogram call section 1 times beside this build's")
    args = ap.parse_args()
    s = ratelib.Session(args)
    lib, base, f = s.lib, s.baseline(), s.f
    variants = {v.split("=", 1)[0]: ratelib.load_build(v.split("=", 1)[1]) for v in args.variant_lib}
    d_soft, d_hist, d_tally = s.dev(s.cap_max + 8), s.dev(1024 * f), s.dev(4 * PERIOD)
    native.check(lib.svs_memset(d_tally, 0, 4 * PERIOD, None), "memset")
    s.noise()

    def histogram(which, n_ac, src):
        """the rows are added to call after call: 1 + reps calls of at most 129 600 * 63 bytes a frame stay far inside uint32"""
        return lambda: native.check(which.svs_soft_histogram_dev(src, s.P, None, None, DELTA, n_ac, d_hist, 0, C.byref(s.done), None),
                                    "svs_soft_histogram_dev")

    def histogram_rows(src, n_ac):
        """one histogram call into cleared rows -> [frames, 256]"""
        native.check(lib.svs_memset(d_hist, 0, 1024 * f, None), "memset")
        histogram(lib, n_ac, src)()
        out = np.zeros(256 * f, np.uint32)
        native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_hist, out.nbytes, None), "d2h")
        ratelib.sync()
        return out.reshape(f, 256)

    s.say(f"fused per-frame soft histograms, {f} x {s.w}x{s.h} gray, delta = {DELTA:g}, {args.reps} alternated repetitions "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.say("1. svs_soft_histogram_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT) of the same build")
    for n_ac in N_ACS:
        s.embed(lib, DELTA, n_ac, X)()                 # the stego the calls read: the reference rule, a full payload at n_ac
        for content, src in (("noise in [16, 240), never embedded", s.gray), ("reference-rule full-capacity stego", s.stego)):
            rows = histogram_rows(src, n_ac)
            top2 = np.sort(rows, axis=1)[:, -2:].sum() / rows.sum()
            s.say(f"  n_ac = {n_ac}, {content}: rows sum to {int(rows[0].sum())} a frame, {int((rows[0] != 0).sum())} entries of "
                  f"frame 0 are not 0, the two largest entries of a row hold {100 * top2:.1f} % of it")
            todo = {"hard": s.extract(lib, DELTA, n_ac, X, src), "soft": s.soft(lib, DELTA, n_ac, d_soft, src),
                    "histogram": histogram(lib, n_ac, src)}
            for name, so in variants.items():
                todo[f"histogram, {name}"] = histogram(so, n_ac, src)
            t = s.measure(todo)
            for k, v in t.items():
                s.say(ratelib.row(k, v) + f"  spread {ratelib.spread(v):.1f} %")
            for k in list(t)[2:]:
                s.say(f"    {k}: ratio to soft {statistics.median(t[k]) / statistics.median(t['soft']):.3f}, to hard "
                      f"{statistics.median(t[k]) / statistics.median(t['hard']):.3f}")

    if base is not None:
        s.say("2. the calls that existed: this build against the baseline (the parent commit's library)")
        s.embed(lib, DELTA, 63, X)()
        s.against_baseline((what, make(base), make(lib)) for what, make in s.eight_row_calls(DELTA, d_soft) + [
            (f"soft vote n 10, period {PERIOD}", lambda so: s.vote(so, DELTA, 10, PERIOD, d_tally))])
    s.close()


if __name__ == "__main__":
    main()
