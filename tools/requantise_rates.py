"""Cost of the requantisation channel (include/svsdct.h svs_requantise_dev), 200 x 3840x2160 gray frames of noise in
[16, 240).  One process; each call is timed with a pair of HIP events on the null stream, the sides of a comparison alternated
inside every repetition and the order rotated from one repetition to the next.
  1. svs_requantise_dev at quality 50, 75, 90 and with the all-ones table, out of place and in place, against
     svs_embed_dev(SVS_EXACT_POCKETFFT) of the same build at n_ac = 63, delta = 20 (a full payload).  Both move 2 B/pixel and run
     the same two transforms; per coefficient the channel has one division, one round and one multiply where the embed has the
     parity logic and the payload window.  The ratio is reported, not asserted.
  2. the calls that existed, this build against the baseline library (the parent commit's): the exact embed at n_ac = 20 and 63
     with delta = 20 and delta = 7.3, the dithered embed at n_ac = 10 and the delta <= 0 round-trip route.  The delta = 7.3 rows
     run the instantiation that now also holds the channel body; the others only take one more kernel argument.  The yardstick
     is the baseline's own run-to-run spread in the same process (ratelib.verdict).
Output: profiles/requantise_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc baseline REV=<parent commit> NAME=pre_requantise
    python tools/requantise_rates.py --reps 15 \\
        --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_requantise.so
"""
import ctypes as C
import statistics

import numpy as np

import ratelib
from ratelib import KEY, X, native
from svsdct import channel

DELTA = 20.0
TABLES = (("quality 50", 50), ("quality 75", 75), ("quality 90", 90), ("all ones", np.ones(64, np.uint16)))


def main():
    args = ratelib.parser("requantise_rates.txt", reps=15, baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline(ratelib.variant_path("pre_requantise"))
    s.noise()

    def requantise(steps, dst):
        return lambda: native.check(lib.svs_requantise_dev(s.gray, dst, s.P, C.byref(steps), 0, None), "svs_requantise_dev")

    s.say(f"requantisation channel, {s.f} x {s.w}x{s.h} gray, noise in [16, 240), {args.reps} alternated repetitions "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.say("1. svs_requantise_dev against svs_embed_dev(SVS_EXACT_POCKETFFT), n_ac = 63, delta = 20, of the same build")
    todo = {"embed n 63": s.embed(lib, DELTA, 63, X)}
    structs = [channel.steps_struct(t) for _, t in TABLES]
    for (name, _), steps in zip(TABLES, structs):
        todo[f"channel, {name}"] = requantise(steps, s.stego)
    t = s.measure(todo)
    s.report_rows(t)
    for k in list(t)[1:]:
        s.say(f"    {k}: ratio to the embed {statistics.median(t[k]) / statistics.median(t['embed n 63']):.3f}")
    # in place last: it overwrites the cover, which from here on is requantised noise (the same traffic and arithmetic)
    t = s.measure({"embed n 63": s.embed(lib, DELTA, 63, X), "channel, quality 75, in place": requantise(structs[1], s.gray)})
    s.report_rows(t)
    s.say(f"    in place: ratio to the embed {statistics.median(t['channel, quality 75, in place']) / statistics.median(t['embed n 63']):.3f}")

    if base is not None:
        s.say("2. the calls that existed: this build against the baseline (the parent commit's library)")
        s.noise()
        cases = [(f"exact embed n {n}, delta {d:g}", lambda so, d=d, n=n: s.embed(so, d, n, X)) for d in (20.0, 7.3) for n in (20, 63)]
        cases.append(("dithered embed n 10, delta 20", lambda so: s.embed_dithered(so, KEY, DELTA, 10, X)))
        cases.append(("round trip (delta 0), n 10", lambda so: s.embed(so, 0.0, 10, X)))
        s.against_baseline((what, make(base), make(lib)) for what, make in cases)
    else:
        s.say("2. no baseline library: the calls that existed were not compared")
    s.close()


if __name__ == "__main__":
    main()
