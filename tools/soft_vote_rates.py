"""Cost of the fused soft vote (include/svsdct.h svs_soft_vote_dev), gray frames of synthetic noise in [16, 240) carrying a
full-capacity payload, n_ac = 10, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the
sides of a comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. svs_soft_vote_dev at period = 2 400, 10^6 and capacity / 3 against svs_soft_extract_dev and
     svs_extract_dev(SVS_EXACT_POCKETFFT) at the same n_ac.  The vote writes no soft byte; what it adds instead is one global
     int32 atomic per byte, or per entry a wave touches.  At period = 2 400 every wave of the launch adds into the same 9.6 KB:
     the rate of the atomics there is the open number.  At 10^6 and capacity / 3 the adds spread over megabytes.
  2. the calls that existed - the hard eight-row calls (n = 63, a zig-zag selection, a dither) and the soft call -, this build
     against the baseline library (the parent commit's): the vote tail shares their four instantiations.  The yardstick is the
     baseline's own run-to-run spread in the same process: this build's median should lie inside its min-max.
No ratio is asserted: the file reports what is seen next to the spread of the same session.
Output: profiles/soft_vote_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_vote      # lib/variants/libsvsdct_pre_vote.so, from git
    python tools/soft_vote_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_vote.so
"""
import ctypes as C
import statistics

import ratelib
from ratelib import KEY, X, batch, native

DELTA, N = 20.0, 10


def main():
    args = ratelib.parser("soft_vote_rates.txt", baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline()
    periods = (2400, 10 ** 6, max(1, s.capacity(N) // 3))
    d_soft, d_tally = s.dev(s.cap_max + 8), s.dev(4 * max(periods))
    s.noise()
    s.say(f"fused soft vote, {s.f} x {s.w}x{s.h} gray noise in [16, 240), full-capacity payload, n_ac = {N}, delta = {DELTA:g}, "
          f"{args.reps} alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.say("1. svs_soft_vote_dev against svs_soft_extract_dev and svs_extract_dev(SVS_EXACT_POCKETFFT)")
    s.embed(lib, DELTA, N, X)()                        # the stego the extract calls read: a full payload at n_ac
    todo = {"hard": s.extract(lib, DELTA, N, X), "soft": s.soft(lib, DELTA, N, d_soft)}
    # At the default size a call adds at most 108 000 copies of 511 to an entry of the smallest period, 5.5e7: the 1 + reps calls
    # stay inside int32 up to 38 of them.
    for period in periods:
        todo[f"vote, period {period}"] = s.vote(lib, DELTA, N, period, d_tally)
    order = batch.block_order(KEY, 0)
    todo["vote under an order, period 2400"] = s.vote(lib, DELTA, N, 2400, d_tally, C.byref(order))
    native.check(lib.svs_memset(d_tally, 0, 4 * max(periods), None), "memset")
    t = s.measure(todo)
    for k, v in t.items():
        s.say(ratelib.row(k, v) + f"  spread {ratelib.spread(v):.1f} %")
    for k in list(t)[2:]:
        s.say(f"    {k}: ratio to soft {statistics.median(t[k]) / statistics.median(t['soft']):.3f}, to hard "
              f"{statistics.median(t[k]) / statistics.median(t['hard']):.3f}")

    if base is not None:
        s.say("2. the calls that existed: this build against the baseline (the parent commit's library)")
        s.embed(lib, DELTA, 63, X)()
        s.against_baseline((what, make(base), make(lib)) for what, make in s.eight_row_calls(DELTA, d_soft))
    s.close()


if __name__ == "__main__":
    main()
