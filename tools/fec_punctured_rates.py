"""Cost of the Viterbi decoder under the punctured codes (include/svsfec.h "Punctured codes": rate 23, 34, 56, 78) beside the
rate-2 call of the same build, gray frames of synthetic noise in [16, 240) carrying a full-capacity payload, n_ac = 10,
delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the calls alternated inside every
repetition and the order rotated from one repetition to the next.
  svs_fec_decode_soft_dev, rate 2, 3         over the full capacity: n_info = svs_fec_info_bits(capacity, rate)
  svs_fec_decode_soft_dev, code 23 .. 78     the same soft bytes read as a punctured stream of full-capacity n_info
  svs_fec_decode_weights_dev, rate 2, code 34   over a tally of the same length
A punctured call runs the rate-2 decoder's add-compare-select and traceback over more steps (the capacity holds more of them)
and reads fewer bytes a step, so the figure to compare is ms per 10^6 trellis steps; no ratio is asserted.  The payload is
random bits, not a codeword: no branch of the kernel depends on its data.
With --baseline-lib (libsvsfec.so of the parent commit: `make -C <package>/csrc fec-baseline REV=<commit>`), the calls that
existed before - rate 2, rate 3, weights at rate 2 - are timed against that library's, each pair alternated and judged by the
baseline's own spread (ratelib.verdict).
Output: profiles/fec_punctured_rates.txt.

    python tools/fec_punctured_rates.py [--baseline-lib <package>/lib/variants/libsvsfec_parent.so]
"""
import ctypes as C
import os
import statistics

import ratelib
from ratelib import X, native

from svsdct import fec

DELTA, N = 20.0, 10


def load_fec_build(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in fec.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def main():
    args = ratelib.parser("fec_punctured_rates.txt", reps=15, baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, flib = s.lib, fec.load()
    cap = s.capacity(N)
    codes = fec.RATES + fec.PUNCTURED
    info = {r: int(flib.svs_fec_info_bits(cap, r)) for r in codes}
    assert all(0 < flib.svs_fec_coded_bits(info[r], r) <= cap for r in codes)
    out_bytes = (max(info.values()) + 7) // 8
    d_soft, d_tally, d_out = s.dev(s.cap_max + 8), s.dev(4 * cap + 8), s.dev(out_bytes + 8)
    s.noise()
    s.say(f"Viterbi decoder under punctured codes, {s.f} x {s.w}x{s.h} gray noise in [16, 240), full-capacity payload, n_ac = {N}, "
          f"delta = {DELTA:g}: {cap} capacity bits; {args.reps} alternated repetitions ({s.order_text()}), HIP events; "
          f"ms per call: median (min .. max)")
    s.embed(lib, DELTA, N, X)()
    s.soft(lib, DELTA, N, d_soft)()                        # the soft bytes the decoder reads
    native.check(lib.svs_memset(d_tally, 0, 4 * cap, None), "memset")
    s.vote(lib, DELTA, N, int(flib.svs_fec_coded_bits(info[2], 2)), d_tally)()     # a tally: one copy's votes
    ratelib.sync()

    def soft_decode(rate, build=flib):
        return lambda: fec.check(build.svs_fec_decode_soft_dev(d_soft, info[rate], rate, d_out, out_bytes, None), "svs_fec_decode_soft_dev")

    def weights_decode(rate, build=flib):
        return lambda: fec.check(build.svs_fec_decode_weights_dev(d_tally, info[rate], rate, d_out, out_bytes, None),
                                 "svs_fec_decode_weights_dev")

    todo = {f"svs_fec_decode_soft_dev, {'rate' if r in fec.RATES else 'code'} {r}": soft_decode(r) for r in codes}
    todo["svs_fec_decode_weights_dev, rate 2"] = weights_decode(2)
    todo["svs_fec_decode_weights_dev, code 34"] = weights_decode(34)
    rate_of = dict(zip(todo, codes + (2, 34)))
    t = s.measure(todo)
    for k, v in t.items():
        s.say(ratelib.row(k, v, 38) + f"  spread {ratelib.spread(v):.1f} %")
    s.say("  per trellis step (n_info + 6 steps a call): ms per 10^6 steps, median (min .. max); payload bits; sent values read")
    per_step = {}
    for k, v in t.items():
        r = rate_of[k]
        steps = (info[r] + fec.TAIL) / 1e6
        per_step[k] = [x / steps for x in v]
        s.say(f"    {k:38s} {statistics.median(per_step[k]):.5f}  ({min(per_step[k]):.5f} .. {max(per_step[k]):.5f})  {info[r]} payload bits, "
              f"{int(flib.svs_fec_coded_bits(info[r], r))} values, {info[r] / statistics.median(v) / 1e6:.2f} Gbit/s of payload")
    for ref, prefix in (("svs_fec_decode_soft_dev, rate 2", "svs_fec_decode_soft_dev, code"),
                        ("svs_fec_decode_weights_dev, rate 2", "svs_fec_decode_weights_dev, code")):
        lo, hi = min(per_step[ref]), max(per_step[ref])
        for k in per_step:
            if k.startswith(prefix):
                m = statistics.median(per_step[k])
                where = "inside" if lo <= m <= hi else "BELOW (cheaper than)" if m < lo else "ABOVE (dearer than)"
                s.say(f"    {k}: a step costs {m / statistics.median(per_step[ref]):.3f} x the rate-2 call's, {where} its spread")

    if not args.baseline_lib:
        s.say("  no --baseline-lib: the calls that existed before were not timed against the parent commit's library")
    else:
        old = load_fec_build(args.baseline_lib)
        s.say(f"  against {os.path.basename(args.baseline_lib)} (the parent commit's libsvsfec.so), each pair alternated")
        s.against_baseline([("svs_fec_decode_soft_dev, rate 2", soft_decode(2, old), soft_decode(2)),
                            ("svs_fec_decode_soft_dev, rate 3", soft_decode(3, old), soft_decode(3)),
                            ("svs_fec_decode_weights_dev, rate 2", weights_decode(2, old), weights_decode(2))])
    s.close()


if __name__ == "__main__":
    main()
