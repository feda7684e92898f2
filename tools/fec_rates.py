"""Cost of the Viterbi decoder (include/svsfec.h svs_fec_decode_soft_dev / svs_fec_decode_weights_dev) beside the call that
produces its input, gray frames of synthetic noise in [16, 240) carrying a full-capacity payload, n_ac = 10, delta = 20.  One
process; each call is timed with a pair of HIP events on the null stream, the calls alternated inside every repetition and the
order rotated from one repetition to the next.
  svs_soft_extract_dev                 one byte per capacity bit: the decoder's input
  svs_fec_decode_soft_dev, rate 2, 3   over the full capacity: n_info = svs_fec_info_bits(capacity, rate)
  svs_fec_decode_weights_dev, rate 2   over a tally of the same length (svs_soft_vote_dev at period = n_coded)
The payload is random bits, not a codeword: the decoder's work does not depend on its data (no branch of the kernel does), so
the times are those of a real stream; what it decodes is tested elsewhere (tests/test_fec_gpu.py).  No ratio is asserted: the
file reports the decode time beside the extract's, and the decoded payload bits per second.
Output: profiles/fec_rates.txt.

    python tools/fec_rates.py
"""
import statistics

import ratelib
from ratelib import X, native

from svsdct import fec

DELTA, N = 20.0, 10


def main():
    args = ratelib.parser("fec_rates.txt", reps=15).parse_args()
    s = ratelib.Session(args)
    lib, flib = s.lib, fec.load()
    cap = s.capacity(N)
    info = {r: int(flib.svs_fec_info_bits(cap, r)) for r in fec.RATES}
    coded = {r: fec.coded_bits(info[r], r) for r in fec.RATES}
    d_soft, d_tally, d_out = s.dev(s.cap_max + 8), s.dev(4 * cap + 8), s.dev((max(info.values()) + 7) // 8 + 8)
    out_bytes = (max(info.values()) + 7) // 8
    s.noise()
    s.say(f"Viterbi decoder, {s.f} x {s.w}x{s.h} gray noise in [16, 240), full-capacity payload, n_ac = {N}, delta = {DELTA:g}: "
          f"{cap} soft bytes; {args.reps} alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.embed(lib, DELTA, N, X)()
    s.soft(lib, DELTA, N, d_soft)()                        # the soft bytes the decoder reads
    native.check(lib.svs_memset(d_tally, 0, 4 * cap, None), "memset")
    s.vote(lib, DELTA, N, coded[2], d_tally)()             # a tally of n_coded entries: one copy's votes
    ratelib.sync()

    def soft_decode(rate):
        return lambda: fec.check(flib.svs_fec_decode_soft_dev(d_soft, info[rate], rate, d_out, out_bytes, None), "svs_fec_decode_soft_dev")

    todo = {"svs_soft_extract_dev": s.soft(lib, DELTA, N, d_soft),
            "svs_fec_decode_soft_dev, rate 2": soft_decode(2),
            "svs_fec_decode_soft_dev, rate 3": soft_decode(3),
            "svs_fec_decode_weights_dev, rate 2": lambda: fec.check(
                flib.svs_fec_decode_weights_dev(d_tally, info[2], 2, d_out, out_bytes, None), "svs_fec_decode_weights_dev")}
    t = s.measure(todo)
    extract = statistics.median(t["svs_soft_extract_dev"])
    for k, v in t.items():
        s.say(ratelib.row(k, v, 36) + f"  spread {ratelib.spread(v):.1f} %")
    for k, rate in (("svs_fec_decode_soft_dev, rate 2", 2), ("svs_fec_decode_soft_dev, rate 3", 3), ("svs_fec_decode_weights_dev, rate 2", 2)):
        m = statistics.median(t[k])
        s.say(f"    {k}: {info[rate]} payload bits, {info[rate] / m / 1e6:.2f} Gbit/s of payload, {m / extract:.2f} x the soft extract")
    s.close()


if __name__ == "__main__":
    main()
