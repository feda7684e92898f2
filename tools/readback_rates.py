"""Cost of SVS_READBACK: svs_embed_readback_dev (embed, then the read-back pass over the stego) against svs_embed_dev, the same
call without the flag, on noise and on letterboxed frames (noise with black bars over a third of the rows), full-capacity
payload, guarded mode.  The two calls alternate in the same rounds; each call is timed with a pair of HIP events on the null
stream.  Output: profiles/readback_rates.txt.

    python tools/readback_rates.py [--frames 600 --h 2160 --w 3840 --rounds 10]
"""
import statistics

import ratelib
from ratelib import G


def main():
    ap = ratelib.parser("readback_rates.txt", frames=600, reps=10, rounds=True)
    ap.add_argument("--configs", default="8:3,20:10", help="delta:n_ac,...")
    args = ap.parse_args()
    s = ratelib.Session(args)
    blocks = s.f * (s.h // 8) * (s.w // 8)
    s.say(f"SVS_READBACK cost, {s.f} x {s.w}x{s.h}, guarded, full-capacity payload, {args.reps} alternated rounds "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")
    for delta, n_ac in ratelib.configs(args.configs):
        for kind in ("noise", "letterbox"):
            s.content(kind)
            todo = {"embed": s.embed(s.lib, delta, n_ac, G), "embed+readback": s.embed_readback(s.lib, delta, n_ac, G)}
            t = s.measure(todo)
            s.say(f"delta {delta:g} n {n_ac:2d} {kind}")
            s.report_rows(t)
            a, b = statistics.median(t["embed"]), statistics.median(t["embed+readback"])
            repaired, unrepaired = s.counts_of(todo["embed+readback"])
            s.say(f"    read-back pass {b - a:8.3f} ms   x{b / a:.2f}   per call: repaired {repaired} unrepaired {unrepaired} "
                  f"of {blocks} blocks")
    s.close()


if __name__ == "__main__":
    main()
