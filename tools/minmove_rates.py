"""Cost and gain of SVS_MINMOVE (include/svsdct.h) on the gray embed, guarded mode, full-capacity payload, synthetic noise frames
(the benchmark's content).  One process; each call is timed with a pair of HIP events on the null stream (torch.cuda.Event; the
library's calls with stream NULL are enqueued on the same stream), the builds and the flags alternated inside every repetition
and the order of the calls rotated from one repetition to the next, so that no call always runs behind the same neighbour
(--fixed-order keeps one order):
  baseline, flag clear     --baseline-lib PATH: the library of the commit before the flag (it refuses the flag)
  baseline, SVS_NEAREST    the parent's nearest-rule time: what the time with the new flag set is compared with
  this build, flag clear   must stay inside the baseline's own min-max spread of the baseline's median
  this build, SVS_NEAREST  likewise against the baseline's nearest time
  this build, SVS_MINMOVE  reported beside them (no bar)
and, per setting, the PSNR of frame 0 against the cover under the three rules (svs_frame_sse_dev) and the payload bit errors of
the minimum-move stego through svs_extract_dev.  The fused colour embed (svs_embed_bgr_dev, --bgr-frames frames) is timed the
same way for the settings of --bgr-configs.  Output: profiles/minmove_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_minmove      # lib/variants/libsvsdct_pre_minmove.so, from git
    python tools/minmove_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_minmove.so
"""
import statistics

import ratelib
from ratelib import G, native

RULES = {"flag clear": 0, "SVS_NEAREST": native.SVS_NEAREST, "SVS_MINMOVE": native.SVS_MINMOVE}


def main():
    ap = ratelib.parser("minmove_rates.txt", baseline="optional")
    ap.add_argument("--configs", default="20:3,20:10,20:20", help="delta:n_ac,...")
    ap.add_argument("--bgr-frames", type=int, default=48)
    ap.add_argument("--bgr-configs", default="20:10", help="delta:n_ac,... of the fused colour embed")
    args = ap.parse_args()
    s = ratelib.Session(args)
    lib, base = s.lib, s.baseline()

    def section(embed, delta, n_ac):
        """medians with their ranges; against a baseline: each of this build's older sides against the baseline's spread, and
        the new flag's time against the baseline's SVS_NEAREST time"""
        todo = {"this build, " + rule: embed(lib, delta, n_ac, G | flag) for rule, flag in RULES.items()}
        if base is not None:
            todo = {"baseline,   flag clear": embed(base, delta, n_ac, G),
                    "baseline,   SVS_NEAREST": embed(base, delta, n_ac, G | native.SVS_NEAREST), **todo}
        t = s.measure(todo)
        s.say(f"delta {delta:g} n {n_ac}")
        s.report_rows(t, width=24)
        if base is not None:
            m = {k: statistics.median(v) for k, v in t.items()}
            for side in ("flag clear", "SVS_NEAREST"):
                b = t["baseline,   " + side]
                s.say(f"    {side}: this build - baseline = {m['this build, ' + side] - m['baseline,   ' + side]:+.3f} ms, "
                      f"baseline spread {max(b) - min(b):.3f} ms")
                s.say(ratelib.verdict(b, t["this build, " + side])[1])
            over = m["this build, SVS_MINMOVE"] - m["baseline,   SVS_NEAREST"]
            s.say(f"    SVS_MINMOVE: this build - baseline's SVS_NEAREST = {over:+.3f} ms "
                  f"({100 * over / m['baseline,   SVS_NEAREST']:+.1f} %)")
        return todo

    s.noise()
    s.say(f"SVS_MINMOVE cost and gain, {s.f} x {s.w}x{s.h} gray noise in [16, 240), guarded, full-capacity payload, {args.reps} "
          f"alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    for delta, n_ac in ratelib.configs(args.configs):
        todo = section(s.embed, delta, n_ac)
        psnr = []
        for rule in RULES:
            todo["this build, " + rule]()
            psnr.append(s.psnr_frame0())
        s.extract(lib, delta, n_ac, G)()
        cap = s.capacity(n_ac)
        s.say(f"    PSNR frame 0: reference {psnr[0]:.2f}, SVS_NEAREST {psnr[1]:.2f}, SVS_MINMOVE {psnr[2]:.2f} dB "
              f"({psnr[2] - psnr[0]:+.2f} / {psnr[2] - psnr[1]:+.2f}); payload bit errors with SVS_MINMOVE: {s.bit_errors(cap)} of {cap}")

    # ---- the fused colour embed (its kernel tests the rule once per block) ----
    fb = min(args.bgr_frames, s.f)
    s.bgr_buffers(fb)
    s.noise(bgr=True)
    s.say(f"fused colour embed, {fb} x {s.w}x{s.h} BGR")
    for delta, n_ac in ratelib.configs(args.bgr_configs):
        section(s.embed_bgr, delta, n_ac)
    s.close()


if __name__ == "__main__":
    main()
