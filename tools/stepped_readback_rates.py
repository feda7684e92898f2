"""Cost of the stepped read-back pass (svs_stepped_embed_readback_dev) and what its presence costs the calls that launch the
read-back instantiation which hosts it, readback_kernel<8, QM_POW2, true, BlockOrderArgs>.  Full-capacity payload; everything
alternated in the same rounds of one process, each call timed with a pair of HIP events on the null stream:
  (i)   stepped_embed / stepped_embed_readback       a uniform table of 20 with the zig-zag selection of 10 and a keyed dither,
                                                     on noise and on letterboxed noise; pass = the difference; the counts of one call
  (ii)  stepped_embed_readback / embed_dithered_readback   the same call against the keyed read-back at delta = 20: the extra is
                                                     the per-coefficient division (profiles/stepped_rates.txt)
  (iii) the calls that launch the hosting instantiation, this build against --baseline-lib (the parent commit's library: `make -C
        csrc pre_stepped_readback`), each judged against the parent's own spread (ratelib.verdict): svs_embed_readback_dev with an
        order at delta = 16, n = 63; svs_embed_bgr_readback_dev plain and keep-colour; svs_embed_dithered_readback_dev
Output: profiles/stepped_readback_rates.txt (--out).

    python tools/stepped_readback_rates.py [--frames 200 --h 2160 --w 3840 --reps 15 --baseline-lib PATH]
"""
import ctypes as C
import os
import statistics

import ratelib
from ratelib import G, KEY, batch, coeffs, native


def main():
    ap = ratelib.parser("stepped_readback_rates.txt", reps=15, baseline="optional")
    ap.add_argument("--n-ac", type=int, default=10)
    args = ap.parse_args()
    s = ratelib.Session(args)
    s.bgr_buffers(s.f)
    default = ratelib.variant_path("pre_stepped_readback")
    lib, old, n_ac, delta = s.lib, s.baseline(default), args.n_ac, 20.0
    sel = coeffs.native_coeffs(coeffs.scan("zigzag", 1, n_ac))
    dith = native.Dither(KEY, 0, 0)
    order = batch.block_order(KEY, 0)
    from svsdct import steps as _steps
    table = _steps.steps_struct(_steps.uniform(20))
    cap, blocks = s.capacity(n_ac), s.f * (s.h // 8) * (s.w // 8)

    def stepped(readback):
        if readback:
            return lambda: native.check(lib.svs_stepped_embed_readback_dev(
                s.gray, s.stego, s.P, None, C.byref(sel), C.byref(dith), C.byref(table), n_ac, s.bits, 0, cap, G, C.byref(s.done),
                s.small, None), "svs_stepped_embed_readback_dev")
        return lambda: native.check(lib.svs_stepped_embed_dev(
            s.gray, s.stego, s.P, None, C.byref(sel), C.byref(dith), C.byref(table), n_ac, s.bits, 0, cap, G, C.byref(s.done), None),
            "svs_stepped_embed_dev")

    def keyed_readback(so):
        return lambda: native.check(so.svs_embed_dithered_readback_dev(
            s.gray, s.stego, s.P, None, C.byref(sel), C.byref(dith), delta, n_ac, s.bits, 0, cap, G, C.byref(s.done), s.small, None),
            "svs_embed_dithered_readback_dev")

    def ordered_readback(so):
        c63 = s.capacity(63)
        return lambda: native.check(so.svs_embed_readback_dev(s.gray, s.stego, s.P, C.byref(order), 16.0, 63, s.bits, 0, c63, G,
                                                              C.byref(s.done), s.small, None), "svs_embed_readback_dev")

    def bgr_readback(so, keep):
        return s.embed_bgr_readback(so, delta, n_ac, G | (native.SVS_KEEP_COLOUR if keep else 0))

    s.say(f"stepped read-back cost, {s.f} x {s.w}x{s.h}, uniform table 20 / delta 20, n {n_ac} (zig-zag selection), keyed dither, "
          f"guarded flags, full-capacity payload, {args.reps} alternated repetitions ({s.order_text()}), HIP events; ms per call: "
          f"median (min .. max)")
    if old is None:
        s.say(f"(no baseline library at {os.path.relpath(default, ratelib.ROOT)}: comparison (iii) not measured)")
    for kind in ("noise", "letterbox"):
        s.content(kind, bgr=True)
        s.say(f"{kind}")
        todo = {"stepped_embed": stepped(False), "stepped_embed_readback": stepped(True),
                "embed_dithered_readback": keyed_readback(lib)}
        t = s.measure(todo)
        s.report_rows(t, width=38)
        m = {k: statistics.median(v) for k, v in t.items()}
        c1 = s.counts_of(todo["stepped_embed_readback"])
        c2 = s.counts_of(todo["embed_dithered_readback"])
        s.say(f"    (i) the pass {m['stepped_embed_readback'] - m['stepped_embed']:.3f} ms "
              f"({m['stepped_embed_readback'] / m['stepped_embed']:.2f} x svs_stepped_embed_dev); counts (repaired, unrepaired) {c1} of "
              f"{blocks} blocks")
        s.say(f"    (ii) against the keyed read-back at delta 20: {m['stepped_embed_readback'] / m['embed_dithered_readback']:.2f} x "
              f"({m['stepped_embed_readback'] - m['embed_dithered_readback']:+.3f} ms); its counts {c2}")
        if old is not None:
            s.say("  (iii) the calls that launch the hosting instantiation, against the parent commit's library")
            s.against_baseline([
                ("embed_readback, keyed order, delta 16, n 63", ordered_readback(old), ordered_readback(lib)),
                ("embed_bgr_readback, plain", bgr_readback(old, False), bgr_readback(lib, False)),
                ("embed_bgr_readback, keep-colour", bgr_readback(old, True), bgr_readback(lib, True)),
                ("embed_dithered_readback, zig-zag 10, dither", keyed_readback(old), keyed_readback(lib)),
            ])
    s.close()


if __name__ == "__main__":
    main()
