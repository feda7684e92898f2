"""Cost of the soft-margin pass (svs_stepped_embed_readback_margin_dev) and what its presence costs the calls that launch the
read-back instantiation which hosts it, readback_kernel<8, QM_POW2, true, BlockOrderArgs>.  Full-capacity payload; everything
alternated in the same rounds of one process, each call timed with a pair of HIP events on the null stream:
  (i)   stepped_embed_readback / stepped_embed_readback_margin at g = --gate (64): a uniform table of 20 with the zig-zag
        selection of 10 and a keyed dither, on noise and on letterboxed noise; pass 2 = the difference; the four counts of one
        call; and the call at g = 0, which must cost what the read-back call costs
  (ii)  the calls that launch the hosting instantiation, this build against --baseline-lib (the parent commit's library: `make -C
        csrc pre_readback_margin`), each judged against the parent's own spread (ratelib.verdict): svs_embed_readback_dev with an
        order at delta = 16, n = 63; svs_embed_bgr_readback_dev plain and keep-colour; svs_embed_dithered_readback_dev;
        svs_stepped_embed_readback_dev; and, so that every body of the pass is covered, the gray pass in raster order in a two-row
        instantiation (delta = 20, n = 10) and an eight-row one at 128 VGPRs (delta = 7.5, n = 20), and
        svs_stepped_embed_readback_margin_dev at g = --gate where the baseline has it
Output: profiles/readback_margin_rates.txt (--out).

    python tools/readback_margin_rates.py [--frames 200 --h 2160 --w 3840 --reps 15 --gate 64 --baseline-lib PATH]
"""
import ctypes as C
import os
import statistics

import ratelib
from ratelib import G, KEY, batch, coeffs, native


def main():
    ap = ratelib.parser("readback_margin_rates.txt", reps=15, baseline="optional")
    ap.add_argument("--n-ac", type=int, default=10)
    ap.add_argument("--gate", type=int, default=64)
    args = ap.parse_args()
    s = ratelib.Session(args)
    s.bgr_buffers(s.f)
    default = ratelib.variant_path("pre_readback_margin")
    lib, old, n_ac, delta, gate = s.lib, s.baseline(default), args.n_ac, 20.0, args.gate
    sel = coeffs.native_coeffs(coeffs.scan("zigzag", 1, n_ac))
    dith = native.Dither(KEY, 0, 0)
    order = batch.block_order(KEY, 0)
    from svsdct import steps as _steps
    table = _steps.steps_struct(_steps.uniform(20))
    cap, blocks = s.capacity(n_ac), s.f * (s.h // 8) * (s.w // 8)
    four = s.dev(32)          # svs_margin_counts: the session's small buffer holds two counts only

    def stepped_readback(so):
        return lambda: native.check(so.svs_stepped_embed_readback_dev(
            s.gray, s.stego, s.P, None, C.byref(sel), C.byref(dith), C.byref(table), n_ac, s.bits, 0, cap, G, C.byref(s.done),
            s.small, None), "svs_stepped_embed_readback_dev")

    def margin(g, so=lib):
        return lambda: native.check(so.svs_stepped_embed_readback_margin_dev(
            s.gray, s.stego, s.P, None, C.byref(sel), C.byref(dith), C.byref(table), n_ac, s.bits, 0, cap, g, G, C.byref(s.done),
            four, None), "svs_stepped_embed_readback_margin_dev")

    def four_counts(fn):
        native.check(lib.svs_memset(four, 0, 32, None), "memset")
        fn()
        out = (C.c_uint64 * 4)()
        native.check(lib.svs_memcpy_d2h(out, four, 32, None), "d2h")
        ratelib.sync()
        return tuple(int(c) for c in out)

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

    s.say(f"soft-margin pass cost, {s.f} x {s.w}x{s.h}, uniform table 20 / delta 20, n {n_ac} (zig-zag selection), keyed dither, "
          f"gate {gate}, guarded flags, full-capacity payload, {args.reps} alternated repetitions ({s.order_text()}), HIP events; ms "
          f"per call: median (min .. max)")
    if old is None:
        s.say(f"(no baseline library at {os.path.relpath(default, ratelib.ROOT)}: comparison (ii) not measured)")
    for kind in ("noise", "letterbox"):
        s.content(kind, bgr=True)
        s.say(f"{kind}")
        todo = {"stepped_embed_readback": stepped_readback(lib), "stepped_embed_readback_margin, g = 0": margin(0),
                f"stepped_embed_readback_margin, g = {gate}": margin(gate)}
        t = s.measure(todo)
        s.report_rows(t, width=44)
        m = {k: statistics.median(v) for k, v in t.items()}
        with_gate, alone = m[f"stepped_embed_readback_margin, g = {gate}"], m["stepped_embed_readback"]
        s.say(f"    (i) pass 2 {with_gate - alone:.3f} ms ({with_gate / alone:.2f} x svs_stepped_embed_readback_dev); counts "
              f"(repaired, unrepaired, strengthened, weak) {four_counts(margin(gate))} of {blocks} blocks; at g = 0 "
              f"{four_counts(margin(0))}, {m['stepped_embed_readback_margin, g = 0'] / alone:.3f} x")
        if old is not None:
            s.say("  (ii) the calls that launch the hosting instantiation, against the parent commit's library")
            cases = [
                ("embed_readback, keyed order, delta 16, n 63", ordered_readback(old), ordered_readback(lib)),
                ("embed_bgr_readback, plain", bgr_readback(old, False), bgr_readback(lib, False)),
                ("embed_bgr_readback, keep-colour", bgr_readback(old, True), bgr_readback(lib, True)),
                ("embed_dithered_readback, zig-zag 10, dither", keyed_readback(old), keyed_readback(lib)),
                ("stepped_embed_readback, zig-zag 10, dither, uniform 20", stepped_readback(old), stepped_readback(lib)),
                ("embed_readback, raster, delta 20, n 10", s.embed_readback(old, 20.0, 10, G), s.embed_readback(lib, 20.0, 10, G)),
                ("embed_readback, raster, delta 7.5, n 20", s.embed_readback(old, 7.5, 20, G), s.embed_readback(lib, 7.5, 20, G)),
            ]
            if hasattr(old, "svs_stepped_embed_readback_margin_dev"):      # a baseline from before the margin pass has none
                cases.append((f"stepped_embed_readback_margin, g = {gate}", margin(gate, old), margin(gate, lib)))
            s.against_baseline(cases)
    s.close()


if __name__ == "__main__":
    main()
