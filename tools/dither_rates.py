"""Cost and effect of the keyed dither (include/svsdct.h svs_dither), gray frames of synthetic noise in [16, 240), full-capacity
payload, delta = 20.  One process; each call is timed with a pair of HIP events on the null stream, the two sides of a
comparison alternated inside every repetition and the order rotated from one repetition to the next.
  1. the dithered embed and extract against the SVS_EXACT_POCKETFFT call at the same n_ac (n = 3, 10, 63): ratio, and the
     run-to-run spread of each side; and the dithered selected call against the selected call (zig-zag, the same counts).
  2. calls WITHOUT a dither, this build against the baseline library (the parent commit's): embed at n = 3, 10 (guarded) and
     10, 63 (exact), extract at n = 3, 10, 63.  This build's median should lie inside the baseline's own min-max spread.
  3. the numbers of the header, from frame 0 of the batch: PSNR against the cover with and without a dither under the three
     rules, the share of recomputed payload coefficients within delta / 4 of a multiple of delta, and the payload bit errors
     over the batch with the right key, another key and no key.
Output: profiles/dither_rates.txt.

    make -C secure-video-steganography-using-ecc-and-dct_amd/csrc pre_dither      # lib/variants/libsvsdct_pre_dither.so, from git
    python tools/dither_rates.py --baseline-lib secure-video-steganography-using-ecc-and-dct_amd/lib/variants/libsvsdct_pre_dither.so
"""
import statistics

import numpy as np

import ratelib
from ratelib import G, KEY, X, coeffs, native

DELTA, OTHER_KEY = 20.0, 0x0123456789ABCDEE


def main():
    args = ratelib.parser("dither_rates.txt", baseline="optional").parse_args()
    s = ratelib.Session(args)
    lib, base, h, w = s.lib, s.baseline(), s.h, s.w
    s.noise()

    def compare(title, a_name, a, b_name, b):
        t = s.measure({a_name: a, b_name: b})
        s.report_rows(t, title + " ")
        r = statistics.median(t[b_name]) / statistics.median(t[a_name])
        s.say(f"    {title} ratio {b_name} / {a_name} = {r:.3f}  (spread {a_name} {ratelib.spread(t[a_name]):.1f} %, "
              f"{b_name} {ratelib.spread(t[b_name]):.1f} %)")

    s.say(f"keyed dither, {s.f} x {w}x{h} gray noise in [16, 240), full-capacity payload, delta = {DELTA:g}, {args.reps} alternated "
          f"repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.say("1. dithered calls against the SVS_EXACT_POCKETFFT call at the same n_ac")
    for n_ac in (3, 10, 63):
        compare(f"n {n_ac} embed", "exact", s.embed(lib, DELTA, n_ac, X), "dithered", s.embed_dithered(lib, KEY, DELTA, n_ac, G))
        compare(f"n {n_ac} extract", "exact", s.extract(lib, DELTA, n_ac, X), "dithered", s.extract_dithered(lib, KEY, DELTA, n_ac, G))
    s.say("1b. dithered selected calls against the selected call (zig-zag scan, the same counts)")
    for n_ac in (3, 10, 63):
        sel = coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))
        compare(f"zigzag {n_ac} embed", "selected", s.embed_select(lib, sel, DELTA, X),
                "dithered", s.embed_dithered(lib, KEY, DELTA, 0, X, sel))
        compare(f"zigzag {n_ac} extract", "selected", s.extract_select(lib, sel, DELTA, X),
                "dithered", s.extract_dithered(lib, KEY, DELTA, 0, X, sel))

    if base is not None:
        s.say("2. calls without a dither: this build against the baseline (the parent commit's library)")

        def undithered():
            for what, n_ac, flags in (("embed", 3, G), ("embed", 10, G), ("embed", 10, X), ("embed", 63, X), ("extract", 3, G),
                                      ("extract", 10, G), ("extract", 63, G)):
                make = s.embed if what == "embed" else s.extract
                s.embed(lib, 8, n_ac, flags)()                     # the stego the extract calls read
                title = f"{what} delta 8 n {n_ac} {'exact' if flags == X else 'guarded'}"
                yield title, make(base, 8, n_ac, flags), make(lib, 8, n_ac, flags)

        s.against_baseline(undithered())

    s.say("3. frame 0 of the batch, n = 10 (MI355X): PSNR against the cover, the share of recomputed payload coefficients within "
          "delta / 4 of a multiple of delta, payload bit errors over the batch")
    from scipy.fftpack import dct

    def comb(n_ac):
        """the share of frame 0's recomputed payload coefficients within delta / 4 of a multiple of delta"""
        stego = np.empty(h * w, np.uint8)
        native.check(lib.svs_memcpy_d2h(stego.ctypes.data, s.stego, stego.nbytes, None), "d2h")
        ratelib.sync()
        blk = np.float32(stego).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        c = dct(dct(blk, axis=2, norm="ortho"), axis=3, norm="ortho").reshape(-1, 64)[:, 1:n_ac + 1].reshape(-1)
        return float((np.abs(c - DELTA * np.rint(c / DELTA)) < DELTA / 4).mean())

    n_ac = 10
    cap = s.capacity(n_ac)
    for rule, flag in (("reference", 0), ("SVS_NEAREST", native.SVS_NEAREST), ("SVS_MINMOVE", native.SVS_MINMOVE)):
        res = []
        for name, call in (("no dither", s.embed(lib, DELTA, n_ac, X | flag)),
                           ("dither", s.embed_dithered(lib, KEY, DELTA, n_ac, X | flag))):
            call()
            res.append(f"{name}: PSNR {s.psnr_frame0():.2f} dB, comb share {comb(n_ac):.4f}")
        s.say(f"    {rule:12s} " + ";  ".join(res))
    s.embed_dithered(lib, KEY, DELTA, n_ac, G)()
    for name, call in (("right key", s.extract_dithered(lib, KEY, DELTA, n_ac, G)),
                       ("another key", s.extract_dithered(lib, OTHER_KEY, DELTA, n_ac, G)),
                       ("no dither (svs_extract_dev)", s.extract(lib, DELTA, n_ac, G))):
        call()
        e = s.bit_errors(cap)
        s.say(f"    dithered stego read with {name:28s} {e:12d} errors of {cap}  (rate {e / cap:.4f})")
    s.close()


if __name__ == "__main__":
    main()
