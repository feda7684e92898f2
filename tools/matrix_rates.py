"""Cost of matrix embedding (svs_matrix_embed_dev / svs_matrix_extract_dev) and what its presence costs the calls that run in the
four instantiations which hold it: embed_exact_kernel<QM_DOUBLE, 8> and extract_exact_kernel<8, QM_POW2>, with and without an
order.  Noise in [16, 240), full-capacity payload; everything alternated in the same rounds of one process, each call timed with a
pair of HIP events on the null stream:
  (i)   svs_matrix_embed_dev at k = 3 and 4, both searches, under SVS_MINMOVE with a uniform table of 20 on the zig-zag selection
        of 2^k - 1, against svs_stepped_embed_dev with the same selection, table and rule in the same build; svs_matrix_extract_dev
        against svs_stepped_extract_dev likewise; the round trip's bit errors and the PSNR of frame 0
  (ii)  the calls that run in the four holders, this build against --baseline-lib (the parent commit's library: `make -C csrc
        baseline REV=<parent> NAME=pre_matrix`), each judged against the parent's own spread (ratelib.verdict): the stepped embed and
        extract, the delta = 7.3 exact embed at n = 20 and 63, the channel, and the soft extract, vote and histogram under steps
Output: profiles/matrix_rates.txt (--out).

    python tools/matrix_rates.py [--frames 200 --h 2160 --w 3840 --reps 15 --baseline-lib PATH]
"""
import ctypes as C
import os
import statistics

import ratelib
from ratelib import X, coeffs, native


def main():
    ap = ratelib.parser("matrix_rates.txt", reps=15, baseline="optional")
    args = ap.parse_args()
    s = ratelib.Session(args)
    default = ratelib.variant_path("pre_matrix")
    lib, old = s.lib, s.baseline(default)
    from svsdct import channel as _channel
    from svsdct import matrix as _matrix
    from svsdct import steps as _steps
    table = _steps.steps_struct(_steps.uniform(20))
    minmove = X | native.SVS_MINMOVE

    def selection(n):
        return coeffs.native_coeffs(coeffs.scan("zigzag", 1, n))

    def stepped_embed(so, sel, flags):
        cap = s.capacity(sel.count)
        return lambda: native.check(so.svs_stepped_embed_dev(s.gray, s.stego, s.P, None, C.byref(sel), None, C.byref(table), sel.count,
                                                             s.bits, 0, cap, flags, C.byref(s.done), None), "svs_stepped_embed_dev")

    def stepped_extract(so, sel):
        return lambda: native.check(so.svs_stepped_extract_dev(s.stego, s.P, None, C.byref(sel), None, C.byref(table), sel.count, s.ext,
                                                               s.packed_bytes, X, C.byref(s.done), None), "svs_stepped_extract_dev")

    def matrix_embed(sel, m, flags):
        cap = _matrix.capacity_bits(s.f, s.h, s.w, m.k)
        return lambda: native.check(lib.svs_matrix_embed_dev(s.gray, s.stego, s.P, None, C.byref(sel), None, C.byref(table), C.byref(m),
                                                             sel.count, s.bits, 0, cap, flags, C.byref(s.done), None),
                                    "svs_matrix_embed_dev")

    def matrix_extract(sel, m):
        return lambda: native.check(lib.svs_matrix_extract_dev(s.stego, s.P, None, C.byref(sel), None, C.byref(table), C.byref(m),
                                                               sel.count, s.ext, s.packed_bytes, X, C.byref(s.done), None),
                                    "svs_matrix_extract_dev")

    s.say(f"matrix embedding, {s.f} x {s.w}x{s.h}, noise in [16, 240), uniform table 20, zig-zag selections, full-capacity payload, "
          f"{args.reps} alternated repetitions ({s.order_text()}), HIP events; ms per call: median (min .. max)")
    s.noise()
    s.say("(i) the new calls against the stepped calls with the same 2^k - 1 selection, SVS_MINMOVE")
    for k in (3, 4):
        sel = selection(_matrix.slots(k))
        single, pair = _matrix.matrix_struct(k, 0), _matrix.matrix_struct(k, 1)
        s.say(f"  k = {k}, n = {sel.count}")
        t = s.measure({"stepped_embed": stepped_embed(lib, sel, minmove), "matrix_embed, single": matrix_embed(sel, single, minmove),
                       "matrix_embed, pair": matrix_embed(sel, pair, minmove)})
        s.report_rows(t)
        m = {name: statistics.median(v) for name, v in t.items()}
        s.say(f"    matrix / stepped: single {m['matrix_embed, single'] / m['stepped_embed']:.2f}, pair "
              f"{m['matrix_embed, pair'] / m['stepped_embed']:.2f}")
        for name, call in (("single", matrix_embed(sel, single, minmove)), ("pair", matrix_embed(sel, pair, minmove))):
            call()
            psnr = s.psnr_frame0()
            matrix_extract(sel, single)()
            errors = s.bit_errors(_matrix.capacity_bits(s.f, s.h, s.w, k))
            s.say(f"    {name}: PSNR of frame 0 {psnr:.2f} dB, bit errors of the round trip {errors}")
        stepped_embed(lib, sel, minmove)()
        t = s.measure({"stepped_extract": stepped_extract(lib, sel), "matrix_extract": matrix_extract(sel, single)})
        s.report_rows(t)
        s.say(f"    matrix / stepped: {statistics.median(t['matrix_extract']) / statistics.median(t['stepped_extract']):.2f}")

    if old is None:
        s.say(f"(no baseline library at {os.path.relpath(default, ratelib.ROOT)}: comparison (ii) not measured)")
        s.close()
        return
    s.say("(ii) the calls that run in the four holders, against the parent commit's library")
    sel10 = selection(10)
    codec = _channel.steps_struct(75)
    soft = s.dev(s.capacity(10))
    period = 4096
    tally, hist = s.dev(4 * period), s.dev(4 * 256 * s.f)
    native.check(lib.svs_memset(tally, 0, 4 * period, None), "memset")
    native.check(lib.svs_memset(hist, 0, 4 * 256 * s.f, None), "memset")
    order = ratelib.batch.block_order(ratelib.KEY, 0)

    def stepped_embed_keyed(so):
        cap = s.capacity(10)
        return lambda: native.check(so.svs_stepped_embed_dev(s.gray, s.stego, s.P, C.byref(order), C.byref(sel10), None, C.byref(table), 10,
                                                             s.bits, 0, cap, X, C.byref(s.done), None), "svs_stepped_embed_dev")

    def stepped_extract_keyed(so):
        return lambda: native.check(so.svs_stepped_extract_dev(s.stego, s.P, C.byref(order), C.byref(sel10), None, C.byref(table), 10, s.ext,
                                                               s.packed_bytes, X, C.byref(s.done), None), "svs_stepped_extract_dev")

    def channel(so):
        return lambda: native.check(so.svs_requantise_dev(s.stego, s.stego, s.P, C.byref(codec), 0, None), "svs_requantise_dev")

    def soft_extract(so):
        return lambda: native.check(so.svs_stepped_soft_extract_dev(s.stego, s.P, None, C.byref(sel10), None, C.byref(table), 10, soft,
                                                                    s.capacity(10), X, C.byref(s.done), None), "svs_stepped_soft_extract_dev")

    def soft_vote(so):
        return lambda: native.check(so.svs_stepped_soft_vote_dev(s.stego, s.P, None, C.byref(sel10), None, C.byref(table), 10, period, 0,
                                                                 tally, X, C.byref(s.done), None), "svs_stepped_soft_vote_dev")

    def soft_histogram(so):
        return lambda: native.check(so.svs_stepped_soft_histogram_dev(s.stego, s.P, C.byref(sel10), None, C.byref(table), 10, hist, X,
                                                                      C.byref(s.done), None), "svs_stepped_soft_histogram_dev")

    s.against_baseline([
        ("stepped_embed, zig-zag 10, uniform 20", stepped_embed(old, sel10, X), stepped_embed(lib, sel10, X)),
        ("stepped_embed, zig-zag 10, uniform 20, keyed order", stepped_embed_keyed(old), stepped_embed_keyed(lib)),
        ("embed, delta 7.3, n 20, exact", s.embed(old, 7.3, 20, X), s.embed(lib, 7.3, 20, X)),
        ("embed, delta 7.3, n 63, exact", s.embed(old, 7.3, 63, X), s.embed(lib, 7.3, 63, X)),
        ("stepped_extract, zig-zag 10, uniform 20", stepped_extract(old, sel10), stepped_extract(lib, sel10)),
        ("stepped_extract, zig-zag 10, uniform 20, keyed order", stepped_extract_keyed(old), stepped_extract_keyed(lib)),
        ("stepped_soft_extract, zig-zag 10", soft_extract(old), soft_extract(lib)),
        ("stepped_soft_vote, zig-zag 10, period 4096", soft_vote(old), soft_vote(lib)),
        ("stepped_soft_histogram, zig-zag 10", soft_histogram(old), soft_histogram(lib)),
        ("requantise, quality 75 (in place)", channel(old), channel(lib)),
    ])
    s.close()


if __name__ == "__main__":
    main()
