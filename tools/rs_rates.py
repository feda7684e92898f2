"""Cost of the Reed-Solomon decoder (include/svsrs.h svs_rs_decode_dev) beside the call in front of it, the Viterbi decoder
(svs_fec_decode_soft_dev at rate 2) on the same payload in the same process.  The workload is the RS stream that fills
svs_fec_info_bits of the frames' capacity at n_ac = 10, rate 1/2: k = svs_rs_data_bytes(info_bits / 8) random data bytes,
encoded on the host (svs_rs_encode), and four received streams made from it:
  clean                        as sent: every codeword leaves after the screening pass
  1 % dirty                    one codeword in a hundred with 1 .. 16 wrong bytes
  16 errors a codeword         every codeword repaired at the code's limit
  uncorrectable                40 wrong bytes in every codeword: every repair runs and fails
The decoder works in place, so before every timed call the received stream is copied back over the working buffer, outside the
pair of HIP events.  The calls are alternated inside every repetition and the order rotated from one repetition to the next.
Before the timing each case is decoded once into zeroed counters, which the report shows.  The Viterbi call reads soft bytes
of the same length extracted from noise frames: its work does not depend on its data (tools/fec_rates.py).  No ratio is
asserted: the file reports the four times, their ratios to the Viterbi call and the clean pass's bytes per second.
With --baseline-lib (libsvsrs.so of the parent commit: `make -C <package>/csrc rs-baseline REV=<commit>`), each of the four cases
is also timed against that library's svs_rs_decode_dev, each pair alternated and judged by the baseline's own spread
(ratelib.verdict).
Output: profiles/rs_rates.txt.

    python tools/rs_rates.py [--baseline-lib <package>/lib/variants/libsvsrs_parent.so]
"""
import ctypes as C
import os
import statistics

import numpy as np

import ratelib
from ratelib import X

from svsdct import fec, rs

DELTA, N = 20.0, 10
PLACES = 250                      # error positions are drawn among a codeword's first 250 bytes: every codeword has at least 254


def received(sent, k, rng, share, lo, hi):
    """`sent` with lo .. hi wrong bytes in a share of the codewords (1: every one)"""
    n_cw = rs.codewords(k)
    kc = -(-(k - np.arange(n_cw)) // n_cw)
    chosen = np.flatnonzero(rng.random(n_cw) < share) if share < 1 else np.arange(n_cw)
    count = rng.integers(lo, hi + 1, chosen.size)
    places = np.argsort(rng.random((chosen.size, PLACES)), axis=1)[:, :hi]             # distinct bytes of a codeword
    use = np.arange(hi)[None, :] < count[:, None]
    c = np.broadcast_to(chosen[:, None], places.shape)[use]
    i = places[use]
    at = np.where(i < kc[c], i * n_cw + c, k + (i - kc[c]) * n_cw + c)
    out = sent.copy()
    out[at] ^= rng.integers(1, 256, at.size).astype(np.uint8)
    return out


def load_rs_build(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in rs.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def main():
    args = ratelib.parser("rs_rates.txt", reps=15, baseline="optional").parse_args()
    s = ratelib.Session(args)
    torch = ratelib._torch
    lib, flib, rlib = s.lib, fec.load(), rs.load()
    cap = s.capacity(N)
    info_cap = int(flib.svs_fec_info_bits(cap, 2))
    k = int(rlib.svs_rs_data_bytes(info_cap // 8))
    n_cw, total = rs.codewords(k), rs.coded_bytes(k)
    n_info = 8 * total
    rng = np.random.default_rng(7)
    sent = rs.encode_array(rng.integers(0, 256, k).astype(np.uint8))
    cases = {"clean": sent,
             "1 % of codewords with 1 .. 16 errors": received(sent, k, rng, 0.01, 1, 16),
             "every codeword with 16 errors": received(sent, k, rng, 1, 16, 16),
             "every codeword uncorrectable (40 errors)": received(sent, k, rng, 1, 40, 40)}
    master = {name: torch.from_numpy(a).cuda() for name, a in cases.items()}
    work = torch.empty(total + 1, dtype=torch.uint8, device="cuda")[1:]                 # an odd address: any alignment
    status = torch.empty(n_cw, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_soft, d_out = s.dev(s.cap_max + 8), s.dev((info_cap + 7) // 8 + 8)
    s.noise()
    s.say(f"Reed-Solomon decoder, the stream that fills the rate-1/2 payload of {s.f} x {s.w}x{s.h} gray frames at n_ac = {N}: "
          f"k = {k} data bytes, {n_cw} codewords, {total} bytes; {args.reps} alternated repetitions ({s.order_text()}), HIP events; "
          f"ms per call: median (min .. max)")
    s.embed(lib, DELTA, N, X)()
    s.soft(lib, DELTA, N, d_soft)()                        # the soft bytes the Viterbi decoder reads
    ratelib.sync()

    def decode(name, d_counts=None, build=rlib):
        fn = lambda: rs.check(build.svs_rs_decode_dev(work.data_ptr(), k, status.data_ptr(), n_cw, d_counts, None), "svs_rs_decode_dev")  # noqa: E731
        fn.prepare = lambda: work.copy_(master[name])
        return fn

    s.say("  one decode of each case into zeroed counters: bytes corrected, codewords uncorrectable, codewords with status 0")
    for name in cases:
        counts.zero_()
        call = decode(name, counts.data_ptr())
        call.prepare()
        call()
        ratelib.sync()
        got = counts.cpu().numpy().view(np.uint32)
        s.say(f"    {name:42s} {int(got[0]):9d} {int(got[1]):7d} {int((status == 0).sum().item()):7d}")

    viterbi = "svs_fec_decode_soft_dev, rate 2, same payload"
    todo = {viterbi: lambda: fec.check(flib.svs_fec_decode_soft_dev(d_soft, n_info, 2, d_out, (n_info + 7) // 8, None),
                                       "svs_fec_decode_soft_dev")}
    todo.update({name: decode(name) for name in cases})
    t = s.measure(todo)
    base = statistics.median(t[viterbi])
    for name, v in t.items():
        s.say(ratelib.row(name, v, 46) + f"  spread {ratelib.spread(v):.1f} %" + ("" if name == viterbi else f"  {statistics.median(v) / base:.3f} x the Viterbi call"))
    clean = statistics.median(t["clean"])
    s.say(f"    the clean pass reads {total} bytes in {clean:.3f} ms: {total / clean / 1e6:.1f} GB/s")
    if not args.baseline_lib:
        s.say("  no --baseline-lib: the four cases were not timed against the parent commit's library")
    else:
        old = load_rs_build(args.baseline_lib)
        s.say(f"  against {os.path.basename(args.baseline_lib)} (the parent commit's libsvsrs.so), each pair alternated")
        s.against_baseline([(name, decode(name, build=old), decode(name)) for name in cases])
    s.close()


if __name__ == "__main__":
    main()
