"""Cost of the errors-and-erasures decoder (include/svsrse.h svs_rse_decode_dev) beside the call in front of it, the Viterbi
decoder (svs_fec_decode_soft_dev at rate 2) on the same payload, all in one process.  svs_rs_decode_dev (include/svsrs.h) runs
the same kernel without a mask; tools/rs_rates.py --baseline-lib times that against an earlier build.  The workload is that of
tools/rs_rates.py: the RS stream that fills svs_fec_info_bits of the frames' capacity at n_ac = 10, rate 1/2.  Cases:
  clean, NULL mask             the screening pass without the mask load
  clean, mask of zeros         what the second byte load costs the clean pass
  clean, a run of 32 C erased  every codeword has f = 32 and a zero remainder: status 0 from the screening pass
  that run randomised          every codeword repairs at f = 32: 32 locator steps, no Berlekamp-Massey step, degree 32
  16 errors, NULL mask         every codeword repaired at the blind limit
The decoders work in place, so before every timed call the received stream is copied back over the working buffer, outside the
pair of HIP events.  The calls are alternated inside every repetition and the order rotated from one repetition to the next.
Before the timing each case is decoded once into zeroed counters, which the report shows.  No ratio is asserted: the file
reports the times and their ratios to the Viterbi call.
Output: profiles/rse_rates.txt.

    python tools/rse_rates.py
"""
import statistics

import numpy as np

import ratelib
from ratelib import X
from rs_rates import received

from svsdct import fec, rs, rse

DELTA, N = 20.0, 10


def main():
    args = ratelib.parser("rse_rates.txt", reps=15).parse_args()
    s = ratelib.Session(args)
    torch = ratelib._torch
    lib, flib, rlib, elib = s.lib, fec.load(), rs.load(), rse.load()
    cap = s.capacity(N)
    info_cap = int(flib.svs_fec_info_bits(cap, 2))
    k = int(rlib.svs_rs_data_bytes(info_cap // 8))
    n_cw, total = rs.codewords(k), rs.coded_bytes(k)
    n_info = 8 * total
    rng = np.random.default_rng(7)
    sent = rs.encode_array(rng.integers(0, 256, k).astype(np.uint8))
    run = rse.mask(k, [(n_cw, 33 * n_cw)])                              # inside the data bytes: 32 bytes of every codeword
    randomised = sent.copy()
    randomised[n_cw: 33 * n_cw] ^= rng.integers(1, 256, 32 * n_cw).astype(np.uint8)
    sixteen = received(sent, k, rng, 1, 16, 16)
    zeros = np.zeros(total, np.uint8)
    # name -> (received stream, mask or None)
    cases = {"clean, NULL mask": (sent, None),
             "clean, mask of zeros": (sent, zeros),
             "clean, a run of 32 C bytes erased": (sent, run),
             "that run randomised: every codeword f = 32": (randomised, run),
             "every codeword with 16 errors, NULL mask": (sixteen, None)}
    master = {name: torch.from_numpy(a).cuda() for name, (a, _) in cases.items()}
    masks = {name: None if m is None else torch.from_numpy(np.concatenate([[0], m]).astype(np.uint8)).cuda()[1:] for name, (_, m) in cases.items()}
    work = torch.empty(total + 1, dtype=torch.uint8, device="cuda")[1:]                 # an odd address: any alignment
    status = torch.empty(n_cw, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_soft, d_out = s.dev(s.cap_max + 8), s.dev((info_cap + 7) // 8 + 8)
    s.noise()
    s.say(f"errors-and-erasures Reed-Solomon decoder, the stream that fills the rate-1/2 payload of {s.f} x {s.w}x{s.h} gray frames at "
          f"n_ac = {N}: k = {k} data bytes, {n_cw} codewords, {total} bytes; {args.reps} alternated repetitions ({s.order_text()}), "
          f"HIP events; ms per call: median (min .. max)")
    s.embed(lib, DELTA, N, X)()
    s.soft(lib, DELTA, N, d_soft)()                        # the soft bytes the Viterbi decoder reads
    ratelib.sync()

    def new(name, d_counts=None):
        m = masks[name]
        fn = lambda: rse.check(elib.svs_rse_decode_dev(work.data_ptr(), k, None if m is None else m.data_ptr(), status.data_ptr(), n_cw,  # noqa: E731
                                                       d_counts, None), "svs_rse_decode_dev")
        fn.prepare = lambda: work.copy_(master[name])
        return fn

    s.say("  one decode of each case into zeroed counters: bytes changed, codewords with status 255, codewords with status 0")
    for name in cases:
        counts.zero_()
        call = new(name, counts.data_ptr())
        call.prepare()
        call()
        ratelib.sync()
        got = counts.cpu().numpy().view(np.uint32)
        s.say(f"    {name:46s} {int(got[0]):9d} {int(got[1]):7d} {int((status == 0).sum().item()):7d}")

    viterbi = "svs_fec_decode_soft_dev, rate 2, same payload"
    todo = {viterbi: lambda: fec.check(flib.svs_fec_decode_soft_dev(d_soft, n_info, 2, d_out, (n_info + 7) // 8, None),
                                       "svs_fec_decode_soft_dev")}
    todo.update({name: new(name) for name in cases})
    t = s.measure(todo)
    base = statistics.median(t[viterbi])
    for name, v in t.items():
        s.say(ratelib.row(name, v, 50) + f"  spread {ratelib.spread(v):.1f} %" + ("" if name == viterbi else f"  {statistics.median(v) / base:.3f} x the Viterbi call"))
    clean, masked = statistics.median(t["clean, NULL mask"]), statistics.median(t["clean, mask of zeros"])
    s.say(f"    the clean pass reads {total} bytes in {clean:.3f} ms: {total / clean / 1e6:.1f} GB/s; with the mask beside them "
          f"{2 * total} bytes in {masked:.3f} ms: {2 * total / masked / 1e6:.1f} GB/s")
    s.close()


if __name__ == "__main__":
    main()
