"""Cost of the device encoders (include/svsenc.h: svs_rs_encode_dev, svs_fec_encode_dev, svs_bits_tile_dev) beside the launch they
feed, svs_embed_dev at n_ac = 10 in the product's default mode on the same frames in the same process, and beside the host
encoders they stand in for, timed on the same machine.  The workload is the payload that fills rate 1/2 under the outer code:
k = svs_rs_data_bytes(svs_fec_info_bits(capacity, 2) / 8) random data bytes.
  svs_rs_encode_dev            out of place (the data is copied by the launch) and in place (parity only)
  svs_fec_encode_dev           at the rate codes 2, 3, 34 and 78, each on the payload that fills the capacity at that rate, so every
                               call writes capacity / 8 bytes
  svs_bits_tile_dev            a period of capacity / 3 bits tiled to the capacity
  svs_embed_dev                reading the rate-2 coded stream
The device calls are alternated inside every repetition and the order rotated from one repetition to the next, HIP events.  The
device's RS stream and its rate-2 coded stream are compared with the host encoders' bytes before anything is timed.
svs_rs_encode and svs_fec_encode (rate codes 2 and 34) run on the host with a host clock, and batch.embed_coded_frames end to end
(frames and payload on the host, stego back on the host) with encoder="host" against encoder="device" with a wall clock round
the call, which synchronises.  No ratio is asserted: the file reports the times and their ratios to the embed launch.
Output: profiles/enc_rates.txt.

    python tools/enc_rates.py [--host-reps 3]
"""
import statistics
import time

import numpy as np

import ratelib

from svsdct import batch, enc, fec, native, rs

DELTA, N = 20.0, 10
C_RATES = (2, 3, 34, 78)
HOST_RATES = (2, 34)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = ratelib.parser("enc_rates.txt", reps=15)
    ap.add_argument("--host-reps", type=int, default=3, help="repetitions of each host-clock timing")
    args = ap.parse_args()
    s = ratelib.Session(args)
    torch = ratelib._torch
    lib, elib, flib, rlib = s.lib, enc.load(), fec.load(), rs.load()
    cap = s.capacity(N)
    k = int(rlib.svs_rs_data_bytes(int(flib.svs_fec_info_bits(cap, 2)) // 8))
    n_cw, total = rs.codewords(k), rs.coded_bytes(k)
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, k).astype(np.uint8)
    n_infos = {rate: int(flib.svs_fec_info_bits(cap, rate)) for rate in C_RATES}
    info = rng.integers(0, 256, (max(n_infos.values()) + 7) // 8).astype(np.uint8)       # packed payload bits for the inner code alone
    cap_bytes = (cap + 7) // 8
    d_data = torch.from_numpy(data).cuda()
    d_info = torch.from_numpy(info).cuda()
    d_stream = torch.empty(total + 1, dtype=torch.uint8, device="cuda")[1:]               # an odd address: any alignment
    d_place = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_place[:k] = d_data
    d_coded = torch.empty(cap_bytes + 8, dtype=torch.uint8, device="cuda")
    d_tiled = torch.empty(cap_bytes + 8, dtype=torch.uint8, device="cuda")
    s.noise()
    s.say(f"device encoders, {s.f} x {s.w}x{s.h} gray frames at n_ac = {N}: capacity {cap} bits; the payload that fills rate 1/2 under the "
          f"outer code is k = {k} data bytes, {n_cw} codewords, {total} stream bytes; {args.reps} alternated repetitions "
          f"({s.order_text()}), HIP events; ms per call: median (min .. max)")

    def rs_call(src, dst):
        return lambda: enc.check(elib.svs_rs_encode_dev(src.data_ptr(), k, dst.data_ptr(), total, None), "svs_rs_encode_dev")

    def fec_call(src, n_info, rate):
        return lambda: enc.check(elib.svs_fec_encode_dev(src.data_ptr(), n_info, rate, d_coded.data_ptr(), cap_bytes + 8, None),
                                 "svs_fec_encode_dev")

    # the bytes are the host encoders': the RS stream, and the rate-2 coded stream of it (which the embed call below then reads)
    host_stream = rs.encode_array(data)
    rs_call(d_data, d_stream)()
    rs_call(d_place, d_place)()
    ratelib.sync()
    same_rs = bool((d_stream.cpu().numpy() == host_stream).all() and (d_place.cpu().numpy() == host_stream).all())
    host_coded = np.empty((fec.coded_bits(8 * total, 2) + 7) // 8, np.uint8)
    fec.check(flib.svs_fec_encode(host_stream.ctypes.data, 8 * total, 2, host_coded.ctypes.data, host_coded.size, None), "svs_fec_encode")
    fec_call(d_place, 8 * total, 2)()
    ratelib.sync()
    same_fec = bool((d_coded[: host_coded.size].cpu().numpy() == host_coded).all())
    s.say(f"  the device's bytes are the host encoders': RS stream out of place and in place {same_rs}, rate-2 coded stream {same_fec}")
    assert same_rs and same_fec

    period = cap // 3
    embed = "svs_embed_dev, default mode, reading the coded stream"
    flags = batch.embed_flags()
    todo = {embed: lambda: native.check(lib.svs_embed_dev(s.gray, s.stego, s.P, DELTA, N, d_coded.data_ptr(), 0, cap, flags,
                                                          ratelib.C.byref(s.done), None), "svs_embed_dev"),
            f"svs_rs_encode_dev, out of place, {total} bytes": rs_call(d_data, d_stream),
            "svs_rs_encode_dev, in place": rs_call(d_place, d_place)}
    for rate in C_RATES:
        todo[f"svs_fec_encode_dev, rate code {rate}, n_info {n_infos[rate]}"] = fec_call(d_info, n_infos[rate], rate)
    todo[f"svs_bits_tile_dev, period {period} -> {cap} bits"] = lambda: enc.check(
        elib.svs_bits_tile_dev(d_coded.data_ptr(), period, d_tiled.data_ptr(), cap, cap_bytes + 8, None), "svs_bits_tile_dev")
    t = s.measure(todo)
    base = statistics.median(t[embed])
    for name, v in t.items():
        s.say(ratelib.row(name, v, 58) + f"  spread {ratelib.spread(v):.1f} %" + ("" if name == embed else f"  {statistics.median(v) / base:.3f} x the embed launch"))
    above = [name for name, v in t.items() if name != embed and statistics.median(v) >= base]
    s.say(f"  encoder calls at or above the embed launch they feed: {len(above)}" + "".join(f"\n    {name}" for name in above))

    s.say(f"  the host encoders on this machine's CPU, host clock, {args.host_reps} repetitions; ms: median (min .. max); the ratio is to the device call above")
    out = np.empty(total, np.uint8)
    v = wall(lambda: rs.check(rlib.svs_rs_encode(data.ctypes.data, k, out.ctypes.data, total, None), "svs_rs_encode"), args.host_reps)
    dev = statistics.median(t[f"svs_rs_encode_dev, out of place, {total} bytes"])
    s.say(ratelib.row(f"svs_rs_encode, {k} data bytes", v, 58) + f"  {statistics.median(v) / dev:.0f} x")
    coded = np.empty(cap_bytes + 8, np.uint8)
    for rate in HOST_RATES:
        n_info = n_infos[rate]
        v = wall(lambda: fec.check(flib.svs_fec_encode(info.ctypes.data, n_info, rate, coded.ctypes.data, coded.size, None), "svs_fec_encode"),
                 args.host_reps)
        dev = statistics.median(t[f"svs_fec_encode_dev, rate code {rate}, n_info {n_info}"])
        s.say(ratelib.row(f"svs_fec_encode, rate code {rate}, n_info {n_info}", v, 58) + f"  {statistics.median(v) / dev:.0f} x")

    s.say(f"  batch.embed_coded_frames end to end (frames and payload on the host, stego back on the host), rate 2, outer=True, wall clock, "
          f"{args.host_reps} alternated repetitions; ms: median (min .. max)")
    frames = torch.randint(0, 256, (s.f, s.h, s.w), dtype=torch.uint8).numpy()
    bits = np.unpackbits(data)
    sides = {side: [] for side in ("host", "device")}
    stego = {}
    for _ in range(args.host_reps + 1):                          # the first repetition warms both sides up and is not kept
        for side in sides:
            t0 = time.perf_counter()
            stego[side] = batch.embed_coded_frames(frames, DELTA, N, bits, rate=2, outer=True, encoder=side)[0]
            sides[side].append(1e3 * (time.perf_counter() - t0))
    same = bool((stego["host"] == stego["device"]).all())
    for side, v in sides.items():
        s.say(ratelib.row(f'encoder="{side}"', v[1:], 58))
    s.say(f"    the two stego stacks are the same bytes: {same}")
    assert same
    s.close()


if __name__ == "__main__":
    main()
