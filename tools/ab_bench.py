#!/usr/bin/env python3
"""A/B timing of kernel build variants in ONE process, interleaved rounds (guide rule 24).

usage: python tools/ab_bench.py [--frames 600] [--rounds 15] [--n-ac 3] [--delta 8] [--h 2160 --w 3840] [--key K] lib1.so ...
--key K: every library is also timed with the keyed block order K (svs_embed_ordered_dev / svs_extract_ordered_dev), keyed
and unkeyed calls alternated in the same rounds (profiles/block_order_rates.txt).
Reports median / min kernel time (HIP events on the launch stream) and algorithmic GB/s, and checks that
every variant produces byte-identical stego frames and extracted bits.
"""
import argparse, ctypes as C, hashlib, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"))
import torch
from svsdct import native
from svsdct.native import Planes

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=600); ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--n-ac", type=int, default=3); ap.add_argument("--delta", type=float, default=8.0)
ap.add_argument("--h", type=int, default=2160); ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--mode", default="fast", choices=["fast", "guarded", "exact"])
ap.add_argument("--env-sweep", default="", help="NAME=v1,v2,...: sweep one environment knob on the first lib - which must be "
                "lib/variants/libsvsdct_exp.so (make -C csrc exp): the product library reads no environment variable")
ap.add_argument("--key", type=lambda x: int(x, 0), default=None, help="also time the keyed block order with this key")
ap.add_argument("libs", nargs="+")
a = ap.parse_args()
FLAGS = {"fast": 0, "exact": 1, "guarded": 2}[a.mode]       # SVS_EXACT_POCKETFFT = 1, SVS_EXACT_GUARDED = 2

from ratelib import load_build as load      # a library of an earlier round (lib/variants/libsvsdct_r02.so) lacks the newer entry points

libs = [(os.path.basename(p).replace("libsvsdct", "").replace(".so", "") or "base", load(p), None) for p in a.libs]
if a.env_sweep:
    _name, _vals = a.env_sweep.split("=")
    libs = [(f"{_name}={v}", libs[0][1], v) for v in _vals.split(",")]
if a.key is not None:
    libs = [v for name, lib, env_value in libs for v in ((name, lib, env_value), (name + "+key", lib, env_value))]
ORDER = native.BlockOrder(a.key or 0, 0, 0)
dev = torch.device("cuda", 0); torch.cuda.set_device(0)
F, H, W, n = a.frames, a.h, a.w, a.n_ac
planes = Planes.contiguous(F, H, W)
cap = F * (H // 8) * (W // 8) * min(n, 63); nbytes = (cap + 7) // 8
gray = torch.empty((F, H, W), dtype=torch.uint8, device=dev); stego = torch.empty_like(gray)
pay = torch.zeros(nbytes + 8, dtype=torch.uint8, device=dev); ext = torch.zeros(nbytes + 8, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream().cuda_stream
l0 = libs[0][1]
assert l0.svs_fill_synthetic_dev(gray.data_ptr(), C.byref(planes), 20250620, 0, 16, 224, st) == 0
assert l0.svs_fill_bits_dev(pay.data_ptr(), cap, 20250620, 0, st) == 0
torch.cuda.synchronize()
times = {name: {"embed": [], "extract": []} for name, _, _ in libs}
digests = {}
done = C.c_uint64()
for r in range(a.rounds + 2):
    for name, lib, env_value in libs:
        if env_value is not None:
            os.environ[_name] = env_value
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        keyed = name.endswith("+key")
        e[0].record()
        if keyed:
            rc = lib.svs_embed_ordered_dev(gray.data_ptr(), stego.data_ptr(), C.byref(planes), C.byref(ORDER), a.delta, n, pay.data_ptr(),
                                           0, cap, FLAGS, C.byref(done), st)
        else:
            rc = lib.svs_embed_dev(gray.data_ptr(), stego.data_ptr(), C.byref(planes), a.delta, n, pay.data_ptr(), 0, cap, FLAGS, C.byref(done), st)
        assert rc == 0, lib.svs_last_error()
        e[1].record()
        if keyed:
            rc = lib.svs_extract_ordered_dev(stego.data_ptr(), C.byref(planes), C.byref(ORDER), a.delta, n, ext.data_ptr(), ext.numel(),
                                             FLAGS, C.byref(done), st)
        else:
            rc = lib.svs_extract_dev(stego.data_ptr(), C.byref(planes), a.delta, n, ext.data_ptr(), ext.numel(), FLAGS, C.byref(done), st)
        assert rc == 0, lib.svs_last_error()
        e[2].record()
        torch.cuda.synchronize()
        if r >= 2:
            times[name]["embed"].append(e[0].elapsed_time(e[1])); times[name]["extract"].append(e[1].elapsed_time(e[2]))
        if r == 0:
            h = hashlib.sha256(stego[:2].cpu().numpy().tobytes()); h.update(ext[:nbytes].cpu().numpy().tobytes())
            digests[name] = h.hexdigest()[:16]
            same = bool(torch.equal(ext[:nbytes], pay[:nbytes]))
            digests[name] += " roundtrip_ok" if same else " ROUNDTRIP_MISMATCH"
# ceilings on this box: (1) the embed kernel's own access pattern with the arithmetic skipped (n_bits = 0 ->
# every lane copies its block), (2) torch's contiguous device-to-device copy
ceil = {"pattern_copy": [], "torch_copy": [], "copy16_nt": [], "copy_gridstride_nt": [], "copy_gridstride": [], "read_nt": [],
        "copy16_nt_sc1st": [], "copy16_nt_sc0sc1nt_st": [], "copy16_sc1ld_sc1st": []}
# the plain copy / read kernels are measurement hooks: they live in the experiments library only (round 5)
l0 = C.CDLL(os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd", "lib", "variants", "libsvsdct_exp.so"))
l0.svs_ref_copy_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
l0.svs_ref_read_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
sink = torch.zeros(4096, dtype=torch.int32, device=dev)
for r in range(a.rounds + 2):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    assert libs[0][1].svs_embed_dev(gray.data_ptr(), stego.data_ptr(), C.byref(planes), a.delta, n, pay.data_ptr(), 0, 0, 0, C.byref(done), st) == 0
    e[1].record()
    stego.copy_(gray)
    e[2].record()
    ey = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ey[0].record()
    for m in range(3):
        assert l0.svs_ref_copy_dev(gray.data_ptr(), stego.data_ptr(), gray.numel(), 3 + m, st) == 0
        ey[m + 1].record()
    ex = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ex[0].record()
    for m in range(3):
        assert l0.svs_ref_copy_dev(gray.data_ptr(), stego.data_ptr(), gray.numel(), m, st) == 0
        ex[m + 1].record()
    assert l0.svs_ref_read_dev(gray.data_ptr(), sink.data_ptr(), gray.numel(), st) == 0
    ex[4].record()
    torch.cuda.synchronize()
    if r >= 2:
        ceil["pattern_copy"].append(e[0].elapsed_time(e[1])); ceil["torch_copy"].append(e[1].elapsed_time(e[2]))
        for m, k in enumerate(["copy16_nt", "copy_gridstride_nt", "copy_gridstride"]):
            ceil[k].append(ex[m].elapsed_time(ex[m + 1]))
        for m, k in enumerate(["copy16_nt_sc1st", "copy16_nt_sc0sc1nt_st", "copy16_sc1ld_sc1st"]):
            ceil[k].append(ey[m].elapsed_time(ey[m + 1]))
        ceil["read_nt"].append(2 * ex[3].elapsed_time(ex[4]))   # x2: reported below against 2 B/px like the copies
eb, xb = F * H * W * 2 + nbytes, F * H * W + nbytes
for k, v in ceil.items():
    print(f"{k:18s} copy  med {statistics.median(v):7.4f} min {min(v):7.4f} ms -> {F*H*W*2/statistics.median(v)/1e6:7.1f} GB/s")
print(f"{F} frames {W}x{H} n={n} delta={a.delta:g}; {a.rounds} interleaved rounds")
for name, _, _ in libs:
    te, tx = times[name]["embed"], times[name]["extract"]
    print(f"{name:18s} embed med {statistics.median(te):7.4f} min {min(te):7.4f} ms -> {eb/statistics.median(te)/1e6:7.1f} GB/s | "
          f"extract med {statistics.median(tx):7.4f} min {min(tx):7.4f} ms -> {xb/statistics.median(tx)/1e6:7.1f} GB/s | {digests[name]}")
