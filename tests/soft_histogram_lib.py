"""Helpers of the fused soft-histogram tests (tests/test_soft_histogram_cpu.py, tests/test_soft_histogram_gpu.py): the host
build of the histogram's integer side (tests/soft/hist_emu.cpp - the plan, the launch arguments, the split of a wave's run of
blocks into per-frame runs), the shapes at which the frame split can go wrong, and the scenario of
examples/find_payload_frames.py."""
import ctypes
import glob
import os
import subprocess

import numpy as np

from testlib import CSRC, REPO

_EMU = None
_PTR = ctypes.c_void_p
WG = 256                # blocks of a workgroup (csrc/svs_device.hpp SVS_WG)

# name -> (frames, height, width): blocks per frame 1, 1, 6, 6, 120, 64, 256, 257
SHAPES = {"one_block": (1, 8, 8), "one_block_frames": (70, 8, 8), "tight": (2, 16, 24), "pitched": (2, 16, 24),
          "straddle": (5, 64, 120), "wave_edge": (3, 64, 64), "workgroup_edge": (2, 128, 128), "past_workgroup_edge": (3, 8, 2056)}


def hist_emu():
    """builds (when stale, as soft_lib.soft_emu does) and loads tests/soft/libsvs_hist_emu.so"""
    global _EMU
    if _EMU is not None:
        return _EMU
    here = os.path.join(REPO, "tests", "soft")
    src, out = os.path.join(here, "hist_emu.cpp"), os.path.join(here, "libsvs_hist_emu.so")
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + [src]
    stale = not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)
    if stale and os.path.exists(out) and os.path.exists("/dev/kfd"):
        stale = False      # on a GPU box use the library built by build(): no compiler child processes there
    if stale:
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + CSRC, src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.hist_emu_args.restype = ctypes.c_uint64
    lib.hist_emu_args.argtypes = [ctypes.c_double, ctypes.c_uint32, ctypes.c_int, _PTR, _PTR]
    lib.hist_emu_runs.restype = ctypes.c_uint32
    lib.hist_emu_runs.argtypes = [ctypes.c_uint32] * 5 + [_PTR, ctypes.c_uint32]
    lib.hist_emu_bins.restype = ctypes.c_uint32
    lib.hist_emu_bins.argtypes = []
    _EMU = lib
    return lib


def host_hist_args(delta, n_ac, keyed=False):
    """-> (plan dict, SoftArgs dict, sizeof(SoftArgs)) of a histogram call through svs_route.hpp"""
    plan, fields = np.zeros(6, np.int32), np.zeros(3, np.uint32)
    size = hist_emu().hist_emu_args(float(delta), int(n_ac), int(keyed), plan.ctypes.data, fields.ctypes.data)
    return (dict(zip(("path", "rows", "soft", "vote", "hist", "keyed"), map(int, plan))),
            dict(zip(("on", "vote", "hist"), map(int, fields))), int(size))


def host_runs(wg_first, wave_first, total, bpf):
    """-> [(frame, begin, end)] of the wave at wave_first in the workgroup at wg_first, as the kernel's tail walks them"""
    out = np.zeros(3 * (WG + 2), np.uint32)
    k = hist_emu().hist_emu_runs(int(wg_first), WG, int(wave_first), int(total), int(bpf), out.ctypes.data, WG + 2)
    return [tuple(int(v) for v in out[3 * i: 3 * i + 3]) for i in range(k)]


def python_runs(wg_first, wave_first, total, bpf):
    """the same in Python integers: for every frame the workgroup's live blocks touch, the wave's live blocks inside it"""
    wg_last = min(wg_first + WG, total) - 1
    if wg_last < wg_first:
        return []
    lo, hi = wave_first, max(wave_first, min(wave_first + 64, total))
    out = []
    for f in range(wg_first // bpf, wg_last // bpf + 1):
        b, e = max(lo, min(hi, f * bpf)), max(lo, min(hi, (f + 1) * bpf))
        out.append((f, b - lo, e - lo))
    return out


# ---- the scenario of examples/find_payload_frames.py ---------------------------------------------------------------------
SCENARIO = dict(frames=8, height=240, width=320, delta=20, n_ac=10, key=0x5EED0FD17E12, first=2, last=4, seed=7)


def scenario_cover():
    s = SCENARIO
    return np.random.default_rng(s["seed"]).integers(16, 240, (s["frames"], s["height"], s["width"])).astype(np.uint8)


def scenario_payload():
    s = SCENARIO
    per_frame = (s["height"] // 8) * (s["width"] // 8) * s["n_ac"]
    return np.random.default_rng(s["seed"] + 1).integers(0, 2, (s["last"] - s["first"] + 1) * per_frame).astype(np.uint8)


def scenario_stego_model():
    """the clip with frames first..last replaced by the NumPy model's dithered stego (dither_lib), first_frame = first"""
    import dither_lib as dl
    s = SCENARIO
    clip = scenario_cover()
    lo, hi = s["first"], s["last"] + 1
    stego, used = dl.model_batch_embed(clip[lo:hi], s["delta"], scenario_payload(), s["n_ac"], key=s["key"], first_frame=lo)
    assert used == scenario_payload().size
    clip[lo:hi] = stego
    return clip


def assert_scenario(with_key, without_key):
    """lattice_share per frame of the clip read with the key and without it: 1.0 on the payload frames with the key, a fair
    coin (0.45 .. 0.55) everywhere else"""
    s = SCENARIO
    for f in range(s["frames"]):
        if s["first"] <= f <= s["last"]:
            assert with_key[f] == 1.0, (f, with_key[f])
        else:
            assert 0.45 <= with_key[f] <= 0.55, (f, with_key[f])
        assert 0.45 <= without_key[f] <= 0.55, (f, without_key[f])
