"""Helpers of the fused soft-histogram tests (tests/test_soft_histogram_cpu.py, tests/test_soft_histogram_gpu.py): the
histogram's integer side through tests/hostemu (the plan, the launch arguments, the split of a wave's run of blocks into
per-frame runs, a whole call's counts), the shapes at which the frame split can go wrong, and the scenario of
examples/find_payload_frames.py."""
import numpy as np

import soft_lib as sl
import testlib

WG = 256                # blocks of a workgroup (csrc/svs_device.hpp SVS_WG)

# name -> (frames, height, width): blocks per frame 1, 1, 6, 6, 120, 64, 256, 257
SHAPES = {"one_block": (1, 8, 8), "one_block_frames": (70, 8, 8), "tight": (2, 16, 24), "pitched": (2, 16, 24),
          "straddle": (5, 64, 120), "wave_edge": (3, 64, 64), "workgroup_edge": (2, 128, 128), "past_workgroup_edge": (3, 8, 2056)}


def host_hist_args(delta, n_ac, keyed=False):
    """-> (plan dict, SoftArgs dict, sizeof(SoftArgs)) of a histogram call through svs_route.hpp"""
    plan = sl.host_plan(delta, n_ac, order=keyed, output=testlib.EMU_HIST)
    args = testlib.host_soft_args((1000, 8, 8), delta, n_ac, block_key=0 if keyed else None, output=testlib.EMU_HIST)
    return ({k: plan[k] for k in ("path", "rows", "soft", "vote", "hist", "keyed")}, {k: args[k] for k in ("on", "vote", "hist")},
            args["size"])


def host_runs(wg_first, wave_first, total, bpf):
    """-> [(frame, begin, end)] of the wave at wave_first in the workgroup at wg_first, as the kernel's tail walks them"""
    out = np.zeros(3 * (WG + 2), np.uint32)
    k = testlib.hostemu().emu_hist_runs(int(wg_first), WG, int(wave_first), int(total), int(bpf), out.ctypes.data, WG + 2)
    return [tuple(int(v) for v in out[3 * i: 3 * i + 3]) for i in range(k)]


def host_hist(frames, delta, n_ac, **call):
    """a histogram call through the product headers on the host (the extract walker) -> uint32 [F, 256], from zero"""
    frames = np.ascontiguousarray(frames)
    hist = np.zeros((frames.shape[0], 256), np.uint32)
    testlib._emu_call("emu_extract_call", frames, delta, n_ac, frames_in=frames, output=testlib.EMU_HIST, hist=hist, **call)
    return hist


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
