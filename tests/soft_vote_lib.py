"""Helpers of the fused soft-vote tests (tests/test_soft_vote_cpu.py, tests/test_soft_vote_gpu.py): the vote's integer
side through tests/hostemu (the launch arguments, the residue of a bit, a whole call's tally) and the periods
at which the kernel's vote tail takes another path."""
import ctypes

import numpy as np

import soft_lib as sl
import testlib

SHAPE = (1000, 8, 8)        # frames of the calls that are asked for their plan and launch arguments alone


def host_vote_args(delta, n_ac, period, stream_bit0):
    """-> (plan dict, SoftArgs dict) of a vote call through svs_route.hpp"""
    vote = dict(output=testlib.EMU_VOTE, vote_period=int(period), vote_bit0=int(stream_bit0))
    plan, args = sl.host_plan(delta, n_ac, **vote), testlib.host_soft_args(SHAPE, delta, n_ac, **vote)
    return {k: plan[k] for k in ("path", "rows", "soft", "vote")}, {k: args[k] for k in ("vote", "period", "base", "head")}


def host_residues(period, stream_bit0, indices):
    """-> ([(stream_bit0 + i) mod period], [stream_bit0 + i < period]) as the kernel takes them, Python ints and bools"""
    i = np.asarray(indices, np.uint64)
    res, head = np.zeros(i.size, np.uint64), np.zeros(i.size, np.uint8)
    call, keep = testlib._fill_call(SHAPE, 20.0, 10, output=testlib.EMU_VOTE, vote_period=int(period), vote_bit0=int(stream_bit0))
    assert testlib.hostemu().emu_vote_residues(ctypes.byref(call), i.ctypes.data, i.size, res.ctypes.data, head.ctypes.data) == 0
    return [int(r) for r in res], [bool(h) for h in head]


def host_tally(frames, delta, n_ac, period, stream_bit0=0, **call):
    """a vote call through the product headers on the host (the extract walker) -> the tally, int32 [period], from zero"""
    frames = np.ascontiguousarray(frames)
    tally = np.zeros(int(period), np.int32)
    testlib._emu_call("emu_extract_call", frames, delta, n_ac, frames_in=frames, output=testlib.EMU_VOTE, vote_period=int(period),
                      vote_bit0=int(stream_bit0), tally=tally, **call)
    return tally


def landmark_periods(f, h, w, n):
    """The periods at which the vote tail can go wrong for a stack of f frames of h x w at n coefficients: one entry; one block
    and its neighbours; the 64-entry threshold of the keyed pre-reduction; a wave's run of 64 n bytes +- 1 (the threshold of
    the raster pre-reduction); a frame +- 1; two frames +- 1; the capacity +- 1; beyond the capacity."""
    bpf = (h // 8) * (w // 8)
    cap = f * bpf * n
    want = {1, 7, n - 1, n, n + 1, 63, 64, 65, 64 * n - 1, 64 * n, 64 * n + 1, bpf * n - 1, bpf * n, bpf * n + 1, 2 * bpf * n - 1,
            2 * bpf * n, 2 * bpf * n + 1, cap // 3 + 1, cap - 1, cap, cap + 1, 100_000}
    return sorted(p for p in want if p >= 1)
