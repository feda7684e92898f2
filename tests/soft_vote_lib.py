"""Helpers of the fused soft-vote tests (tests/test_soft_vote_cpu.py, tests/test_soft_vote_gpu.py): the host build of the
vote's integer side (tests/soft/vote_emu.cpp - the launch arguments, the residue of a bit, the vote of a byte) and the periods
at which the kernel's vote tail takes another path."""
import ctypes
import glob
import os
import subprocess

import numpy as np

from testlib import CSRC, REPO

_EMU = None
_PTR = ctypes.c_void_p


def vote_emu():
    """builds (when stale, as soft_lib.soft_emu does) and loads tests/soft/libsvs_vote_emu.so"""
    global _EMU
    if _EMU is not None:
        return _EMU
    here = os.path.join(REPO, "tests", "soft")
    src, out = os.path.join(here, "vote_emu.cpp"), os.path.join(here, "libsvs_vote_emu.so")
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + [src]
    stale = not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)
    if stale and os.path.exists(out) and os.path.exists("/dev/kfd"):
        stale = False      # on a GPU box use the library built by build(): no compiler child processes there
    if stale:
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + CSRC, src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.vote_emu_args.restype = None
    lib.vote_emu_args.argtypes = [ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, _PTR, _PTR]
    lib.vote_emu_residues.restype = None
    lib.vote_emu_residues.argtypes = [ctypes.c_uint64, ctypes.c_uint64, _PTR, ctypes.c_uint64, _PTR, _PTR]
    lib.vote_emu_vote.restype = ctypes.c_int32
    lib.vote_emu_vote.argtypes = [ctypes.c_uint32, ctypes.c_int]
    lib.vote_emu_period_max.restype = ctypes.c_uint64
    lib.vote_emu_period_max.argtypes = []
    _EMU = lib
    return lib


def host_vote_args(delta, n_ac, period, stream_bit0):
    """-> (plan dict, SoftArgs dict) of a vote call through svs_route.hpp"""
    plan, fields = np.zeros(4, np.int32), np.zeros(4, np.uint64)
    vote_emu().vote_emu_args(float(delta), int(n_ac), int(period), int(stream_bit0), plan.ctypes.data, fields.ctypes.data)
    return (dict(zip(("path", "rows", "soft", "vote"), map(int, plan))),
            dict(zip(("vote", "period", "base", "head"), map(int, fields))))


def host_residues(period, stream_bit0, indices):
    """-> ([(stream_bit0 + i) mod period], [stream_bit0 + i < period]) as the kernel takes them, Python ints and bools"""
    i = np.asarray(indices, np.uint64)
    res, head = np.zeros(i.size, np.uint64), np.zeros(i.size, np.uint8)
    vote_emu().vote_emu_residues(int(period), int(stream_bit0), i.ctypes.data, i.size, res.ctypes.data, head.ctypes.data)
    return [int(r) for r in res], [bool(h) for h in head]


def landmark_periods(f, h, w, n):
    """The periods at which the vote tail can go wrong for a stack of f frames of h x w at n coefficients: one entry; one block
    and its neighbours; the 64-entry threshold of the keyed pre-reduction; a wave's run of 64 n bytes +- 1 (the threshold of
    the raster pre-reduction); a frame +- 1; two frames +- 1; the capacity +- 1; beyond the capacity."""
    bpf = (h // 8) * (w // 8)
    cap = f * bpf * n
    want = {1, 7, n - 1, n, n + 1, 63, 64, 65, 64 * n - 1, 64 * n, 64 * n + 1, bpf * n - 1, bpf * n, bpf * n + 1, 2 * bpf * n - 1,
            2 * bpf * n, 2 * bpf * n + 1, cap // 3 + 1, cap - 1, cap, cap + 1, 100_000}
    return sorted(p for p in want if p >= 1)
