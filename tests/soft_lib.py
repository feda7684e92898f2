"""Helpers of the soft-extraction tests (tests/test_soft_extract_cpu.py, tests/test_soft_extract_gpu.py): the NumPy model of
the format (include/svsdct.h) - the oracle's forward transform and quantiser index, the dither of dither_lib, the keyed order of
svsdct/order.py, and the seven float32 steps of the byte written out -, the host build of the soft block body and of a soft
call's routing (tests/soft/soft_emu.cpp), and the disturbed three-copy experiment the README's table comes from."""
import ctypes
import glob
import os
import subprocess

import numpy as np

import dither_lib as dl
from oracle.qim_dct_oracle import BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _quant_index, frame_embed
from testlib import CSRC, REPO

ZIGZAG = [1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]                      # JPEG zig-zag scan positions 1..63 as flat row-major indices


def zigzag(n):
    return ZIGZAG[:max(0, min(int(n), MAX_AC))]


# ---- the model ---------------------------------------------------------------------------------------------------------
def model_bytes(x, delta):
    """float32 quantiser inputs -> the soft bytes, every step one float32 operation"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    df = np.float32(delta)
    q = _quant_index(x, delta)                           # the extract call's own index
    x0 = q.astype(np.float32) * df                       # one multiply, in every quantiser mode
    a = np.abs(x - x0)
    h = np.float32(0.5) * df
    s = np.float32(254.0 / float(df))                    # rounded once
    v = (h - a) * s
    assert x0.dtype == a.dtype == v.dtype == np.float32
    m = np.clip(np.trunc(v.astype(np.float64)), 0, 127).astype(np.int64)   # truncation toward zero, then the clamp
    return (((q & 1) << 7) | m).astype(np.uint8)


def model_soft(gray, delta, n_ac=MAX_AC, index=None, key=None, t=0, perm=None):
    """One frame -> the soft bytes in stream order (dither_lib.model_extract with the byte in the place of the parity)"""
    _check_plane(gray)
    index = dl._index(n_ac, index)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    if index.size == 0:
        return np.zeros(0, np.uint8)
    if delta <= 0:
        return np.zeros(n_blocks * index.size, np.uint8)
    perm = np.arange(n_blocks) if perm is None else np.asarray(perm, np.int64)
    blk = _blocks_view(np.float32(gray)).reshape(1, n_blocks, BLOCK, BLOCK)
    x = _fwd(blk).reshape(n_blocks, BLOCK * BLOCK)[:, index]
    if key is not None:
        x = x - dl.dither_table(key, t, n_blocks, delta)[:, index]
    return model_bytes(np.ascontiguousarray(x, np.float32), delta)[perm].reshape(-1)


def model_batch_soft(frames, delta, n_ac=MAX_AC, index=None, key=None, first_frame=0, order_key=None):
    n_blocks = (frames.shape[1] // BLOCK) * (frames.shape[2] // BLOCK)
    return np.concatenate([model_soft(frames[f], delta, n_ac, index, key, first_frame + f,
                                      dl._perm(order_key, first_frame + f, n_blocks)) for f in range(frames.shape[0])])


def packed_hard(soft):
    return np.packbits(np.asarray(soft, np.uint8) >> 7)


# ---- the soft block body and a soft call's plan on the host (tests/soft/soft_emu.cpp) ---------------------------------------
_EMU = None
_PTR = ctypes.c_void_p
PLAN_FIELDS = ("path", "rows", "qm", "selected", "dithered", "soft", "keyed")
PATH_EXACT = 1          # svs::ExtractPath::EXACT


def soft_emu():
    """builds (when stale, as testlib.hostemu does) and loads tests/soft/libsvs_soft_emu.so"""
    global _EMU
    if _EMU is not None:
        return _EMU
    here = os.path.join(REPO, "tests", "soft")
    src, out = os.path.join(here, "soft_emu.cpp"), os.path.join(here, "libsvs_soft_emu.so")
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + [src]
    stale = not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)
    if stale and os.path.exists(out) and os.path.exists("/dev/kfd"):
        stale = False      # on a GPU box use the library built by build(): no compiler child processes there
    if stale:
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + CSRC, src, "-o", out])
    lib = ctypes.CDLL(out)
    lib.soft_emu_plan.restype = ctypes.c_int
    lib.soft_emu_plan.argtypes = [ctypes.c_double, ctypes.c_int, _PTR, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_uint64, _PTR]
    lib.soft_emu_extract.restype = ctypes.c_uint64
    lib.soft_emu_extract.argtypes = [_PTR, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, _PTR, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, _PTR]
    _EMU = lib
    return lib


def _index_arg(index):
    if index is None:
        return None, None, 0
    idx = np.ascontiguousarray(np.asarray(index, np.int64).reshape(-1).astype(np.uint8))
    return idx, idx.ctypes.data, idx.size


def host_plan(delta, n_ac, index=None, dither=False, order=False, flags=0, total_blocks=1000):
    """svs::plan_extract of a soft call -> dict of PLAN_FIELDS"""
    keep, ptr, count = _index_arg(index)
    out = np.zeros(len(PLAN_FIELDS), np.int32)
    rc = soft_emu().soft_emu_plan(float(delta), int(n_ac), ptr, count, int(dither), int(order), flags & 1, (flags >> 1) & 1,
                                  int(total_blocks), out.ctypes.data)
    assert rc == 0, "the host library refused the selection"
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def host_soft(frames, delta, n_ac, index=None, key=None, first_frame=0, order_key=None):
    """a soft call through the product headers on the host -> the soft bytes"""
    frames = np.ascontiguousarray(frames if frames.ndim == 3 else frames[None])
    f, h, w = frames.shape
    keep, ptr, count = _index_arg(index)
    n = count if count else max(0, min(int(n_ac), MAX_AC))
    out = np.full(f * (h // 8) * (w // 8) * n + 8, 0xA5, np.uint8)
    cap = soft_emu().soft_emu_extract(frames.ctypes.data, f, h, w, float(delta), int(n_ac), ptr, count, int(key is not None),
                                      int(key or 0), int(order_key is not None), int(order_key or 0), int(first_frame),
                                      out.ctypes.data)
    assert cap == out.size - 8, (cap, out.size - 8)
    assert (out[cap:] == 0xA5).all(), "the host body wrote past the capacity"
    return out[:cap]


# ---- three copies under pixel noise: the README's table -------------------------------------------------------------------
VOTE_SHAPE = (96, 160)
VOTE_ROWS = ((20, 10, 6), (20, 10, 8), (20, 10, 10), (8, 10, 3))     # (delta, n_ac, noise amplitude a)


def vote_experiment(delta, n_ac, amp, seed, copies=3):
    """The full payload of one frame, embedded by the oracle's frame_embed into `copies` frames of noise in [64, 192), uniform
    integer pixel noise of +-amp added to each stego, read with the model.  Fixed seeds: every number is reproducible.
    -> dict(single=[errors of each copy alone], majority=, soft=) payload bit errors"""
    from svsdct import soft as sv
    rng = np.random.default_rng(seed)
    h, w = VOTE_SHAPE
    cap = (h // 8) * (w // 8) * n_ac
    pay = rng.integers(0, 2, cap).astype(np.uint8)
    streams = []
    for _ in range(copies):
        cover = rng.integers(64, 192, (h, w)).astype(np.uint8)
        _, stego, used = frame_embed(cover, delta, pay, n_ac)
        assert used == cap
        noisy = np.clip(stego.astype(np.int64) + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)
        streams.append(model_soft(noisy, delta, n_ac))
    hard = np.array([s >> 7 for s in streams])
    single = [int((b != pay).sum()) for b in hard]
    majority = int(((2 * hard.sum(0) > copies).astype(np.uint8) != pay).sum())
    bits, _ = sv.combine(np.concatenate(streams), cap)
    return dict(single=single, majority=majority, soft=int((bits != pay).sum()))
