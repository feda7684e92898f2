"""Helpers of the soft-extraction tests (tests/test_soft_extract_cpu.py, tests/test_soft_extract_gpu.py): the NumPy model of
the format (include/svsdct.h) - the oracle's forward transform and quantiser index, the dither of dither_lib, the keyed order of
svsdct/order.py, and the seven float32 steps of the byte written out -, the soft block body and a soft call's routing
through the host build of the product headers (tests/hostemu), and the disturbed three-copy experiment the README's table
comes from."""
import numpy as np

import dither_lib as dl
import testlib
from oracle.qim_dct_oracle import BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _quant_index, frame_embed

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


# ---- the soft block body and a soft call's plan on the host (tests/hostemu: the extract walker with a soft output) --------
PLAN_FIELDS = ("path", "rows", "qm", "selected", "dithered", "soft", "keyed")
PATH_EXACT = 1          # svs::ExtractPath::EXACT


def host_plan(delta, n_ac, index=None, dither=False, order=False, flags=0, total_blocks=1000, output=testlib.EMU_SOFT, **call):
    """svs::plan_extract of a soft call -> dict of PLAN_FIELDS (no frames: the walker stops at the plan)"""
    res = testlib._emu_call("emu_extract_call", np.empty((total_blocks, 8, 8), np.uint8), delta, n_ac, index=index,
                            dither_key=0 if dither else None, block_key=0 if order else None, pocketfft=flags & 1,
                            guarded=(flags >> 1) & 1, output=output, **call)
    return {k: int(getattr(res, k)) for k in PLAN_FIELDS + ("vote", "hist")}


def host_soft(frames, delta, n_ac, index=None, key=None, first_frame=0, order_key=None):
    """a soft call through the product headers on the host -> the soft bytes"""
    frames = np.ascontiguousarray(frames if frames.ndim == 3 else frames[None])
    f, h, w = frames.shape
    n = len(index) if index is not None and len(index) else max(0, min(int(n_ac), MAX_AC))
    out = np.full(f * (h // 8) * (w // 8) * n + 8, 0xA5, np.uint8)
    cap = testlib._emu_call("emu_extract_call", frames, delta, n_ac, index=index, dither_key=key, block_key=order_key,
                            first_frame=int(first_frame), frames_in=frames, output=testlib.EMU_SOFT, soft_out=out).used
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
