"""Helpers of the requantisation-channel tests (tests/test_requantise_cpu.py, tests/test_requantise_gpu.py): the NumPy model of
the format (include/svsdct.h, "requantisation channel") built from the oracle's own pieces - its block view, its pocketfft
forward and inverse - with float32 division, np.rint and a rounding store; the tables and frames the GPU test runs, so that the
CPU tier can check what those inputs exercise; and the survival experiment the README's table comes from."""
import numpy as np

import minmove_lib as ml
import soft_lib as sl
from oracle.qim_dct_oracle import BLOCK, _blocks_view, _fwd, _inv, frame_embed
from svsdct import channel
from svsdct import soft as sv


# ---- the model ---------------------------------------------------------------------------------------------------------------
def model_requantise(frames, steps, counts=None):
    """uint8 [F,H,W] (or one plane) -> the channel's output, every step one float32 operation in the header's order.
    counts (optional dict) receives `q_ties`, the quantiser inputs c / step exactly on k + 1/2, `p_ties`, the inverse outputs
    exactly on k + 1/2, and `low` / `high`, the pixels whose rounded value lay below 0 / above 255."""
    frames = np.asarray(frames, np.uint8)
    stack = frames if frames.ndim == 3 else frames[None]
    st = np.asarray(steps).reshape(64).astype(np.float32)[None, :]
    f, h, w = stack.shape
    nb = (h // BLOCK) * (w // BLOCK)
    out = np.empty_like(stack)
    tally = dict(q_ties=0, p_ties=0, low=0, high=0)
    for i in range(f):
        c = _fwd(_blocks_view(np.float32(stack[i])).reshape(1, nb, BLOCK, BLOCK)).reshape(nb, 64)
        c[:, 0] = c[:, 0] - np.float32(1024)
        x = c / st
        q = np.rint(x)
        c2 = q * st
        assert c.dtype == x.dtype == c2.dtype == np.float32
        c2[:, 0] = c2[:, 0] + np.float32(1024)
        rec = _inv(c2.reshape(1, nb, BLOCK, BLOCK)).reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
        assert rec.dtype == np.float32
        r = np.rint(rec)
        out[i] = np.uint8(np.clip(r, 0, 255))
        tally["q_ties"] += int((np.abs(x - np.floor(x)) == 0.5).sum())
        tally["p_ties"] += int((rec - np.floor(rec) == 0.5).sum())
        tally["low"] += int((r < 0).sum())
        tally["high"] += int((r > 255).sum())
    if counts is not None:
        counts.update(tally)
    return out if frames.ndim == 3 else out[0]


# ---- what the GPU test runs (tests/test_requantise_gpu.py); the CPU tier checks what these inputs exercise ---------------------
def odd_steps():
    """64 distinct odd steps 3, 5, 7, 11, 13, ...: the odd numbers that are no multiple of 3 after 3 itself, and then 9, 15, .. - no
    step is a power of two, so no division is a multiplication in disguise"""
    primes_like = [3] + [v for v in range(5, 256, 2) if v % 3]
    return np.array(primes_like[:64], np.uint16)


def dc_only(value):
    t = np.ones(64, np.uint16)
    t[0] = value
    return t


TABLES = {
    "ones": np.ones(64, np.uint16),
    "q90": channel.quality_steps(90),
    "q75": channel.quality_steps(75),
    "q50": channel.quality_steps(50),
    "all255": np.full(64, 255, np.uint16),
    "odd": odd_steps(),
    "dc200": dc_only(200),
    "ac200": np.where(np.arange(64) == 0, 1, 200).astype(np.uint16),
}

SHAPES = {"one_block": (1, 8, 8), "even": (3, 48, 272), "odd": (3, 40, 200)}     # the last two: kernel_matrix.SHAPES
PITCHED = "even"                                                                 # the shape that is also run with padding
CONTENTS = ("full", "mid", "flat", "stego")
CONTENT_SEED = 11


def content(kind, shape):
    """the frames of one content kind at one shape: noise in [0, 256) (saturates), noise in [64, 192), flat frames at 0, 127, 128
    and 255 (cycled over the frames; at one block: four frames), reference-rule stego at delta = 20, n = 10"""
    f, h, w = shape
    rng = np.random.default_rng(CONTENT_SEED)
    if kind == "full":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "mid":
        return rng.integers(64, 192, shape).astype(np.uint8)
    if kind == "flat":
        levels = (0, 127, 128, 255)
        return np.stack([np.full((h, w), levels[i % 4], np.uint8) for i in range(max(f, 4))])
    cover = rng.integers(16, 240, shape).astype(np.uint8)
    cap = (h // 8) * (w // 8) * 10
    return np.stack([frame_embed(cover[i], 20, rng.integers(0, 2, cap).astype(np.uint8), 10)[1] for i in range(f)])


def gpu_cases():
    """(shape name, content kind, frames) of every batch the GPU test sends through every table"""
    return [(s, k, content(k, SHAPES[s])) for s in SHAPES for k in CONTENTS]


# ---- embed, requantise, read: the README's table and the example --------------------------------------------------------------
SURVIVAL_SHAPE = (3, 96, 160)
SURVIVAL_SEED = 5
QUALITIES = (95, 90, 85, 75, 50)
RULES = ("reference", "nearest", "minmove")
# (label, delta, n_ac, selection): delta = 20 and 40 at n = 10, and delta = 20 on zig-zag scan positions 6 .. 15
SETTINGS = (("20, 10", 20, 10, None), ("40, 10", 40, 10, None), ("20, zigzag:6 x 10", 20, 10, tuple(sl.ZIGZAG[5:15])))


def model_stego(cover, delta, n_ac, payload, rule="reference", index=None):
    """one payload copy per frame, embedded by the oracle (reference rule, the row-major prefix) or by the rule models built on
    it (minmove_lib.model_embed: the nearest and the minimum-move rule, and a selection)"""
    if rule == "reference" and index is None:
        return np.stack([frame_embed(g, delta, payload, n_ac)[1] for g in cover])
    if rule == "reference":
        import coeff_select_lib as cs
        return np.stack([cs.select_embed(g, delta, payload, index)[1] for g in cover])
    return np.stack([ml.model_embed(g, delta, payload, n_ac, minmove=rule == "minmove", index=index)[1] for g in cover])


def read_copies(frames, delta, n_ac, payload, index=None):
    """the model's soft bytes of frames that carry one payload copy each -> dict(single=[bit errors of each copy alone],
    majority=, soft=, share=[lattice_share of each frame])"""
    copies = frames.shape[0]
    soft = sl.model_batch_soft(frames, delta, n_ac, index=index)
    hard = (soft >> 7).reshape(copies, payload.size)
    bits, _ = sv.combine(soft, payload.size)
    return dict(single=[int((b != payload).sum()) for b in hard],
                majority=int(((2 * hard.sum(0) > copies).astype(np.uint8) != payload).sum()),
                soft=int((bits != payload).sum()),
                share=[float(s) for s in sv.lattice_share(sv.byte_histogram(soft, copies))])


def survival(delta, n_ac, index, rule, quality, seed=SURVIVAL_SEED):
    """Three frames of noise in [64, 192), one full-capacity payload copy per frame, through the channel at `quality`.  Fixed
    seed: every number is reproducible."""
    rng = np.random.default_rng(seed)
    f, h, w = SURVIVAL_SHAPE
    cover = rng.integers(64, 192, SURVIVAL_SHAPE).astype(np.uint8)
    payload = rng.integers(0, 2, (h // 8) * (w // 8) * n_ac).astype(np.uint8)
    stego = model_stego(cover, delta, n_ac, payload, rule, index)
    return read_copies(model_requantise(stego, channel.quality_steps(quality)), delta, n_ac, payload, index)
