"""Helpers of the SVS_MINMOVE tests (tests/test_minmove_cpu.py, tests/test_minmove_gpu.py): the NumPy model of the minimum-move
embed - nearest_lib.model_embed with the one assignment changed to the clamp of include/svsdct.h, and the coefficient lookup of
coeff_select_lib.select_embed so that one model serves the prefix and a selection -, the margin table recomputed from its
definition, and the host build of the embed bodies of csrc/svs_block.hpp with the flag (tests/hostemu)."""
import numpy as np

from nearest_lib import content, payload, sse  # noqa: F401  (the content classes and seeds the feature was measured on)
from oracle.qim_dct_oracle import (BLOCK, MAX_AC, _blocks_view, _check_plane, _fwd, _inv, _quant_index, _requantised,
                                   bits_from_any)
from testlib import host_embed_call, hostemu

DELTAS = (8, 20, 40, 7.3, 12.5, 5000.3)       # QM_POW2, QM_F32, QM_F32, QM_DOUBLE, QM_F32, and a QM_DOUBLE step on the exact route
N_ACS = (1, 3, 7, 8, 10, 15, 16, 63)
QM_F32, QM_DOUBLE, QM_POW2 = 0, 1, 2
# (content, n_ac, delta) -> CPU-measured PSNR in dB against the cover: reference, SVS_NEAREST, SVS_MINMOVE (include/svsdct.h)
MEASURED = {("noise", 10, 20): (32.50, 34.90, 39.71), ("noise", 3, 20): (37.62, 39.96, 44.45),
            ("noise", 10, 12): (36.85, 39.18, 41.82), ("noise", 10, 40): (26.53, 28.90, 35.64),
            ("noise", 63, 20): (24.59, 26.97, 32.00), ("noise", 10, 8): (40.22, 42.49, 43.00),
            ("smooth", 10, 20): (32.80, 34.31, 38.39), ("smooth", 63, 20): (25.05, 26.18, 30.25)}


def basis_sums():
    """S_u = sum_x |a_u cos((2 x + 1) u pi / 16)|, a_0 = sqrt(1/8), a_u = 1/2 (float64)"""
    x = np.arange(8)
    return np.array([np.abs((np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)).sum() for u in range(8)])


def margin_table():
    """MARGIN[k] = float32(0.5 * S_u * S_v + 1/16), k = 8 u + v -> float32 [64] (entry 0, the DC position, is never read)"""
    s = basis_sums()
    return np.float32(0.5 * np.outer(s, s).reshape(64) + 0.0625)


def half_cell(delta):
    """h = (float)(0.5 * (double)delta)"""
    return np.float32(0.5 * float(delta))


def band(delta):
    """r_k = fmaxf(0, h - MARGIN[k]) -> float32 [64]"""
    return np.maximum(np.float32(0.0), half_cell(delta) - margin_table())


def noclip_content(delta, h=480, w=640, seed=1):
    """uniform noise that no setting of the tests drives to 0 or 255: [64, 192) at delta = 40, [16, 240) otherwise"""
    lo, hi = (64, 192) if delta >= 40 else (16, 240)
    return np.random.default_rng(seed).integers(lo, hi, (h, w), dtype=np.uint8)


def model_embed(gray, delta, payload, n_ac=MAX_AC, minmove=True, index=None, stats=None):
    """nearest_lib.model_embed (oracle.frame_embed with the nearest rule) with the ONE assignment that writes the coefficient
    changed: c' = min(max(c, c_t - r_k), c_t + r_k) in float32 instead of c_t (include/svsdct.h, SVS_MINMOVE).  index: None
    (coefficients 1..n_ac) or a selection (stream bit i of a block goes to coefficient index[i], as
    coeff_select_lib.select_embed).  minmove=False is the nearest rule itself.  Returns (gray copy, stego uint8, bits
    consumed).  stats (optional dict) receives, per payload coefficient, `c` (before), `new` (after), `ct` (the lattice point),
    `r` (the band) and `k`, and `rec` - the float32 stego before clip and truncate."""
    _check_plane(gray)
    gray = np.ascontiguousarray(gray, np.uint8)
    bits = bits_from_any(payload)
    if index is None:
        index = np.arange(1, max(0, min(int(n_ac), MAX_AC)) + 1)
    index = np.asarray(index, np.int64).reshape(-1)
    n_use = int(index.size)
    h, w = gray.shape
    n_blocks = (h // BLOCK) * (w // BLOCK)
    budget = int(bits.size)
    out_f = np.float32(gray)
    if budget == 0:
        return gray.copy(), gray.copy(), 0
    if delta <= 0 or n_use == 0:
        touched, consumed = n_blocks, 0
    else:
        touched = min(n_blocks, -(-budget // n_use))
        consumed = min(budget, n_blocks * n_use)
    blk = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)[:touched]
    coef = _fwd(blk.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK * BLOCK)
    if consumed:
        use = bits[:consumed].astype(np.int64)
        bi = np.arange(consumed) // n_use
        ki = index[np.arange(consumed) % n_use]
        c = coef[bi, ki]
        q = _quant_index(c, delta)
        wrong = (q & 1) != use
        c0 = _requantised(q, delta)
        step = np.where(c > c0, 1, np.where(c < c0, -1, np.where(use == 1, 1, -1)))
        ct = np.float32(_requantised(np.where(wrong, q + step, q), delta))
        if minmove:
            r = band(delta)[ki]
            new = np.minimum(np.maximum(c, ct - r), ct + r)            # the rule
        else:
            r = np.zeros_like(ct)
            new = ct
        assert new.dtype == np.float32 and c.dtype == np.float32
        coef[bi, ki] = new
        if stats is not None:
            stats.update(c=c.copy(), new=new.copy(), ct=ct, r=r, k=ki)
    rec = _inv(coef.reshape(1, touched, BLOCK, BLOCK)).reshape(touched, BLOCK, BLOCK)
    full = _blocks_view(out_f).reshape(n_blocks, BLOCK, BLOCK)
    full[:touched] = rec
    out_f = full.reshape(h // BLOCK, w // BLOCK, BLOCK, BLOCK).transpose(0, 2, 1, 3).reshape(h, w)
    if stats is not None:
        stats["rec"] = out_f.copy()
    return gray.copy(), np.uint8(np.clip(out_f, 0, 255)), int(consumed)


def model_batch(frames, delta, bits, n_ac, minmove=True, index=None):
    """the frame loop of oracle.batch_embed over model_embed: frame k takes bits [k * cap, (k + 1) * cap) -> (stego, consumed)"""
    bits = bits_from_any(bits)
    out = np.empty_like(frames)
    pos = 0
    for k in range(frames.shape[0]):
        if pos < bits.size:
            _, out[k], used = model_embed(frames[k], delta, bits[pos:], n_ac, minmove, index)
            pos += used
        else:
            out[k] = frames[k]
    return out, pos


def psnr(a, b):
    e = sse(a, b)
    return float("inf") if e == 0 else 10 * np.log10(255.0 ** 2 * a.size / e)


# ---- the embed bodies on the host (tests/hostemu) ---------------------------------------------------------------------
def host_embed(frames, delta, n_ac, bits, bit_offset=0, n_bits=None, pocketfft=False, minmove=True, nearest=False, index=None,
               qm=-1, guard_scale=None, replay_map=False):
    """a gray embed call through the product headers on the host -> (stego, bits embedded, info dict: `replayed` blocks, `path`,
    the plan's `minmove`, `nearest` and `qm`, the rule `word`).  The exact body is the instantiation the plan names (1, 2 or 8
    coefficient rows).  guard_scale: RouteArgs::guard_scale, as SVS_GUARD_SCALE of the experiments library (None: the product's
    guard).  replay_map=True: info gains `replay_map`, bool per block of the call in raster order - the guard handed the block
    to the exact replay."""
    out, res, rmap = host_embed_call(frames, delta, n_ac, bits, bit_offset=bit_offset, n_bits=n_bits, index=index,
                                     pocketfft=pocketfft, guarded=not pocketfft, nearest=int(nearest), minmove=int(minmove),
                                     force_qm=int(qm), exact_rows=0, guard_scale=1.0 if guard_scale is None else float(guard_scale))
    info = dict(replayed=int(res.replayed), path=int(res.path), minmove=int(res.minmove), nearest=int(res.nearest), qm=int(res.qm),
                word=int(res.word))
    if replay_map:
        info["replay_map"] = rmap
    return out, int(res.used), info


def plan(delta, n_ac, total, n_bits, pocketfft=False, bgr=False, minmove=True, nearest=False):
    """-> (path, minmove, use, half_cell as float32, rule word) of csrc/svs_route.hpp plan_embed"""
    out = np.zeros(6, np.int64)
    hostemu().emu_plan_rule(float(delta), int(n_ac), int(total), int(n_bits), int(pocketfft), int(bgr), int(nearest), int(minmove),
                            out.ctypes.data)
    return int(out[0]), int(out[2]), int(out[3]), np.array([out[4]], np.uint32).view(np.float32)[0], int(out[5])

