"""Batched embed / extract over stacks of gray frames - the frame loops of the reference
(embed_process.py:108-128, extract_process.py:55-86,173-182) turned into one kernel launch per
batch.  Frame k of a batch takes stream bits [k*cap, (k+1)*cap) (cap = blocks per frame * n_ac);
the extracted stream is the frames' bits in order.

Two levels:
  * `embed_frames` / `extract_frames`      NumPy in, NumPy out (host entry points of the C ABI).
  * `embed_device` / `extract_device`      raw device pointers + stream (what bench.py and a
                                           device-resident pipeline use); nothing is copied.
  * `extract_soft_frames` / `extract_soft_device`   the same two levels of the soft-decision extraction: a byte per bit.
  * `embed_repeated_frames`, `extract_vote_frames` / `extract_vote_device`   a payload tiled through the stream, and the
                                           fused soft vote that folds its copies on the device: `period` integers come back.
  * `extract_histogram_frames` / `extract_histogram_device`   the fused per-frame soft histograms: 256 counts a frame come back.
  * `embed_coded_frames` / `extract_coded_frames`   a payload under the convolutional code of svsdct/fec.py: the soft bytes (or the
                                           tally of its copies) stay on the device and feed the Viterbi decoder; the payload comes back.
Bits travel packed MSB-first (numpy.packbits order), so `unpack_to_str` of the extract output is
the reference operator's '0'/'1' string.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import channel as _channel
from . import coeffs as _coeffs
from . import dither as _dither
from . import enc as _enc
from . import fec as _fec
from . import native
from . import matrix as _matrix
from . import rs as _rs
from . import rse as _rse
from . import steps as _steps
from . import soft as _soft
from .hostmem import pinned_empty
from .native import BlockOrder, Dither, Planes
from .order import check_key
from .staging import Staged

MAX_AC = 63

# Transform mode (include/svsdct.h `flags`).  Every mode produces the reference's stego pixels and bits; the modes only
# differ in which kernels get there:
#   "guarded" n_ac <= 15 and 0.25 <= delta <= 4096: the streaming kernel (cheap sparse transform wherever a rigorous bound
#            on the reference's float32 round-trip noise proves it equals the reference's truncation, the pocketfft-identical
#            arithmetic inside the same launch for the blocks where it cannot; 8 tests per block at n_ac <= 7, 64 at
#            n_ac = 8..15); otherwise the "exact" kernels.  Extraction: n_ac <= 7 the pocketfft-identical forward, n_ac >= 8 the
#            FMA-factored forward with a proven per-block tie margin (the reference's bits for any input).
#   "fast"   flags = 0 of the C ABI: the same launches as "guarded" (kept for ABI compatibility).
#   "exact"  pocketfft-identical arithmetic on every block, one lane per block - the yardstick (VALU-bound).
# DEFAULT_MODE is THE product default: every entry point of this module, FramePipeline, the drop-in operator, both drop-in
# video loops and bench.py resolve an unspecified mode through resolve_mode() - nothing else chooses one
# (tests/test_capi_cpu.py::test_one_default_mode_everywhere).  The Python layer (not the shared library) lets
# SVS_DCT_MODE=fast|exact|guarded override it for a whole process.
DEFAULT_MODE = "guarded"
_MODE_FLAGS = {"fast": 0, "exact": native.SVS_EXACT_POCKETFFT, "guarded": native.SVS_EXACT_GUARDED}
_ENV_MODE = os.environ.get("SVS_DCT_MODE")


def resolve_mode(mode: str | None = None) -> str:
    """explicit argument > SVS_DCT_MODE > DEFAULT_MODE"""
    mode = mode or _ENV_MODE or DEFAULT_MODE
    if mode not in _MODE_FLAGS:
        raise ValueError(f"unknown transform mode {mode!r} (use 'fast', 'exact' or 'guarded')")
    return mode


def mode_flags(mode: str | None = None) -> int:
    """`flags` word of the C ABI for a transform mode (None = the product default)"""
    return _MODE_FLAGS[resolve_mode(mode)]


def embed_flags(mode: str | None = None, nearest: bool = False, minmove: bool = False) -> int:
    """`flags` word of an embed call: the transform mode, plus SVS_NEAREST and SVS_MINMOVE (include/svsdct.h) when asked for"""
    return mode_flags(mode) | (native.SVS_NEAREST if nearest else 0) | (native.SVS_MINMOVE if minmove else 0)


def host_level_mode() -> str:
    """transform mode of the drop-in operator and video pipelines: the product default"""
    return resolve_mode(None)


def clamp_ac(n_ac) -> int:
    return max(0, min(int(n_ac), MAX_AC))  # config_and_setup.py:138


def capacity_bits(n_frames: int, height: int, width: int, n_ac) -> int:
    return n_frames * (height // 8) * (width // 8) * clamp_ac(n_ac)


# ---- payload forms --------------------------------------------------------------------------
def str_to_bits(payload: str, limit: int | None = None) -> np.ndarray:
    """'0101...' -> uint8 0/1 array (vectorised; only the first `limit` characters are touched)."""
    if limit is not None:
        payload = payload[:limit]
    return np.frombuffer(payload.encode("ascii"), np.uint8) - np.uint8(48)


def bits_to_str(bits: np.ndarray) -> str:
    return (np.asarray(bits, np.uint8) + np.uint8(48)).tobytes().decode("ascii")


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """0/1 array -> MSB-first packed bytes, zero padded to a multiple of 4 bytes (the C ABI reads
    the payload as aligned dwords)."""
    packed = np.packbits(np.asarray(bits, np.uint8))
    pad = (-packed.size) % 4
    if pad or packed.size == 0:
        packed = np.concatenate([packed, np.zeros(pad if packed.size else 4, np.uint8)])
    return packed


def _pack_window(bits: np.ndarray, bit_offset: int, n_bits: int):
    """Pack only the part of a long 0/1 stream one call reads: -> (packed bytes, bit offset rebased onto them).
    A frame loop that walks one stream by bit offset then packs O(batch) bits per call, not O(stream)."""
    start = (int(bit_offset) // 32) * 32
    return pack_bits(bits[start:int(bit_offset) + int(n_bits)]), int(bit_offset) - start


def unpack_to_str(packed: np.ndarray, n_bits: int) -> str:
    return bits_to_str(np.unpackbits(np.asarray(packed, np.uint8), count=n_bits))


# ---- host-array level -----------------------------------------------------------------------
def _as_stack(frames: np.ndarray) -> np.ndarray:
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise TypeError("frames must be uint8")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("frames must be [H,W] or [F,H,W] gray planes")
    if a.shape[1] % 8 or a.shape[2] % 8:
        raise ValueError("frame height and width must be multiples of 8")
    return np.ascontiguousarray(a)


def block_order(key, first_frame: int = 0) -> BlockOrder | None:
    """the C ABI's svs_block_order for a block key (None: no order); raises unless 0 <= key < 2**64 and
    0 <= first_frame < 2**32"""
    if key is None:
        return None
    first_frame = int(first_frame)
    if not 0 <= first_frame < (1 << 32):
        raise ValueError(f"first_frame {first_frame} outside 0 .. 2**32 - 1")
    return BlockOrder(check_key(key), first_frame, 0)


def _ref(struct):
    """a pointer to an optional struct argument (svs_block_order, svs_coeffs, svs_dither), NULL for None"""
    return C.byref(struct) if struct is not None else None


def _no_coeffs(coeffs):
    if coeffs is not None:
        raise ValueError("a coefficient selection has no colour form: convert to gray and use the gray calls")


def dither_arg(dither_key, first_frame: int = 0, readback: bool = False) -> Dither | None:
    """the C ABI's svs_dither for a dither key (None: no dither); raises unless 0 <= key < 2**64 and 0 <= first_frame < 2**32,
    and with readback (the dithered call with read-back is readback_keyed's)"""
    if dither_key is None:
        return None
    key = _dither.check_key(dither_key)
    if readback:
        raise ValueError("a keyed dither has no read-back form under readback=True: use readback_keyed=True")
    first_frame = int(first_frame)
    if not 0 <= first_frame < (1 << 32):
        raise ValueError(f"first_frame {first_frame} outside 0 .. 2**32 - 1")
    return Dither(key, first_frame, 0)


def no_dither(dither_key, what: str) -> None:
    """the colour and _str calls: a dither key is refused before the library is loaded"""
    if dither_key is not None:
        raise ValueError(f"a keyed dither has no {what} form: use the gray calls with packed bits")


def _one_readback(readback, readback_keyed):
    """one switch per path: readback is SVS_READBACK's, readback_keyed svs_embed_dithered_readback*'s"""
    if readback and readback_keyed:
        raise ValueError("readback and readback_keyed are two paths: set one of them")


class ReadbackCounts(NamedTuple):
    """what an SVS_READBACK embed did: blocks that did not read back and were repaired / kept the reference's bytes"""
    repaired: int
    unrepaired: int


class MarginCounts(NamedTuple):
    """what a readback_margin embed did: the read-back's two counts, then the margin pass's - blocks that decoded with a weak
    coefficient and were strengthened / kept the read-back's bytes (svs_stepped_embed_readback_margin, include/svsdct.h)"""
    repaired: int
    unrepaired: int
    strengthened: int
    weak: int


class _GrayCall(NamedTuple):
    """the gray keywords of a call, resolved: the structs it adds to the plain call and the entry points that take them"""
    order: BlockOrder | None
    sel: native.Coeffs | None
    dith: Dither | None
    stem: str               # key of _GRAY_CALLS


# C symbol stem (svs_embed<stem>[_dev], svs_extract<stem>[_dev]) -> (the struct pointers that lead its argument list behind
# the planes, takes n_ac, takes counts)
_GRAY_CALLS = {
    "": ((), True, False),
    "_ordered": (("order",), True, False),
    "_select": (("order", "sel"), False, False),
    "_dithered": (("order", "sel", "dith"), True, False),
    "_readback": (("order",), True, True),
    "_dithered_readback": (("order", "sel", "dith"), True, True),
}


def _resolve(n_ac, order=None, block_key=None, first_frame=None, coeffs=None, dither_key=None, readback=False,
             readback_keyed=False) -> _GrayCall:
    """The gray keywords -> the call they make; every ValueError they can cause is raised here, before the library is loaded.
    order: a BlockOrder, or block_key and first_frame to make one of.  coeffs: a spec string ("zigzag", "zigzag:6",
    "rowmajor") resolves with the call's n_ac, an explicit list must have len == n_ac (svsdct/coeffs.py).  The dither shares
    first_frame, by default the order's (0 without one).  readback_keyed with neither a selection nor a dither is readback."""
    _one_readback(readback, readback_keyed)
    if block_key is not None:
        order = block_order(block_key, first_frame)
    sel = _coeffs.selection(coeffs, clamp_ac(n_ac))
    if sel is not None:
        if readback:
            raise ValueError("a coefficient selection has no read-back form under readback=True: use readback_keyed=True")
        sel = _coeffs.native_coeffs(sel)
    if first_frame is None:
        first_frame = int(order.first_frame) if order is not None else 0
    dith = dither_arg(dither_key, first_frame, readback)
    if readback_keyed and (sel is not None or dith is not None):
        stem = "_dithered_readback"
    elif dith is not None:
        stem = "_dithered"
    elif readback or readback_keyed:
        stem = "_readback"
    elif sel is not None:
        stem = "_select"
    else:
        stem = "_ordered" if order is not None else ""
    return _GrayCall(order, sel, dith, stem)


def _gray_call(lib, verb, call: _GrayCall, front, delta, n_ac, back, counts=None, stream=()) -> None:
    """svs_<verb><stem>(*front, <the stem's struct pointers>, delta, [n_ac], *back, [counts]), or with stream = (handle,) its
    _dev form with the stream last; raises unless it returns SVS_OK"""
    structs, takes_n_ac, takes_counts = _GRAY_CALLS[call.stem]
    name = f"svs_{verb}{call.stem}" + ("_dev" if stream else "")
    args = [*front, *(_ref(getattr(call, s)) for s in structs), float(delta), *([int(n_ac)] if takes_n_ac else ()), *back,
            *([counts] if takes_counts else ()), *stream]
    native.check(getattr(lib, name)(*args), name)


def _steps_arg(steps, readback=False, readback_keyed=False):
    """steps= of the gray calls -> struct svs_qim_steps, None for None; every ValueError it can cause is raised here, before the
    library is loaded (steps with readback / readback_keyed is refused: the stepped read-back is readback_stepped's path)"""
    if steps is None:
        return None
    if readback or readback_keyed:
        raise ValueError("per-coefficient steps have no read-back form: drop readback / readback_keyed or steps")
    return _steps.steps_struct(steps)


def _readback_stepped_arg(readback_stepped, steps, readback=False, readback_keyed=False) -> bool:
    """one switch per path: readback_stepped is svs_stepped_embed_readback*'s.  It needs steps and excludes the two other
    read-back switches; raised before the library is loaded (and before _steps_arg's own refusal, which names the pair it
    refuses: steps with readback / readback_keyed stays refused without this switch)."""
    if not readback_stepped:
        return False
    if readback or readback_keyed:
        raise ValueError("readback_stepped is a path of its own: drop readback / readback_keyed")
    if steps is None:
        raise ValueError("readback_stepped needs steps: the read-back of a call without them is readback / readback_keyed")
    return True


def _readback_margin_arg(readback_margin, steps, readback=False, readback_keyed=False) -> int:
    """readback_margin=g of the gray embeds -> the gate, 0 for None.  An int 1..127; it implies readback_stepped, so it needs
    steps and refuses readback / readback_keyed as that switch does; raised before the library is loaded."""
    if readback_margin is None:
        return 0
    if isinstance(readback_margin, bool) or not isinstance(readback_margin, (int, np.integer)) or not 1 <= int(readback_margin) <= 127:
        raise ValueError("readback_margin is an int in 1..127: the smallest soft margin m a payload coefficient may be left with")
    _readback_stepped_arg(True, steps, readback, readback_keyed)
    return int(readback_margin)


def _matrix_arg(matrix, steps, *readbacks):
    """matrix= of the gray calls (k, or (k, "pair"): svsdct/matrix.py) -> struct svs_matrix, None for None.  It needs steps and has
    no read-back form; every ValueError it can cause is raised here, before the library is loaded."""
    if matrix is None:
        return None
    k, search = _matrix.as_pair(matrix)
    if steps is None:
        raise ValueError("matrix needs steps: a matrix call is a stepped call (steps.uniform(delta) for one delta)")
    if any(readbacks):
        raise ValueError("matrix embedding has no read-back form: drop the read-back switch or matrix")
    return _matrix.matrix_struct(k, search)


def _no_matrix(matrix, what: str) -> None:
    if matrix is not None:
        raise ValueError(f"matrix embedding has no {what} form")


def _stepped_call(lib, verb, call: _GrayCall, steps, front, n_ac, back, stream=(), counts=(), matrix=None) -> None:
    """svs_stepped_<verb>(*front, order, coeffs, dither, steps, n_ac, *back), or with stream = (handle,) its _dev form with the
    stream last; raises unless it returns SVS_OK.  The call's delta is not an argument: the table replaces it.  counts =
    (pointer,): the counts argument of the read-back forms (verbs "embed_readback" and "embed_readback_margin", whose `back`
    carries the gate in front of the flags), behind `back`.  matrix (a struct of _matrix_arg; verbs "embed" and "extract"):
    svs_matrix_<verb>, the same call with the struct behind the table."""
    name = (f"svs_stepped_{verb}" if matrix is None else f"svs_matrix_{verb}") + ("_dev" if stream else "")
    args = [*front, _ref(call.order), _ref(call.sel), _ref(call.dith), C.byref(steps), *(() if matrix is None else (C.byref(matrix),)),
            int(n_ac), *back, *counts, *stream]
    native.check(getattr(lib, name)(*args), name)


def embed_frames(frames: np.ndarray, delta, n_ac, bits, bit_offset: int = 0, n_bits: int | None = None,
                 device: int = 0, mode: str | None = None, block_key=None, first_frame: int = 0, readback: bool = False,
                 nearest: bool = False, coeffs=None, minmove: bool = False, dither_key=None, readback_keyed: bool = False,
                 steps=None, readback_stepped: bool = False, readback_margin: int | None = None, matrix=None):
    """Embed a bit stream into a stack of gray frames on the GPU.

    frames : uint8 [F,H,W] (or [H,W]);  bits : 0/1 array or '0'/'1' str (the stream; bit
    `bit_offset` is the first one used);  n_bits : bits available from bit_offset (default: rest).
    block_key : None (the reference's raster order) or an integer key 0 <= key < 2**64: the blocks of each frame take the
    frame's bits in a keyed order (svsdct/order.py); frame f of the stack is clip frame first_frame + f.
    readback : opt-in (SVS_READBACK, include/svsdct.h): every block that carries payload is read back with the reference's
    extraction and repaired where the reference's clipping or truncation lost a bit; repaired blocks are not the reference's
    pixels any more.
    minmove : opt-in (SVS_MINMOVE, include/svsdct.h): a payload coefficient moves only as far as the decision cell of its
    index asks (less a margin that covers the truncation of the stego pixels) and stays where it is when it is already
    there - 4 to 7 dB more PSNR at delta >= 12, the same receiver; the stego pixels are neither the reference's nor the nearest
    rule's.  Implies the nearest direction.  Blocks that clip at 0 / 255 are outside its guarantee: combine with readback.
    nearest : opt-in (SVS_NEAREST, include/svsdct.h): a coefficient whose parity has to change moves to the nearer of its two
    neighbouring lattice points instead of the reference's fixed direction - about 2 dB more PSNR, the same receiver; the
    stego pixels are not the reference's any more.
    coeffs : None (the reference's row-major coefficients 1..n_ac) or a payload coefficient selection (svsdct/coeffs.py:
    "zigzag", "zigzag:<first>", "rowmajor" or a list of n_ac distinct flat indices in 1..63): stream bit i of a block goes
    to coefficient index[i].  It combines with block_key, first_frame, nearest and mode (any selection but the prefix runs
    the exact kernels in every mode); ValueError with readback.  The receiver must use the same selection.
    dither_key : None or an integer key 0 <= key < 2**64 (opt-in, svsdct/dither.py, include/svsdct.h): the quantiser lattice
    of every payload coefficient is shifted by a key-derived offset - no comb in the coefficient histogram, no bits for a
    receiver without the key, no distortion cost.  It shares first_frame with block_key and combines with block_key, coeffs,
    nearest, minmove and mode (a dithered call runs the exact kernels in every mode); ValueError with readback.  The receiver
    must use the same key.
    readback_keyed : opt-in (svs_embed_dithered_readback, include/svsdct.h): the read-back and repair under coeffs and / or
    dither_key - every payload block is read back with the selected / dithered extraction's own verdict and repaired where it
    fails.  With neither it makes the readback call.  ValueError together with readback.
    steps : None, or a table of 64 per-coefficient QIM steps (opt-in, svsdct/steps.py: steps.matched(75), steps.uniform(20);
    svs_stepped_embed, include/svsdct.h): coefficient k is quantised with steps[k] and the call's delta is not used.  It
    combines with block_key, coeffs, dither_key, nearest and minmove and runs the exact kernels in every mode; ValueError with
    readback or readback_keyed: its read-back form is readback_stepped.  The receiver must use the same table.
    readback_stepped : opt-in (svs_stepped_embed_readback, include/svsdct.h): the read-back and repair under steps - every
    payload block is read back with the stepped extraction's own verdict and repaired where it fails.  It needs steps and
    combines with block_key, coeffs, dither_key, nearest, minmove and first_frame; ValueError with readback or readback_keyed.
    readback_margin : None, or an int g in 1..127 (opt-in, svs_stepped_embed_readback_margin, include/svsdct.h): after the
    stepped read-back a second pass strengthens every block that decodes but would reach the receiver with a soft margin m < g
    on some payload coefficient.  It implies readback_stepped: it needs steps; ValueError with readback or readback_keyed.
    matrix : None, k or (k, "pair") (opt-in, svsdct/matrix.py; svs_matrix_embed, include/svsdct.h): matrix embedding - a block
    carries k bits as the Hamming syndrome of the parities of its 2^k - 1 payload coefficients, so at most one of them (with
    "pair": the cheaper of one or two) changes parity.  It needs steps, a selection (or n_ac) of exactly 2^k - 1 coefficients,
    and pays off under minmove; the capacity is blocks * k.  ValueError without steps or with any read-back switch.
    Returns (stego uint8 [F,H,W], n_embedded), with readback, readback_keyed or readback_stepped (stego, n_embedded,
    ReadbackCounts), with readback_margin (stego, n_embedded, MarginCounts)."""
    mx = _matrix_arg(matrix, steps, readback, readback_keyed, readback_stepped, readback_margin)
    gate = _readback_margin_arg(readback_margin, steps, readback, readback_keyed)
    stepped_rb = _readback_stepped_arg(readback_stepped, steps, readback, readback_keyed)
    table = _steps_arg(steps, readback, readback_keyed)
    call = _resolve(n_ac, None, block_key, first_frame, coeffs, dither_key, readback, readback_keyed)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    if isinstance(bits, str):
        bits = str_to_bits(bits)
    bits = np.asarray(bits, np.uint8)
    if n_bits is None:
        n_bits = max(0, bits.size - bit_offset)
    if bit_offset + n_bits > bits.size:
        raise ValueError("bit_offset + n_bits exceeds the payload length")
    packed, bit_offset = _pack_window(bits, bit_offset, n_bits)
    stego = pinned_empty(stack.shape)      # page-locked: the download lands in it by DMA, no staging copy, no page faults
    done = C.c_uint64(0)
    planes = Planes.contiguous(f, h, w)
    counts = native.ReadbackCounts()
    if gate:
        four = native.MarginCounts()
        _stepped_call(lib, "embed_readback_margin", call, table, [stack.ctypes.data, stego.ctypes.data, C.byref(planes)], n_ac,
                      [packed.ctypes.data, int(bit_offset), int(n_bits), gate, embed_flags(mode, nearest, minmove), C.byref(done)],
                      counts=(C.byref(four),))
        return stego, int(done.value), MarginCounts(int(four.repaired), int(four.unrepaired), int(four.strengthened), int(four.weak))
    if table is not None:
        _stepped_call(lib, "embed_readback" if stepped_rb else "embed", call, table,
                      [stack.ctypes.data, stego.ctypes.data, C.byref(planes)], n_ac,
                      [packed.ctypes.data, int(bit_offset), int(n_bits), embed_flags(mode, nearest, minmove), C.byref(done)],
                      counts=(C.byref(counts),) if stepped_rb else (), matrix=mx)
        if stepped_rb:
            return stego, int(done.value), ReadbackCounts(int(counts.repaired), int(counts.unrepaired))
        return stego, int(done.value)
    _gray_call(lib, "embed", call, [stack.ctypes.data, stego.ctypes.data, C.byref(planes)], delta, n_ac,
               [packed.ctypes.data, int(bit_offset), int(n_bits), embed_flags(mode, nearest, minmove), C.byref(done)],
               C.byref(counts))
    if _GRAY_CALLS[call.stem][2]:
        return stego, int(done.value), ReadbackCounts(int(counts.repaired), int(counts.unrepaired))
    return stego, int(done.value)


def extract_frames(frames: np.ndarray, delta, n_ac, device: int = 0, mode: str | None = None, block_key=None,
                   first_frame: int = 0, coeffs=None, dither_key=None, steps=None, matrix=None):
    """Extract the packed bit stream of a stack of gray frames on the GPU.  block_key / first_frame: as embed_frames (the
    sender's key and clip frame index).  coeffs: as embed_frames (the sender's selection).  dither_key: as embed_frames (the
    sender's dither key).  steps: as embed_frames (the sender's step table; delta is then not used).  matrix: as embed_frames
    (the sender's k; svs_matrix_extract: k bits a block, n_bits = blocks * k; "pair" reads as k).
    Returns (packed uint8 [ceil(n_bits/8)], n_bits)."""
    mx = _matrix_arg(matrix, steps)
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, block_key, first_frame, coeffs, dither_key)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    cap = capacity_bits(f, h, w, n_ac) if mx is None else _matrix.capacity_bits(f, h, w, mx.k)
    out = np.zeros(max(4, (cap + 7) // 8 + (-((cap + 7) // 8)) % 4), np.uint8)
    got = C.c_uint64(0)
    planes = Planes.contiguous(f, h, w)
    back = [out.ctypes.data, out.size, mode_flags(mode), C.byref(got)]
    if table is not None:
        _stepped_call(lib, "extract", call, table, [stack.ctypes.data, C.byref(planes)], n_ac, back, matrix=mx)
    else:
        _gray_call(lib, "extract", call, [stack.ctypes.data, C.byref(planes)], delta, n_ac, back)
    n = int(got.value)
    return out[: (n + 7) // 8], n


# svs_soft_<name>[_dev] -> (takes an order, its arguments between n_ac and flags)
_SOFT_CALLS = {
    "extract": (True, ("out", "out_capacity_bytes")),
    "vote": (True, ("period", "stream_bit0", "tally")),
    "histogram": (False, ("hist",)),
}


def _soft_call(lib, name, call: _GrayCall, front, delta, n_ac, middle, flags, stream=(), steps=None) -> int:
    """svs_soft_<name>(*front, [order], coeffs, dither, delta, n_ac, *middle, flags, n_bits_out), or with stream = (handle,) its
    _dev form; -> n_bits_out.  A soft entry point takes each of its structs or NULL, so every stem of _resolve makes the same
    call; raises unless it returns SVS_OK.  steps (a struct of _steps_arg): svs_stepped_soft_<name>, the same call with the
    table in the place of delta."""
    takes_order, names = _SOFT_CALLS[name]
    assert len(middle) == len(names), names
    symbol = ("svs_soft_" if steps is None else "svs_stepped_soft_") + name + ("_dev" if stream else "")
    got = C.c_uint64(0)
    native.check(getattr(lib, symbol)(*front, *([_ref(call.order)] if takes_order else ()), _ref(call.sel), _ref(call.dith),
                                      float(delta) if steps is None else C.byref(steps), int(n_ac), *middle, flags, C.byref(got),
                                      *stream), symbol)
    return int(got.value)


def extract_soft_frames(frames: np.ndarray, delta, n_ac, device: int = 0, mode: str | None = None, block_key=None,
                        first_frame=None, coeffs=None, dither_key=None, steps=None, matrix=None):
    """Soft-decision extraction of a stack of gray frames on the GPU (svs_soft_extract, include/svsdct.h): one byte per
    capacity bit in stream order - bit 7 the hard bit extract_frames returns, bits 0..6 the distance of the coefficient from
    the nearest decision boundary in units of delta / 254 (svsdct/soft.py reads and combines them).  block_key, first_frame,
    coeffs, dither_key: as extract_frames; mode is accepted and changes nothing (a soft call always runs the exact kernel).
    steps: as extract_frames (svs_stepped_soft_extract: the sender's step table; delta is then not used, and the distance of
    coefficient k is in units of steps[k] / 254, its own cell).
    Returns (soft uint8 [capacity], n_bits).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no soft form."""
    _no_matrix(matrix, "soft")
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, block_key, 0 if first_frame is None else first_frame, coeffs, dither_key)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    cap = capacity_bits(f, h, w, n_ac)
    out = pinned_empty(max(4, cap))
    planes = Planes.contiguous(f, h, w)
    n = _soft_call(lib, "extract", call, [stack.ctypes.data, C.byref(planes)], delta, n_ac, [out.ctypes.data, cap], mode_flags(mode),
                   steps=table)
    return out[:n], n


def _period(period) -> int:
    period = int(period)
    if not 1 <= period < 1 << 61:
        raise ValueError(f"period {period} outside 1 .. 2**61 - 1")
    return period


def extract_vote_frames(frames: np.ndarray, delta, n_ac, period, stream_bit0: int = 0, device: int = 0, mode: str | None = None,
                        block_key=None, first_frame=None, coeffs=None, dither_key=None, steps=None, matrix=None):
    """Fused soft vote over a stack of gray frames on the GPU (svs_soft_vote, include/svsdct.h): the soft bytes of
    extract_soft_frames are never written - the kernel adds each into a tally of `period` int32 values at its stream position
    (stream_bit0 + its index) mod period, and only the tally comes back.  period: the payload's length in bits, as the sender
    tiled it (embed_repeated_frames).  stream_bit0: the capacity of the frames before this stack when a clip is read in
    batches - add the tallies of the batches and read the bits with soft.tally_bits.  The other keywords: as
    extract_soft_frames (steps: svs_stepped_soft_vote).  Returns (bits uint8 [period], tally int32 [period]); the bits are
    soft.combine's.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no vote form."""
    _no_matrix(matrix, "vote")
    period = _period(period)
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, block_key, 0 if first_frame is None else first_frame, coeffs, dither_key)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    tally = pinned_empty(4 * period).view(np.int32)
    planes = Planes.contiguous(f, h, w)
    _soft_call(lib, "vote", call, [stack.ctypes.data, C.byref(planes)], delta, n_ac, [period, int(stream_bit0), tally.ctypes.data],
               mode_flags(mode), steps=table)
    return _soft.tally_bits(tally), tally


def extract_histogram_frames(frames: np.ndarray, delta, n_ac, device: int = 0, mode: str | None = None, first_frame=None,
                             coeffs=None, dither_key=None, steps=None, matrix=None):
    """Fused per-frame soft histograms of a stack of gray frames on the GPU (svs_soft_histogram, include/svsdct.h): the soft
    bytes of extract_soft_frames are never written - the kernel counts each into row `frame`, column `byte` of 256 counts a
    frame, and only the rows come back (soft.byte_histogram is the model; soft.margins and soft.lattice_share read them).
    There is no block_key keyword and none is needed: the dither is keyed to a block's physical position and an order only
    permutes the blocks inside a frame, so a frame's counts are the same under every order - frames embedded under a block_key
    are read with this same call.  first_frame, coeffs, dither_key, steps: as extract_soft_frames (steps: svs_stepped_soft_histogram);
    mode is accepted and changes nothing.  Returns (hist uint32 [n_frames, 256], n_bits).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no histogram form."""
    _no_matrix(matrix, "histogram")
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, None, 0 if first_frame is None else first_frame, coeffs, dither_key)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    hist = pinned_empty(max(4, 1024 * f))[: 1024 * f].view(np.uint32).reshape(f, 256)
    planes = Planes.contiguous(f, h, w)
    return hist, _soft_call(lib, "histogram", call, [stack.ctypes.data, C.byref(planes)], delta, n_ac, [hist.ctypes.data], mode_flags(mode),
                            steps=table)


def embed_repeated_frames(frames: np.ndarray, delta, n_ac, bits, copies: int | None = None, **embed_kw):
    """Embed a payload more than once: soft.tile(bits, copies * len(bits)) - copy after copy, copies=None: as many as the
    stack's capacity holds, the last one cut where it ends - through embed_frames, which takes every other keyword.  There is
    no embed kernel path of its own: the tiled stream is an eighth of a byte per capacity bit.
    Returns (stego, used, period), and the ReadbackCounts or MarginCounts behind them where embed_frames returns them; period = len(bits) is
    what the receiver passes to extract_vote_frames."""
    if isinstance(bits, str):
        bits = str_to_bits(bits)
    bits = np.asarray(bits, np.uint8)
    if "bit_offset" in embed_kw or "n_bits" in embed_kw:
        raise ValueError("embed_repeated_frames embeds the whole tiled stream: bit_offset and n_bits are not its keywords")
    f, h, w = _as_stack(frames).shape
    cap = capacity_bits(f, h, w, n_ac)      # a selection lists n_ac coefficients
    if embed_kw.get("matrix") is not None:  # a matrix call carries k bits a block
        cap = _matrix.capacity_bits(f, h, w, _matrix.as_pair(embed_kw["matrix"])[0])
    if copies is not None and int(copies) < 1:
        raise ValueError("copies must be at least 1")
    stream = _soft.tile(bits, cap if copies is None else min(cap, int(copies) * bits.size))
    stego, used, *counts = embed_frames(frames, delta, n_ac, stream, **embed_kw)
    return (stego, used, int(bits.size), *counts)


def _coded_copies(copies):
    if copies is not None and (isinstance(copies, bool) or int(copies) < 1):
        raise ValueError("copies must be at least 1 (None: as many as the capacity holds)")
    return None if copies is None else int(copies)


def _outer_bytes(n_bits: int) -> int:
    if n_bits % 8:
        raise ValueError(f"outer=True: the outer code takes whole bytes, {n_bits} payload bits are not")
    return n_bits // 8


def _lost_frames_arg(lost_frames, erase_margin, outer, copies):
    """(sorted frame indices, margin) of extract_coded_frames' lost_frames; the upper bound is checked where the stack is known"""
    lost = []
    for i in lost_frames:
        if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)):
            raise ValueError(f"lost_frames: {i!r} is no frame index")
        if i < 0:
            raise ValueError(f"lost_frames: frame {i} is outside the stack")
        lost.append(int(i))
    if isinstance(erase_margin, (bool, np.bool_)) or not isinstance(erase_margin, (int, np.integer)) or erase_margin < 0:
        raise ValueError("erase_margin is a number of bytes, 0 or more")
    if lost and not outer:
        raise ValueError("lost_frames needs outer=True: it is the Reed-Solomon decoder that takes erasures")
    if lost and copies != 1:
        raise ValueError("lost_frames needs copies = 1: a tally of copies has no stream range per frame")
    return sorted(set(lost)), int(erase_margin)


def lost_span(lo: int, hi: int, rate: int, k: int, erase_margin: int = 1):
    """[lo, hi) in sent bits of the coded stream -> the [lo, hi) byte range of the Reed-Solomon stream of k data bytes that they
    bear on: the trellis steps (fec.steps_of_sent_bits; payload bit t of the inner code is step t, and its payload IS the
    Reed-Solomon stream) divided by 8, clipped to the stream - the six tail steps fall away - and widened by erase_margin bytes"""
    total = _rs.coded_bytes(k)
    t0, t1 = _fec.steps_of_sent_bits(lo, hi, rate)
    return max(min(t0 // 8, total) - erase_margin, 0), min(min(-(-t1 // 8), total) + erase_margin, total)


def _round4(nbytes: int) -> int:
    return (int(nbytes) + 3) // 4 * 4


class _CodedPlan(NamedTuple):
    """The lengths of a coded stream in a stack of `capacity` bits, and where embed_coded_device puts each stage in its workspace
    (byte offsets, each stage rounded up to 4 bytes): the one place that knows them, for both ends of the chain."""
    capacity: int
    k: int            # the data bytes of the outer code, 0 without it
    inner: int        # the info bits of the inner code: the payload, or the bits of the Reed-Solomon stream
    coded: int        # its coded (sent) bits
    stream: int       # the bits that are embedded: one copy, or the copies cut at the capacity
    at_coded: int     # the Reed-Solomon stream, if there is one, lies at 0
    at_stream: int    # = at_coded when copies is 1: the coded stream is what is embedded
    work_bytes: int

    @classmethod
    def of(cls, n_info: int, rate: int, copies, outer: bool, capacity: int) -> "_CodedPlan":
        """copies: as _coded_copies returns it.  Raises the ValueErrors about a payload that is not whole bytes under outer, a
        rate that is none, and a coded stream above the capacity - in that order."""
        n_info, cap = int(n_info), int(capacity)
        k = _outer_bytes(n_info) if outer else 0
        inner = 8 * _rs.coded_bytes(k) if outer else n_info
        coded = _fec.coded_bits(inner, rate)
        if coded > cap:
            raise ValueError(f"{coded} coded bits exceed the capacity of {cap}: at rate code {rate} it holds "
                             f"{_rs.payload_bits(cap, rate) if outer else _fec.info_bits(cap, rate)} payload bits")
        stream = coded if copies == 1 else cap if copies is None else min(cap, copies * coded)
        at_coded = _round4(_rs.coded_bytes(k)) if outer else 0
        at_stream = at_coded if copies == 1 else at_coded + _round4((coded + 7) // 8)
        return cls(cap, k, inner, coded, stream, at_coded, at_stream, at_stream + _round4((stream + 7) // 8))


def coded_workspace_bytes(n_info: int, rate: int = 2, copies: int | None = 1, outer: bool = False, capacity: int = 0) -> int:
    """The bytes of d_work that embed_coded_device needs for a payload of n_info bits in a stack of `capacity` bits
    (capacity_bits): the Reed-Solomon stream under outer, the coded stream, and the tiled stream unless copies is 1 - each
    rounded up to 4 bytes.  Raises embed_coded_frames' ValueErrors."""
    return _CodedPlan.of(n_info, rate, _coded_copies(copies), outer, capacity).work_bytes


def _embed_coded_on_device(frames, delta, n_ac, info, rate, copies, outer, embed_kw):
    """embed_coded_frames(encoder="device"): the packed payload and the frames go up, embed_coded_device runs, the stego comes
    back; what embed_frames' keywords say is said to embed_device"""
    kw = dict(embed_kw)
    device, block_key, first_frame = kw.pop("device", 0), kw.pop("block_key", None), kw.pop("first_frame", 0)
    counted = 4 if kw.get("readback_margin") is not None else 2 if any(
        kw.get(name) for name in ("readback", "readback_keyed", "readback_stepped")) else 0
    stack = _as_stack(frames)
    f, h, w = stack.shape
    work_bytes = coded_workspace_bytes(info.size, rate, copies, outer, capacity_bits(f, h, w, n_ac))
    order = block_order(block_key, first_frame)
    _enc.load()
    counts = np.zeros(4, np.uint64)
    with Staged(device) as dev:
        d_gray, d_payload = dev.upload(stack), dev.upload(np.packbits(info))
        d_stego, d_work, d_counts = dev.alloc(stack.size), dev.alloc(work_bytes), 0
        if counted:
            d_counts = dev.alloc(32)
            dev.zero(d_counts, 32)
        used = embed_coded_device(d_gray, d_stego, Planes.contiguous(f, h, w), delta, n_ac, d_payload, info.size, d_work, work_bytes,
                                  rate=rate, copies=copies, outer=outer, order=order, first_frame=first_frame, d_counts=d_counts, **kw)
        stego = dev.download(d_stego, pinned_empty(stack.shape))
        if counted:
            dev.download(d_counts, counts)
        dev.synchronise()
    tail = () if not counted else (MarginCounts(*map(int, counts)),) if counted == 4 else (ReadbackCounts(int(counts[0]), int(counts[1])),)
    return (stego, used, int(info.size), *tail)


def embed_coded_frames(frames: np.ndarray, delta, n_ac, info_bits, rate: int = 2, copies: int | None = 1, outer: bool = False,
                       encoder: str = "host", **embed_kw):
    """Embed a payload under the convolutional code (svsdct/fec.py, include/svsfec.h): fec.encode(info_bits, rate) - rate 2 or 3
    coded bits a payload bit, or a punctured code of fec.PUNCTURED (23, 34, 56, 78: rate 2/3 .. 7/8, the unsent bits are not
    embedded), six tail bits -, then soft.tile when copies > 1 (copies=None: as many as the stack's capacity
    holds, the last one cut), then embed_frames, which takes every other keyword (coeffs, dither_key, block_key, steps, the
    rules and read-backs).  The coded stream must fit: fec.info_bits(capacity, rate) is the largest payload of one copy.
    Returns (stego, used, n_info), and the counts behind them where embed_frames returns them; the receiver passes n_info, rate
    and copies to extract_coded_frames.
    outer=True: the payload, whole bytes (ValueError otherwise), first goes through the Reed-Solomon outer code (svsdct/rs.py,
    include/svsrs.h): bytes -> rs.encode -> fec.encode -> embed; rs.payload_bits(capacity, rate) is then the largest payload.
    n_info stays the PAYLOAD's bit count, and the receiver passes outer=True as well.
    matrix: refused (ValueError): a syndrome bit has no margin, so a matrix call has no soft form to decode.
    encoder: "host" (svs_rs_encode, svs_fec_encode and soft.tile on the CPU, the coded stream uploaded) or "device" (the packed
    payload uploaded, then embed_coded_device: libsvsenc.so's encoders and the embed on the GPU).  The same stego and counts
    either way, byte for byte."""
    _no_matrix(embed_kw.get("matrix"), "coded")
    if "bit_offset" in embed_kw or "n_bits" in embed_kw:
        raise ValueError("embed_coded_frames embeds the whole coded stream: bit_offset and n_bits are not its keywords")
    if encoder not in ("host", "device"):
        raise ValueError(f'encoder {encoder!r}: "host" or "device"')
    copies = _coded_copies(copies)
    info = np.asarray(str_to_bits(info_bits) if isinstance(info_bits, str) else info_bits, np.uint8).reshape(-1)
    if info.size == 0:
        raise ValueError("an empty payload cannot be coded")
    if encoder == "device":
        return _embed_coded_on_device(frames, delta, n_ac, info, rate, copies, outer, embed_kw)
    f, h, w = _as_stack(frames).shape
    plan = _CodedPlan.of(info.size, rate, copies, outer, capacity_bits(f, h, w, n_ac))      # refuses before anything is encoded
    coded = _fec.encode(np.unpackbits(_rs.encode_array(np.packbits(info))) if outer else info, rate)
    stream = coded if copies == 1 else _soft.tile(coded, plan.stream)
    stego, used, *counts = embed_frames(frames, delta, n_ac, stream, **embed_kw)
    return (stego, used, int(info.size), *counts)


def extract_coded_frames(frames: np.ndarray, delta, n_ac, n_info: int, rate: int = 2, copies: int | None = 1, device: int = 0,
                         mode: str | None = None, block_key=None, first_frame=None, coeffs=None, dither_key=None, steps=None,
                         matrix=None, outer: bool = False, lost_frames=(), erase_margin: int = 1):
    """Read a payload embedded by embed_coded_frames: the frames go to the device once, the soft bytes never leave it, and only
    ceil(n_info / 8) bytes come back.
      copies = 1:  svs_soft_extract_dev into device memory, then svs_fec_decode_soft_dev on its first fec.coded_bits(n_info, rate)
                   bytes, on the same stream.
      otherwise:   svs_soft_vote_dev with period = n_coded into a zeroed tally, then svs_fec_decode_weights_dev on the tally.
                   Every capacity bit of the stack votes, so bits behind the last copy vote as noise: let the copies fill the
                   capacity (copies=None on both sides does).
    rate: the sender's, 2, 3 or a punctured code of fec.PUNCTURED; n_coded = fec.coded_bits(n_info, rate) is then the number of
    SENT bits, the period of the tally included, and the decoder gives the unsent bits the weight 0.
    coeffs, dither_key, block_key, first_frame, steps: as extract_soft_frames (the sender's).  Returns uint8 0/1 [n_info].
    outer=True (the sender's): n_info is the payload's bit count, whole bytes (ValueError otherwise).  The Viterbi decoder
    writes the 8 rs.coded_bytes(n_info / 8) bits of the Reed-Solomon stream as packed bytes, svs_rs_decode_dev decodes them in
    place on the same stream, and nothing leaves the device in between.  Returns (bits uint8 0/1 [n_info], status uint8
    [rs.codewords(n_info / 8)]: the bytes corrected in each codeword, or 255 - that codeword did not decode and is as the Viterbi
    decoder left it).
    lost_frames: indices within the stack of frames that the receiver gave up on - a replaced frame, an overlaid logo
    (extract_histogram_frames tells such frames apart).  Needs outer=True and copies = 1 (ValueError otherwise, as for an index
    that is no integer or out of range, before any device work).  Frame i owns the capacity bits [i cap / f, (i + 1) cap / f) of
    the stream, under a block key, a selection or a dither as well.  For each lost frame its soft bytes are set to 0x00 behind
    the soft extract (svs_memset on the same stream; 0x00 is the weight -1, the smallest the format has, where noise would vote
    with full margins), its sent bits are mapped to the bytes of the Reed-Solomon stream they bear on
    (fec.steps_of_sent_bits, divided by 8), the span is widened by erase_margin bytes on each side, and the codewords are decoded
    by svs_rse_decode_dev (svsdct/rse.py, include/svsrse.h) with those bytes erased: 2 e + f <= 32 a codeword, where blind decoding
    stops at 16 wrong bytes.  The status is then the bytes changed, 0 .. 32, or 255.  Without lost_frames nothing changes.
    matrix: refused (ValueError): a syndrome bit has no margin."""
    _no_matrix(matrix, "coded")
    copies = _coded_copies(copies)
    lost, erase_margin = _lost_frames_arg(lost_frames, erase_margin, outer, copies)
    n_info = int(n_info)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    plan = _CodedPlan.of(n_info, rate, copies, outer, capacity_bits(f, h, w, n_ac))
    if plan.inner == 0:
        raise ValueError("an empty payload cannot be decoded")
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, block_key, 0 if first_frame is None else first_frame, coeffs, dither_key)
    if lost and not lost[-1] < f:
        raise ValueError(f"lost_frames: frame {lost[-1]} is outside the stack's 0 .. {f - 1}")
    per_frame = plan.capacity // f
    lost_bits = [(i * per_frame, min((i + 1) * per_frame, plan.coded)) for i in lost if i * per_frame < plan.coded]
    _fec.load()
    if outer:
        (_rse if lost else _rs).load()
    n_cw = _rs.codewords(plan.k)
    with Staged(device) as dev:
        d_gray, d_out = dev.upload(stack), dev.alloc((plan.inner + 7) // 8)
        d_work = dev.alloc(plan.capacity if copies == 1 else 4 * plan.coded)
        d_status = dev.alloc(n_cw) if outer else 0
        d_erased = 0
        if lost:
            d_erased = dev.upload(_rse.mask(plan.k, [lost_span(lo, hi, rate, plan.k, erase_margin) for lo, hi in lost_bits]))
        _extract_coded_device(d_gray, Planes.contiguous(f, h, w), delta, n_ac, plan, rate, copies, d_work, d_out, d_status, d_erased,
                              lost_bits, call, table, mode)
        status = dev.download(d_status, n_cw) if outer else None
        packed = dev.download(d_out, (n_info + 7) // 8)      # under outer the data bytes lead the Reed-Solomon stream
        dev.synchronise()
    bits = np.unpackbits(packed, count=n_info)
    return (bits, status) if outer else bits


def requantise_frames(frames: np.ndarray, steps_or_quality, device: int = 0) -> np.ndarray:
    """The requantisation channel on a stack of gray frames on the GPU (svs_requantise, include/svsdct.h): every 8x8 block is
    transformed, each coefficient divided by its step, rounded and multiplied back, the block inverted and ROUNDED to uint8 -
    the luminance path of JPEG / MJPEG on the embed's grid.  A measuring tool: what of a stego clip survives an intra codec.
    steps_or_quality: a quality 1..100 (channel.quality_steps) or a table of 64 steps in 1..255, flat row-major, entry 0 DC.
    Returns a new uint8 array [F,H,W]; the input is not touched."""
    steps = _channel.steps_struct(steps_or_quality)
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    out = pinned_empty(stack.shape)
    planes = Planes.contiguous(f, h, w)
    native.check(lib.svs_requantise(stack.ctypes.data, out.ctypes.data, C.byref(planes), C.byref(steps), 0), "svs_requantise")
    return out


# ---- the reference operator's own payload types: '0' / '1' strings ------------------------------------------
_utf8_and_size = None


def _ascii_address(text: str):
    """(address, length) of the characters of an ASCII str WITHOUT copying them (CPython keeps ASCII strings as one byte per
    character; PyUnicode_AsUTF8AndSize hands out that very buffer).  The reference's frame loop passes the whole remaining
    payload to every call (embed_process.py:116) - slicing or encoding it per frame would copy it per frame."""
    global _utf8_and_size
    if not isinstance(text, str):
        raise TypeError("the payload must be a str of '0' / '1' characters (bit_payload_segment of the reference operator); "
                        "use embed_frames for arrays of bits")
    if _utf8_and_size is None:
        fn = C.pythonapi.PyUnicode_AsUTF8AndSize
        fn.restype, fn.argtypes = C.c_void_p, [C.py_object, C.POINTER(C.c_ssize_t)]
        _utf8_and_size = fn
    size = C.c_ssize_t(0)
    addr = _utf8_and_size(text, C.byref(size))
    if not addr or size.value != len(text):
        raise ValueError("the payload must be a string of '0' / '1' characters")
    return addr, size.value


def embed_frames_str(frames: np.ndarray, delta, n_ac, payload: str | None, device: int = 0, mode: str | None = None,
                     want_gray: bool = False, dither_key=None, matrix=None):
    """`embed_frames` in the reference operator's own types (config_and_setup.py:106-109,172): the payload is a '0'/'1'
    string (bit_payload_segment) of which at most the capacity is read from the front - the characters go to the device as
    they are and are packed there (svs_embed_str); None / "" = nothing to embed.  want_gray: also return a copy of the input
    frames as an array of its own, the operator's first return value - the library makes it while the GPU works.
    dither_key: refused (ValueError) - a keyed dither has no _str form.
    Returns (stego uint8 [F,H,W], n_embedded) or (gray_copy, stego, n_embedded).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no _str form."""
    _no_matrix(matrix, "_str")
    no_dither(dither_key, "_str")
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    addr, n_chars = _ascii_address(payload) if payload else (None, 0)
    stego = pinned_empty(stack.shape)
    gray = np.empty_like(stack) if want_gray else None
    done = C.c_uint64(0)
    planes = Planes.contiguous(f, h, w)
    rc = lib.svs_embed_str(stack.ctypes.data, gray.ctypes.data if want_gray else None, stego.ctypes.data, C.byref(planes),
                           float(delta), int(n_ac), addr, n_chars, mode_flags(mode), C.byref(done))
    native.check(rc, "svs_embed_str")
    return (gray, stego, int(done.value)) if want_gray else (stego, int(done.value))


def extract_frames_str(frames: np.ndarray, delta, n_ac, device: int = 0, mode: str | None = None, dither_key=None, matrix=None) -> str:
    """`extract_frames` returning the reference operator's own type: the '0'/'1' string of config_and_setup.py:173-174
    (expanded on the device, one decode on the host).  dither_key: refused (ValueError) - no _str form.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no _str form."""
    _no_matrix(matrix, "_str")
    no_dither(dither_key, "_str")
    lib = native.load()
    native.ensure_device(device)
    stack = _as_stack(frames)
    f, h, w = stack.shape
    cap = capacity_bits(f, h, w, n_ac)
    if cap == 0:
        return ""
    out = pinned_empty(cap)
    got = C.c_uint64(0)
    planes = Planes.contiguous(f, h, w)
    rc = lib.svs_extract_str(stack.ctypes.data, C.byref(planes), float(delta), int(n_ac), out.ctypes.data, cap,
                             mode_flags(mode), C.byref(got))
    native.check(rc, "svs_extract_str")
    return str(memoryview(out)[: int(got.value)], "ascii")


# ---- device-pointer level -------------------------------------------------------------------
def embed_device(d_gray: int, d_stego: int, planes: Planes, delta, n_ac, d_bits_packed: int,
                 bit_offset: int, n_bits: int, stream: int = 0, mode: str | None = None,
                 order: BlockOrder | None = None, readback: bool = False, d_counts: int = 0,
                 nearest: bool = False, coeffs=None, minmove: bool = False, dither_key=None, first_frame: int | None = None,
                 readback_keyed: bool = False, steps=None, readback_stepped: bool = False,
                 readback_margin: int | None = None, matrix=None) -> int:
    """Enqueue the embed kernel on `stream` (a hipStream_t handle as int); returns bits embedded.  order: None, or a
    native.BlockOrder (block_order(key, first_frame)) - the keyed block order of svs_embed_ordered_dev.  readback: the
    read-back pass follows on the same stream (svs_embed_readback_dev); d_counts: 0, or a device buffer of two uint64 that
    it adds {repaired, unrepaired} into.  nearest, minmove: SVS_NEAREST, SVS_MINMOVE, as embed_frames.  coeffs: a payload coefficient selection,
    as embed_frames (svs_embed_select_dev).  dither_key: a keyed dither, as embed_frames (svs_embed_dithered_dev); its clip
    frame index is first_frame, by default the order's (0 without one) - the two must agree.  readback_keyed: the read-back
    pass under coeffs and / or dither_key (svs_embed_dithered_readback_dev; d_counts as with readback); with neither it makes
    the readback call; ValueError together with readback.  steps: per-coefficient QIM steps, as embed_frames
    (svs_stepped_embed_dev; delta is then not used).  readback_stepped: the read-back pass under steps
    (svs_stepped_embed_readback_dev; d_counts as with readback); it needs steps; ValueError with readback or readback_keyed.
    readback_margin: an int g in 1..127, the margin pass behind that read-back (svs_stepped_embed_readback_margin_dev; it implies
    readback_stepped; d_counts is then FOUR uint64: repaired, unrepaired, strengthened, weak).  matrix: k or (k, "pair"), as
    embed_frames (svs_matrix_embed_dev; it needs steps; ValueError with any read-back switch)."""
    _one_readback(readback, readback_keyed)      # ahead of the mode's ValueError
    mx = _matrix_arg(matrix, steps, readback, readback_keyed, readback_stepped, readback_margin)
    gate = _readback_margin_arg(readback_margin, steps, readback, readback_keyed)
    stepped_rb = _readback_stepped_arg(readback_stepped, steps, readback, readback_keyed)
    done = C.c_uint64(0)
    flags = embed_flags(mode, nearest, minmove)
    table = _steps_arg(steps, readback, readback_keyed)
    call = _resolve(n_ac, order, None, first_frame, coeffs, dither_key, readback, readback_keyed)
    if gate:
        _stepped_call(native.load(), "embed_readback_margin", call, table, [d_gray, d_stego, C.byref(planes)], n_ac,
                      [d_bits_packed, int(bit_offset), int(n_bits), gate, flags, C.byref(done)], (stream or None,),
                      counts=(d_counts or None,))
        return int(done.value)
    if table is not None:
        _stepped_call(native.load(), "embed_readback" if stepped_rb else "embed", call, table, [d_gray, d_stego, C.byref(planes)],
                      n_ac, [d_bits_packed, int(bit_offset), int(n_bits), flags, C.byref(done)], (stream or None,),
                      counts=(d_counts or None,) if stepped_rb else (), matrix=mx)
        return int(done.value)
    _gray_call(native.load(), "embed", call, [d_gray, d_stego, C.byref(planes)], delta, n_ac,
               [d_bits_packed, int(bit_offset), int(n_bits), flags, C.byref(done)], d_counts or None, (stream or None,))
    return int(done.value)


def embed_coded_device(d_gray: int, d_stego: int, planes: Planes, delta, n_ac, d_payload_packed: int, n_info: int, d_work: int,
                       work_bytes: int, rate: int = 2, copies: int | None = 1, outer: bool = False, stream: int = 0, **embed_kw) -> int:
    """embed_coded_frames for a payload that lies on the device: everything is enqueued on `stream`, nothing leaves the device and
    nothing is synchronised.  d_payload_packed: the n_info payload bits, packed MSB first, any alignment (under outer whole
    bytes, the data of the outer code).  d_work: 4-byte aligned scratch of coded_workspace_bytes(n_info, rate, copies, outer,
    capacity) bytes, work_bytes its size.  The chain: with outer svs_rs_encode_dev (out of place, into d_work), then
    svs_fec_encode_dev, with copies != 1 svs_bits_tile_dev, then embed_device on the result, which takes every other keyword
    (mode, order, first_frame, coeffs, dither_key, steps, the rules, the read-backs and d_counts).  Returns the bits embedded.
    ValueError, before any device work: matrix; a payload that is not whole bytes under outer; a coded stream above the
    capacity; a workspace that is misaligned or too small."""
    _no_matrix(embed_kw.get("matrix"), "coded")
    if "bit_offset" in embed_kw or "n_bits" in embed_kw:
        raise ValueError("embed_coded_device embeds the whole coded stream: bit_offset and n_bits are not its keywords")
    copies, n_info = _coded_copies(copies), int(n_info)
    if n_info < 1:
        raise ValueError("an empty payload cannot be coded")
    plan = _CodedPlan.of(n_info, rate, copies, outer, capacity_bits(planes.n_frames, planes.height, planes.width, n_ac))
    if int(d_work) % 4 or int(work_bytes) < plan.work_bytes:
        raise ValueError(f"the workspace must be 4-byte aligned and hold {plan.work_bytes} bytes (coded_workspace_bytes)")
    d_inner, d_coded, d_bits = int(d_payload_packed), int(d_work) + plan.at_coded, int(d_work) + plan.at_stream
    if outer:
        d_inner = int(d_work)
        _enc.rs_encode_device(int(d_payload_packed), plan.k, d_inner, _rs.coded_bytes(plan.k), stream)
    _enc.fec_encode_device(d_inner, plan.inner, rate, d_coded, (plan.coded + 7) // 8, stream)
    if copies != 1:
        _enc.tile_device(d_coded, plan.coded, d_bits, plan.stream, (plan.stream + 7) // 8, stream)
    return embed_device(d_gray, d_stego, planes, delta, n_ac, d_bits, 0, plan.stream, stream=stream, **embed_kw)


def _extract_coded_device(d_gray: int, planes: Planes, delta, n_ac, plan: _CodedPlan, rate: int, copies, d_work: int, d_out: int,
                          d_status: int, d_erased: int, lost_bits, call: _GrayCall, table, mode, stream: int = 0) -> None:
    """The receiving chain, the mirror image of embed_coded_device: everything is enqueued on `stream`, nothing leaves the device
    and nothing is synchronised.  copies = 1: the soft extract into d_work (plan.capacity bytes), the soft bytes of the sent-bit
    ranges lost_bits set to 0x00, the Viterbi decoder on the soft bytes; otherwise d_work (4 plan.coded bytes, 4-byte aligned)
    is zeroed, takes the vote, and the decoder reads the tally.  d_out: ceil(plan.inner / 8) bytes.  d_status: 0, or
    rs.codewords(plan.k) bytes - then the Reed-Solomon decoder follows in place on d_out, with the mask d_erased where it is
    not 0 (svs_rse_decode_dev) and blind without (svs_rs_decode_dev).  call, table: the _GrayCall and the steps of the sender."""
    lib, st = native.load(), (stream or None,)
    front, out_bytes = [d_gray, C.byref(planes)], (plan.inner + 7) // 8
    if copies == 1:
        _soft_call(lib, "extract", call, front, delta, n_ac, [d_work, plan.capacity], mode_flags(mode), st, table)
        for lo, hi in lost_bits:
            native.check(lib.svs_memset(d_work + lo, 0, hi - lo, *st), "svs_memset")
        _fec.decode_soft_device(d_work, plan.inner, rate, d_out, out_bytes, stream)
    else:
        native.check(lib.svs_memset(d_work, 0, 4 * plan.coded, *st), "svs_memset")
        _soft_call(lib, "vote", call, front, delta, n_ac, [plan.coded, 0, d_work], 0, st, table)
        _fec.decode_weights_device(d_work, plan.inner, rate, d_out, out_bytes, stream)
    if d_status and d_erased:
        _rse.decode_device(d_out, plan.k, d_erased, d_status, _rs.codewords(plan.k), stream=stream)
    elif d_status:
        _rs.decode_device(d_out, plan.k, d_status, _rs.codewords(plan.k), stream=stream)


def extract_device(d_gray: int, planes: Planes, delta, n_ac, d_bits_out: int, out_capacity_bytes: int,
                   stream: int = 0, mode: str | None = None, order: BlockOrder | None = None, coeffs=None, dither_key=None,
                   first_frame: int | None = None, steps=None, matrix=None) -> int:
    """Enqueue the extract kernel on `stream`; returns the number of bits the batch yields.  order, coeffs, dither_key,
    first_frame, steps, matrix: as embed_device (matrix: svs_matrix_extract_dev, blocks * k bits)."""
    got = C.c_uint64(0)
    mx = _matrix_arg(matrix, steps)
    table = _steps_arg(steps)
    call = _resolve(n_ac, order, None, first_frame, coeffs, dither_key)
    back = [d_bits_out, int(out_capacity_bytes), mode_flags(mode), C.byref(got)]
    if table is not None:
        _stepped_call(native.load(), "extract", call, table, [d_gray, C.byref(planes)], n_ac, back, (stream or None,), matrix=mx)
    else:
        _gray_call(native.load(), "extract", call, [d_gray, C.byref(planes)], delta, n_ac, back, None, (stream or None,))
    return int(got.value)


def extract_soft_device(d_gray: int, planes: Planes, delta, n_ac, d_soft_out: int, out_capacity_bytes: int, stream: int = 0,
                        mode: str | None = None, order: BlockOrder | None = None, coeffs=None, dither_key=None,
                        first_frame: int | None = None, steps=None, matrix=None) -> int:
    """Enqueue the soft-decision extraction on `stream` (svs_soft_extract_dev): one byte per capacity bit into d_soft_out
    (4-byte aligned, at least the capacity in bytes); returns the number of bytes the batch yields.  order, coeffs, dither_key,
    first_frame, steps: as extract_device (steps: svs_stepped_soft_extract_dev).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no soft form."""
    _no_matrix(matrix, "soft")
    table = _steps_arg(steps)
    call = _resolve(n_ac, order, None, first_frame, coeffs, dither_key)
    return _soft_call(native.load(), "extract", call, [d_gray, C.byref(planes)], delta, n_ac, [d_soft_out, int(out_capacity_bytes)],
                      mode_flags(mode), (stream or None,), table)


def extract_vote_device(d_gray: int, planes: Planes, delta, n_ac, d_tally: int, period, stream_bit0: int = 0, stream: int = 0,
                        order: BlockOrder | None = None, first_frame: int | None = None, coeffs=None, dither_key=None,
                        steps=None, matrix=None) -> int:
    """Enqueue the fused soft vote on `stream` (svs_soft_vote_dev): the batch's votes are ADDED into d_tally, `period` int32
    values in device memory (4-byte aligned) that the caller zeroes before the first batch; stream_bit0 is the capacity of the
    frames before the batch.  Returns the number of bits that voted.  order, coeffs, dither_key, first_frame, steps: as
    extract_soft_device (steps: svs_stepped_soft_vote_dev).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no vote form."""
    _no_matrix(matrix, "vote")
    table = _steps_arg(steps)
    call = _resolve(n_ac, order, None, first_frame, coeffs, dither_key)
    return _soft_call(native.load(), "vote", call, [d_gray, C.byref(planes)], delta, n_ac, [_period(period), int(stream_bit0), d_tally],
                      0, (stream or None,), table)


def extract_histogram_device(d_gray: int, planes: Planes, delta, n_ac, d_hist: int, stream: int = 0, first_frame: int | None = None,
                             coeffs=None, dither_key=None, steps=None, matrix=None) -> int:
    """Enqueue the fused per-frame soft histograms on `stream` (svs_soft_histogram_dev): the batch's bytes are ADDED into d_hist,
    planes.n_frames rows of 256 uint32 in device memory (4-byte aligned) that the caller zeroes before the first call; a clip
    read in batches passes d_hist + 1024 * (frames before the batch) and, under a dither, first_frame advanced by as many.
    Returns the number of bytes counted.  No order and no block_key: a frame's counts do not depend on one (see
    extract_histogram_frames).  coeffs, dither_key, first_frame, steps: as extract_soft_device (steps:
    svs_stepped_soft_histogram_dev).
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no histogram form."""
    _no_matrix(matrix, "histogram")
    table = _steps_arg(steps)
    call = _resolve(n_ac, None, None, first_frame, coeffs, dither_key)
    return _soft_call(native.load(), "histogram", call, [d_gray, C.byref(planes)], delta, n_ac, [d_hist], 0, (stream or None,), table)


def requantise_device(d_in: int, d_out: int, planes: Planes, steps_or_quality, stream: int = 0) -> None:
    """Enqueue the requantisation channel on `stream` (svs_requantise_dev): planes at d_in -> planes of the same geometry at
    d_out, which may be d_in (in place) or must not overlap it.  steps_or_quality: as requantise_frames."""
    steps = _channel.steps_struct(steps_or_quality)
    native.check(native.load().svs_requantise_dev(d_in, d_out, C.byref(planes), C.byref(steps), 0, stream or None),
                 "svs_requantise_dev")


# ---- fused colour path (BGR in, BGR out) ---------------------------------
def _weights_arg(weights):
    if weights is None:
        return None, None
    w = np.ascontiguousarray(weights, np.uint32)
    if w.shape != (4,):
        raise ValueError("weights must be (wb, wg, wr, shift)")
    return w, w.ctypes.data


def _bgr_flags(mode, keep_colour, nearest=False, minmove=False):
    return embed_flags(mode, nearest, minmove) | (native.SVS_KEEP_COLOUR if keep_colour else 0)


def embed_bgr_device(d_bgr_in: int, d_bgr_out: int, d_gray_ref: int, planes: Planes, delta, n_ac,
                     d_bits_packed: int, bit_offset: int, n_bits: int, stream: int = 0, mode: str | None = None,
                     weights=None, in_pitches=None, out_pitches=None, keep_colour: bool = False, readback: bool = False,
                     d_counts: int = 0, nearest: bool = False, coeffs=None, minmove: bool = False, dither_key=None, matrix=None) -> int:
    """Enqueue the fused BGR -> gray -> embed -> BGR kernel over packed (or pitched) interleaved BGR frames;
    `d_gray_ref` (0 to skip) receives the gray frames before embedding.  keep_colour: stego pixels keep the cover's
    colour (SVS_KEEP_COLOUR; their gray is the stego plane) instead of B = G = R.  readback: the read-back pass follows on
    the same stream, in place on the BGR output (svs_embed_bgr_readback_dev); d_counts: 0, or a device buffer of two uint64
    that the call adds {repaired, unrepaired} into.  nearest, minmove: SVS_NEAREST, SVS_MINMOVE, as embed_frames.
    dither_key: refused (ValueError) - no colour form.  Returns bits embedded.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no colour form."""
    _no_matrix(matrix, "colour")
    _no_coeffs(coeffs)
    no_dither(dither_key, "colour")
    irp, ifp = in_pitches or (3 * planes.width, 3 * planes.width * planes.height)
    orp, ofp = out_pitches or (3 * planes.width, 3 * planes.width * planes.height)
    keep, wptr = _weights_arg(weights)
    done = C.c_uint64(0)
    name = "svs_embed_bgr" + ("_readback" if readback else "") + "_dev"
    rc = getattr(native.load(), name)(d_bgr_in, irp, ifp, d_bgr_out, orp, ofp, d_gray_ref or None, C.byref(planes), wptr,
                                      float(delta), int(n_ac), d_bits_packed, int(bit_offset), int(n_bits),
                                      _bgr_flags(mode, keep_colour, nearest, minmove), C.byref(done),
                                      *([d_counts or None] if readback else ()), stream or None)
    native.check(rc, name)
    return int(done.value)


def extract_bgr_device(d_bgr: int, planes: Planes, delta, n_ac, d_bits_out: int, out_capacity_bytes: int,
                       stream: int = 0, weights=None, pitches=None, coeffs=None, dither_key=None, matrix=None) -> int:
    """Enqueue extraction straight from interleaved BGR frames; returns the number of bits the batch yields.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no colour form."""
    _no_matrix(matrix, "colour")
    _no_coeffs(coeffs)
    no_dither(dither_key, "colour")
    rp, fp = pitches or (3 * planes.width, 3 * planes.width * planes.height)
    keep, wptr = _weights_arg(weights)
    got = C.c_uint64(0)
    rc = native.load().svs_extract_bgr_dev(d_bgr, rp, fp, C.byref(planes), wptr, float(delta), int(n_ac),
                                           d_bits_out, int(out_capacity_bytes), C.byref(got), stream or None)
    native.check(rc, "svs_extract_bgr_dev")
    return int(got.value)


def _as_bgr_stack(frames: np.ndarray) -> np.ndarray:
    a = np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise TypeError("frames must be uint8 [F,H,W,3] (BGR)")
    if a.shape[1] % 8 or a.shape[2] % 8:
        raise ValueError("frame height and width must be multiples of 8")
    return np.ascontiguousarray(a)


def embed_bgr_frames(frames_bgr: np.ndarray, delta, n_ac, bits, bit_offset: int = 0, n_bits: int | None = None,
                     device: int = 0, mode: str | None = None, weights=None, want_gray: bool = True,
                     keep_colour: bool = False, readback: bool = False, nearest: bool = False, coeffs=None,
                     minmove: bool = False, dither_key=None, matrix=None):
    """BGR frames in, stego BGR frames out (one fused pass on the GPU).  keep_colour: see embed_bgr_device.  readback: the
    blocks whose payload bits do not read back are repaired in place on the BGR output (svs_embed_bgr_readback,
    include/svsdct.h).  nearest, minmove: SVS_NEAREST, SVS_MINMOVE, as embed_frames.
    Returns (stego_bgr uint8 [F,H,W,3], gray uint8 [F,H,W] (the cover's) or None, n_embedded), with readback
    (stego_bgr, gray, n_embedded, ReadbackCounts).  dither_key: refused (ValueError) - no colour form.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no colour form."""
    _no_matrix(matrix, "colour")
    _no_coeffs(coeffs)
    no_dither(dither_key, "colour")
    lib = native.load()
    native.ensure_device(device)
    stack = _as_bgr_stack(frames_bgr)
    f, h, w, _ = stack.shape
    if isinstance(bits, str):
        bits = str_to_bits(bits)
    bits = np.asarray(bits, np.uint8)
    if n_bits is None:
        n_bits = max(0, bits.size - bit_offset)
    if bit_offset + n_bits > bits.size:
        raise ValueError("bit_offset + n_bits exceeds the payload length")
    packed, bit_offset = _pack_window(bits, bit_offset, n_bits)
    planes = Planes.contiguous(f, h, w)
    out = pinned_empty(stack.shape)
    gray = pinned_empty((f, h, w)) if want_gray else None
    keep, wptr = _weights_arg(weights)
    done = C.c_uint64(0)
    counts = native.ReadbackCounts()
    name = "svs_embed_bgr" + ("_readback" if readback else "")
    rc = getattr(lib, name)(stack.ctypes.data, out.ctypes.data, gray.ctypes.data if want_gray else None, C.byref(planes), wptr,
                            float(delta), int(n_ac), packed.ctypes.data, int(bit_offset), int(n_bits),
                            _bgr_flags(mode, keep_colour, nearest, minmove), C.byref(done),
                            *([C.byref(counts)] if readback else ()))
    native.check(rc, name)
    if readback:
        return out, gray, int(done.value), ReadbackCounts(int(counts.repaired), int(counts.unrepaired))
    return out, gray, int(done.value)


def extract_bgr_frames(frames_bgr: np.ndarray, delta, n_ac, device: int = 0, weights=None, dither_key=None, matrix=None):
    """Extract the packed bit stream straight from BGR frames.  Returns (packed uint8, n_bits).  dither_key: refused.
    matrix: refused (ValueError): matrix embedding (svsdct/matrix.py) has no colour form."""
    _no_matrix(matrix, "colour")
    no_dither(dither_key, "colour")
    lib = native.load()
    native.ensure_device(device)
    stack = _as_bgr_stack(frames_bgr)
    f, h, w, _ = stack.shape
    cap = capacity_bits(f, h, w, n_ac)
    nbytes = max(4, (cap + 7) // 8 + (-((cap + 7) // 8)) % 4)
    out = np.zeros(nbytes, np.uint8)
    planes = Planes.contiguous(f, h, w)
    keep, wptr = _weights_arg(weights)
    got = C.c_uint64(0)
    rc = lib.svs_extract_bgr(stack.ctypes.data, C.byref(planes), wptr, float(delta), int(n_ac), out.ctypes.data,
                             nbytes, C.byref(got))
    native.check(rc, "svs_extract_bgr")
    n = int(got.value)
    return out[: (n + 7) // 8], n


# ---- frame sharding across ranks ----------------------------------------------
def shard_frames(n_frames: int, world_size: int, rank: int) -> tuple[int, int]:
    """Contiguous frame range [first, first+count) of `rank`, so that the global bit stream is the
    rank-order concatenation of the ranks' streams."""
    base, extra = divmod(n_frames, world_size)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)
