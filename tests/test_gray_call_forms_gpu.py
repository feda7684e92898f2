"""The same gray call through every entry point of the C ABI that can express it: identical stego bytes, n_embedded and
read-back counts (extraction: identical bits).  These are equalities between FORMS of a call - equality with the oracle is
what the other GPU tests are for - over one block per lane (3 blocks per row) and the two-blocks-per-lane one-row path (an
even count), one-row streaming, two-row streaming and exact kernels (n_ac 3, 10, 20), and the host-pointer calls against
one device call over the batch when they stage it in at least two chunks of whole frames."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _Dev
from testlib import experiments_library, using_library
from svsdct import batch, coeffs, native, synth
from svsdct.native import BlockOrder, Dither, Planes

pytestmark = pytest.mark.gpu

DELTA, BIT_OFFSET, FIRST = 8.0, 37, 5
ORDER, DITHER = BlockOrder(0xC0FFEE1234, FIRST, 0), Dither(0x0123456789ABCDEF, FIRST, 0)
G, P = native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT
# stem -> does it take (order, coeffs, dither), n_ac, counts
STEMS = {"": ((), True, False), "_ordered": (("order",), True, False), "_select": (("order", "coeffs"), False, False),
         "_dithered": (("order", "coeffs", "dither"), True, False), "_readback": (("order",), True, True),
         "_dithered_readback": (("order", "coeffs", "dither"), True, True)}


@pytest.fixture(autouse=True)
def chunked_experiments_library(monkeypatch):
    """a frame is 384 or 512 bytes: with 1 KB chunks three frames travel in at least two chunks of whole frames"""
    monkeypatch.setenv("SVS_STAGE_CHUNK_KB", "1")
    with using_library(experiments_library()) as lib:
        native.ensure_device(0)
        yield lib


def cover_of(shape, clipping=True):
    frames = synth.synthetic_frames(*shape, seed=shape[2])
    frames[0, :8, :16] = 128                                   # flat blocks: undecided by the streaming guard
    if clipping:
        frames[1, 8:16, 8:24] = 255 * (np.indices((8, 16)).sum(0) % 2)      # 0 / 255 pixels: blocks that clip
    return frames


def payload_of(shape, n_ac):
    bits = synth.synthetic_bits(BIT_OFFSET + batch.capacity_bits(*shape, n_ac) - 5, seed=n_ac)
    return batch.pack_bits(bits), bits.size - BIT_OFFSET


def _structs(stem, given):
    return [C.byref(given[s]) if given.get(s) is not None else None for s in STEMS[stem][0]]


def embed(lib, stem, host, cover, n_ac, flags, **given):
    """svs_embed<stem> (host) or svs_embed<stem>_dev over the cover -> (stego, n_embedded, read-back counts or None)"""
    _, takes_n_ac, takes_counts = STEMS[stem]
    planes, done = Planes.contiguous(*cover.shape), C.c_uint64(0)
    packed, n_bits = payload_of(cover.shape, n_ac)
    middle = [*_structs(stem, given), DELTA, *([n_ac] if takes_n_ac else [])]
    if host:
        stego, counts = np.zeros_like(cover), native.ReadbackCounts(7, 7)
        rc = getattr(lib, "svs_embed" + stem)(cover.ctypes.data, stego.ctypes.data, C.byref(planes), *middle, packed.ctypes.data,
                                              BIT_OFFSET, n_bits, flags, C.byref(done), *([C.byref(counts)] if takes_counts else []))
        native.check(rc, "svs_embed" + stem)
        return stego, done.value, (counts.repaired, counts.unrepaired) if takes_counts else None
    d_gray, d_stego, d_bits, d_counts = _Dev(cover.nbytes), _Dev(cover.nbytes), _Dev(packed.size + 8), _Dev(16)
    d_gray.put(cover)
    d_bits.put(packed)
    d_counts.put(np.zeros(2, np.uint64))
    rc = getattr(lib, f"svs_embed{stem}_dev")(d_gray.ptr, d_stego.ptr, C.byref(planes), *middle, d_bits.ptr, BIT_OFFSET, n_bits, flags,
                                               C.byref(done), *([d_counts.ptr] if takes_counts else []), None)
    native.check(rc, f"svs_embed{stem}_dev")
    return d_stego.get().reshape(cover.shape), done.value, tuple(int(c) for c in d_counts.get(dtype=np.uint64)) if takes_counts else None


def extract(lib, stem, host, stego, n_ac, flags, **given):
    """svs_extract<stem> or svs_extract<stem>_dev -> (packed bits, n_bits)"""
    planes, got = Planes.contiguous(*stego.shape), C.c_uint64(0)
    nbytes = (batch.capacity_bits(*stego.shape, n_ac) + 7) // 8
    middle = [*_structs(stem, given), DELTA, *([n_ac] if STEMS[stem][1] else [])]
    if host:
        out = np.full(nbytes, 0xA5, np.uint8)
        native.check(getattr(lib, "svs_extract" + stem)(stego.ctypes.data, C.byref(planes), *middle, out.ctypes.data, nbytes, flags,
                                                        C.byref(got)), "svs_extract" + stem)
        return out, got.value
    d_gray, d_out = _Dev(stego.nbytes), _Dev(nbytes + 8)
    d_gray.put(stego)
    native.check(getattr(lib, f"svs_extract{stem}_dev")(d_gray.ptr, C.byref(planes), *middle, d_out.ptr, nbytes, flags, C.byref(got),
                                                        None), f"svs_extract{stem}_dev")
    return d_out.get(nbytes), got.value


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


CASES = [(shape, n_ac, flags) for shape in ((3, 16, 24), (3, 16, 32)) for n_ac in (3, 10, 20)
         for flags in (G, P, G | native.SVS_MINMOVE)]


@pytest.mark.parametrize("shape,n_ac,flags", CASES, ids=[f"{s[2]}-n{n}-0x{f:x}" for s, n, f in CASES])
def test_device_forms_of_one_call_agree(chunked_experiments_library, shape, n_ac, flags):
    lib, cover = chunked_experiments_library, cover_of(shape)
    prefix = coeffs.native_coeffs(range(1, n_ac + 1))
    zigzag = coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))
    dev = lambda stem, **given: embed(lib, stem, False, cover, n_ac, flags, **given)   # noqa: E731

    plain = dev("")
    assert plain[1] == batch.capacity_bits(*shape, n_ac) - 5
    assert same(plain, dev("_ordered")) and same(plain, dev("_select", coeffs=prefix))
    bits = extract(lib, "", False, plain[0], n_ac, flags & (G | P))
    assert same(bits, extract(lib, "_ordered", False, plain[0], n_ac, flags & (G | P)))
    assert same(bits, extract(lib, "_select", False, plain[0], n_ac, flags & (G | P), coeffs=prefix))

    for order in (None, ORDER):
        readback = dev("_readback", order=order)
        print(f"{shape} n_ac {n_ac} flags 0x{flags:x} order {order is not None}: read-back counts {readback[2]}")
        assert same(readback, dev("_dithered_readback", order=order))
    assert same(dev("_ordered", order=ORDER), dev("_select", order=ORDER, coeffs=prefix))

    # a cover that does not clip: nothing to repair, and the read-back call reports the bytes of the call without it
    calm = cover_of(shape, clipping=False)
    keyed = dict(order=ORDER, coeffs=zigzag, dither=DITHER)
    stego, used, _ = embed(lib, "_dithered", False, calm, n_ac, flags, **keyed)
    assert same((stego, used, (0, 0)), embed(lib, "_dithered_readback", False, calm, n_ac, flags, **keyed))


@pytest.mark.parametrize("shape,n_ac,flags", CASES, ids=[f"{s[2]}-n{n}-0x{f:x}" for s, n, f in CASES])
def test_host_calls_in_chunks_equal_one_device_call(chunked_experiments_library, shape, n_ac, flags):
    """every embed and extract family; order and dither at first_frame = 5, so the later chunks' first_frame + f0 has f0 > 0"""
    lib, cover = chunked_experiments_library, cover_of(shape)
    zigzag = coeffs.native_coeffs(coeffs.selection("zigzag", n_ac))
    keyed = dict(order=ORDER, coeffs=zigzag, dither=DITHER)
    families = {"": {}, "_ordered": dict(order=ORDER), "_select": dict(order=ORDER, coeffs=zigzag), "_dithered": keyed,
                "_readback": dict(order=ORDER), "_dithered_readback": keyed}
    for stem, given in families.items():
        on_device = embed(lib, stem, False, cover, n_ac, flags, **given)
        assert same(on_device, embed(lib, stem, True, cover, n_ac, flags, **given)), stem
        if not STEMS[stem][2]:
            bits = extract(lib, stem, False, on_device[0], n_ac, flags & (G | P), **given)
            assert bits[1] == batch.capacity_bits(*shape, n_ac)
            assert same(bits, extract(lib, stem, True, on_device[0], n_ac, flags & (G | P), **given)), stem
