"""GPU tier of the guard-sensitivity checks (CPU tier: test_guard_sensitivity_cpu.py): on the frames of
tests/golden/guard_corpus.npz, whose corpus blocks sit at the boundary of the streaming kernels' guard (BETA) and of FAST
extraction's tie margin, the kernels make the decisions hostemu makes.

* product library, guarded and default mode, in place too: the oracle's pixels;
* experiments library, SVS_GUARD_SCALE = 1: the same bytes, and as many blocks replayed as hostemu replays;
* SVS_GUARD_SCALE = 0.9 x max s*: NOT the oracle's pixels - hostemu's at that scale, in the same blocks, same replay count;
* the fused colour path (B = G = R) at the same three points;
* extraction (gray and BGR): SVS_TIE_SCALE = 1 gives the oracle's bits, 0.9 x max t* the bits hostemu predicts when it
  takes step two per wave of 64 blocks, as the kernels do."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from testlib import REPO, emu_embed, emu_extract, emu_scales, guard_corpus_case, experiments_library, using_library
from oracle import qim_dct_oracle as orc
from svsdct import batch, native
from svsdct.native import Planes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(REPO, "tests", "golden")
META = json.load(open(os.path.join(GOLDEN, "guard_corpus.json")))
EMBED = sorted(META["embed"])
EXTRACT = sorted(META["extract"])


@pytest.fixture(scope="module")
def corpus():
    native.ensure_device(0)
    return np.load(os.path.join(GOLDEN, "guard_corpus.npz"))


def embed_case(corpus, name):
    c = guard_corpus_case(corpus, META, name)
    return META["embed"][name], c["frame"], c["bits"], c["positions"], c["stars"]


def differing_blocks(a, b):
    h, w = a.shape[-2:]
    d = (a.reshape(-1, h // 8, 8, w // 8, 8) != b.reshape(-1, h // 8, 8, w // 8, 8)).any(axis=(2, 4))
    return np.flatnonzero(d.reshape(-1))


def in_place(frame, delta, n, bits):
    """the product library's default mode through the device-pointer level, stego written over the frame"""
    lib = native.load()
    packed = batch.pack_bits(bits)
    d_fr, d_bits = C.c_void_p(), C.c_void_p()
    native.check(lib.svs_malloc(C.byref(d_fr), frame.nbytes), "malloc")
    native.check(lib.svs_malloc(C.byref(d_bits), packed.nbytes), "malloc")
    try:
        native.check(lib.svs_memcpy_h2d(d_fr, frame.ctypes.data, frame.nbytes, None), "h2d")
        native.check(lib.svs_memcpy_h2d(d_bits, packed.ctypes.data, packed.nbytes, None), "h2d")
        planes = Planes.contiguous(1, *frame.shape)
        assert batch.embed_device(d_fr.value, d_fr.value, planes, delta, n, d_bits.value, 0, bits.size) == bits.size
        out = np.empty_like(frame)
        native.check(lib.svs_memcpy_d2h(out.ctypes.data, d_fr, out.nbytes, None), "d2h")
        native.check(lib.svs_stream_synchronize(None), "sync")
    finally:
        lib.svs_free(d_fr)
        lib.svs_free(d_bits)
    return out


class counting:
    """`with counting(exp) as c:` - the experiments library's replay counter around the block; c.value afterwards"""

    def __init__(self, exp):
        self.exp, self.d = exp, C.c_void_p()
        native.check(exp.svs_malloc(C.byref(self.d), 8), "malloc")

    def __enter__(self):
        native.check(self.exp.svs_memset(self.d, 0, 8, None), "memset")
        native.check(self.exp.svs_stream_synchronize(None), "sync")
        self.exp.svs_guard_counter_set(self.d)
        return self

    def __exit__(self, *exc):
        self.exp.svs_guard_counter_set(None)
        out = np.zeros(1, np.uint64)
        native.check(self.exp.svs_memcpy_d2h(out.ctypes.data, self.d, 8, None), "d2h")
        native.check(self.exp.svs_stream_synchronize(None), "sync")
        native.check(self.exp.svs_free(self.d), "free")
        self.value = int(out[0])
        return False


@pytest.mark.parametrize("name", EMBED)
def test_embed_guard_decisions_match_hostemu(corpus, name, monkeypatch):
    m, frame, bits, positions, stars = embed_case(corpus, name)
    n, delta, x = m["n_ac"], m["delta"], m["test_scale"]
    ref, used = orc.batch_embed(frame[None], delta, bits, n)
    assert used == bits.size
    rep1 = []
    emu1, _ = emu_embed(frame, delta, n, bits, exact=4, replayed=rep1)
    assert np.array_equal(emu1, ref)
    rep_x = []
    with emu_scales(guard=x):
        emu_x, _ = emu_embed(frame, delta, n, bits, exact=4, replayed=rep_x)
    want_blocks = np.sort(positions[stars >= np.float32(x)])
    assert np.array_equal(differing_blocks(emu_x, ref), want_blocks) and want_blocks.size

    # product library: guarded, default and exact mode, in place
    for mode in ("guarded", None, "exact"):
        got, u = batch.embed_frames(frame[None], delta, n, bits, mode=mode)
        assert u == bits.size and np.array_equal(got, ref), (name, mode)
    assert np.array_equal(in_place(frame, delta, n, bits), ref[0]), name

    # fused colour path, B = G = R: gray is the plane itself with the default weights
    bgr = np.repeat(frame[None, ..., None], 3, axis=3)
    got_bgr, got_gray, u = batch.embed_bgr_frames(bgr, delta, n, bits)
    assert u == bits.size and np.array_equal(got_gray[0], frame)
    assert np.array_equal(got_bgr, np.repeat(ref[..., None], 3, axis=3)), name

    exp = experiments_library()
    with using_library(exp):
        for scale, want, rep in (("1", ref, rep1[0]), (repr(x), emu_x, rep_x[0])):
            monkeypatch.setenv("SVS_GUARD_SCALE", scale)
            with counting(exp) as c:
                got, _ = batch.embed_frames(frame[None], delta, n, bits, mode="guarded")
            assert np.array_equal(differing_blocks(got, ref), differing_blocks(want, ref)), (name, scale)
            assert np.array_equal(got, want), (name, scale)
            assert c.value == rep, (name, scale, c.value, rep)
            got_bgr, _, _ = batch.embed_bgr_frames(bgr, delta, n, bits, mode="guarded")
            assert np.array_equal(got_bgr, np.repeat(want[..., None], 3, axis=3)), (name, scale, "bgr")
        monkeypatch.delenv("SVS_GUARD_SCALE")


@pytest.mark.parametrize("name", EXTRACT)
def test_extract_tie_decisions_match_hostemu(corpus, name, monkeypatch):
    m = META["extract"][name]
    c = guard_corpus_case(corpus, META, name)
    frame, positions, stars = c["frame"], c["positions"], c["stars"]
    n, delta, x = m["n_ac"], m["delta"], m["test_scale"]
    ref = orc.batch_extract_bits(frame[None], delta, n)
    with emu_scales(tie=x):
        emu_x = emu_extract(frame, delta, n, wave=64)     # step two per wave of 64 blocks, as the kernels take it
    wrong = np.flatnonzero((emu_x != ref).reshape(-1, n).any(1))
    assert wrong.size and np.isin(wrong, positions[stars >= np.float32(x)]).all()
    bgr = np.repeat(frame[None, ..., None], 3, axis=3)

    def both():
        p, nb = batch.extract_frames(frame[None], delta, n, mode="fast")
        q, nq = batch.extract_bgr_frames(bgr, delta, n)
        return np.unpackbits(p, count=nb), np.unpackbits(q, count=nq)

    for got in both():
        assert np.array_equal(got, ref), name
    exp = experiments_library()
    with using_library(exp):
        for scale, want in (("1", ref), (repr(x), emu_x)):
            monkeypatch.setenv("SVS_TIE_SCALE", scale)
            for kind, got in zip(("gray", "bgr"), both()):
                assert np.array_equal(got, want), (name, scale, kind, np.flatnonzero((got != want).reshape(-1, n).any(1))[:8])
        monkeypatch.delenv("SVS_TIE_SCALE")
