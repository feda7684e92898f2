"""Read-back and repair under a coefficient selection and a keyed dither (svs_embed_dithered_readback*), CPU tier: the keyed
forms of csrc/svs_readback.hpp built for the host (tests/hostemu) are today's read-back with the prefix table and no
dither, equal a NumPy model bit for bit on the content / delta / selection rows that motivated them, keep SVS_READBACK's
contract, pair the dither with a block's physical position and the bits with its slot, and are routed by new calls only: the
select and dithered calls keep refusing SVS_READBACK."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import dither_lib
import fakes
import keyed_readback_lib as kl
import readback_lib as rl
from oracle import qim_dct_oracle as orc
from test_pipeline import _install, _make_inputs
from testlib import REPO
from svsdct import batch, native, order, pipeline

INVALID = native.SVS_ERR_INVALID_ARG
KEY = kl.DITHER_KEY
NEW = ("svs_embed_dithered_readback_dev", "svs_embed_dithered_readback")


# ---- identity: the prefix table without a dither is today's read-back -------------------------------------------------------
@pytest.mark.parametrize("delta,n_ac", rl.SETTINGS)
@pytest.mark.parametrize("kind", rl.KINDS)
def test_prefix_table_without_dither_is_todays_readback(kind, delta, n_ac):
    g = rl.content(kind)
    bits = rl.payload((g.shape[0] // 8) * (g.shape[1] // 8) * n_ac)
    stego = rl.oracle_stego(g, delta, n_ac, bits)
    want, want_counts, want_status = rl.host_readback(stego, delta, n_ac, bits)
    got, counts, status = kl.host_readback(stego, delta, n_ac, bits)
    assert np.array_equal(got, want) and counts == want_counts and np.array_equal(status, want_status)
    got, counts, status = kl.host_readback(stego, delta, n_ac, bits, index=kl.prefix(n_ac))      # the prefix as a selection
    assert np.array_equal(got, want) and counts == want_counts and np.array_equal(status, want_status)


# ---- the table: host build == NumPy model -----------------------------------------------------------------------------------
def _check_contract(stego, out, counts, status_slots, bits, delta, index, key, t, perm=None):
    """SVS_READBACK's contract under the receiver's own verdict (model_extract), slot by slot on one frame.  status_slots: the
    status in SLOT order (0 reads back, 1 repaired, 2 left, 3 no payload)"""
    n_blocks = status_slots.size
    where = np.arange(n_blocks) if perm is None else np.asarray(perm)
    bad0 = kl.failing_slots(stego, bits, delta, index, key, t, perm)
    bad1 = kl.failing_slots(out, bits, delta, index, key, t, perm)
    blocks = lambda a: orc._blocks_view(a).reshape(-1, 8, 8)[where]        # noqa: E731  blocks in slot order
    same = np.all(blocks(stego) == blocks(out), axis=(1, 2))
    nslot = bad0.size
    assert np.array_equal(status_slots[:nslot] == 0, ~bad0)                # what reads back is recognised as such ...
    assert same[:nslot][~bad0].all() and same[nslot:].all()                # ... and untouched; no byte past the budget moves
    assert (status_slots[nslot:] == 3).all()
    assert not bad1[status_slots[:nslot] == 1].any()                       # every repaired block reads back
    assert same[:nslot][status_slots[:nslot] == 2].all()                   # unrepaired blocks keep their bytes
    assert counts == (int((status_slots == 1).sum()), int((status_slots == 2).sum()))
    assert counts[0] + counts[1] == int(bad0.sum())
    assert np.array_equal(bad1, status_slots[:nslot] == 2)
    return int(bad0.sum())


@pytest.mark.parametrize("rule", ("reference", "minmove"))
@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
@pytest.mark.parametrize("row", range(len(kl.TABLE)), ids=[f"{k}-{d}-{len(i)}@{i[0]}" for k, d, i in kl.TABLE])
def test_host_build_equals_the_numpy_model(row, dither, rule):
    kind, delta, index = kl.TABLE[row]
    bits, stego, key = kl.table_case(kind, delta, index, dither, rule)
    assert bits.size == 240 * len(index) - 7                                # the budget ends inside a block
    model, model_counts = kl.model_repair(stego, bits, delta, index, key, kl.TABLE_T)
    out, counts, status = kl.host_readback(stego, delta, len(index), bits, index=index, dither_key=key, first_frame=kl.TABLE_T)
    failing = _check_contract(stego, out, counts, status, bits, delta, index, key, kl.TABLE_T)
    print(f"{kind}, delta {delta}, {len(index)} from {index[0]}, dither {dither}, {rule}: {failing} -> {counts[1]}")
    assert np.array_equal(out, model) and counts == model_counts           # bit for bit
    if kind in rl.CLIPPING:
        assert counts[1] == 0
        got = dither_lib.model_extract(out, delta, index=index, key=key, t=kl.TABLE_T)[: bits.size]
        assert np.array_equal(got, bits)                                   # the receiver gets every payload bit


def test_the_motivating_failure():
    """the dithered stego of a letterboxed frame does not decode under svs_extract_dithered's arithmetic; after the pass it does"""
    _, delta, index = kl.TABLE[1]
    bits, stego, key = kl.table_case("letterbox", delta, index, True, "minmove")
    assert kl.failing_slots(stego, bits, delta, index, key, kl.TABLE_T).sum() > 40
    out, counts, _ = kl.host_readback(stego, delta, len(index), bits, index=index, dither_key=key, first_frame=kl.TABLE_T)
    assert counts[0] > 40 and counts[1] == 0
    assert np.array_equal(dither_lib.model_extract(out, delta, index=index, key=key, t=kl.TABLE_T)[: bits.size], bits)


@pytest.mark.parametrize("kind", ("letterbox", "noise"))
def test_budget_ends_inside_a_block_in_the_middle_of_the_frame(kind):
    delta, index = 20, kl.zigzag(10)
    g = kl.table_frame(kind)
    bits = dither_lib.payload(1234)                                         # 124 blocks, the last one takes 4 bits
    stego, _ = dither_lib.model_embed(g, delta, bits, index=index, key=KEY, t=kl.TABLE_T)
    out, counts, status = kl.host_readback(stego, delta, 10, bits, index=index, dither_key=KEY, first_frame=kl.TABLE_T)
    _check_contract(stego, out, counts, status, bits, delta, index, KEY, kl.TABLE_T)
    assert (status == 3).sum() == status.size - 124
    # a bit offset and a budget shorter than the buffer: the call's own stream range
    padded = np.concatenate([dither_lib.payload(45, seed=9), bits, dither_lib.payload(77, seed=8)])
    out2, counts2, status2 = kl.host_readback(stego, delta, 10, padded, index=index, dither_key=KEY, first_frame=kl.TABLE_T,
                                              bit_offset=45, n_bits=bits.size)
    assert np.array_equal(out2, out) and counts2 == counts and np.array_equal(status2, status)


def test_keyed_order_dither_of_the_position_bits_of_the_slot():
    delta, index, okey, t = 20, kl.zigzag(10), 0x5EED, 5
    g = kl.table_frame("letterbox")
    n_blocks = (g.shape[0] // 8) * (g.shape[1] // 8)
    perm = order.slot_to_block(okey, t, n_blocks)
    bits = dither_lib.payload(n_blocks * 10 // 2 + 3)
    stego, _ = dither_lib.model_embed(g, delta, bits, index=index, key=KEY, t=t, perm=perm, rule="minmove")
    out, counts, status = kl.host_readback(stego, delta, 10, bits, index=index, dither_key=KEY, block_key=okey, first_frame=t)
    assert counts[0] > 10 and counts[1] == 0
    _check_contract(stego, out, counts, status[perm], bits, delta, index, KEY, t, perm)
    model, model_counts = kl.model_repair(stego, bits, delta, index, KEY, t, perm)
    assert np.array_equal(out, model) and counts == model_counts
    assert np.array_equal(dither_lib.model_extract(out, delta, index=index, key=KEY, t=t, perm=perm)[: bits.size], bits)
    # the two pairings differ: the pass in raster order, or with another frame's dither, repairs other blocks
    other, other_counts, _ = kl.host_readback(stego, delta, 10, bits, index=index, dither_key=KEY, first_frame=t)
    assert not np.array_equal(other, out)
    shifted, _, _ = kl.host_readback(stego, delta, 10, bits, index=index, dither_key=KEY, block_key=okey, first_frame=t + 1)
    assert not np.array_equal(shifted, out)


# ---- the C ABI's argument checks (no GPU: empty batches, NULL pointers) ---------------------------------------------------------
def _calls(dith=None, order=None, coeffs=None, flags=0, n_frames=0):
    lib = native.load()
    planes = native.Planes.contiguous(n_frames, 8, 8)
    done = C.c_uint64(7)
    counts = native.ReadbackCounts(5, 5)
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    return (lib.svs_embed_dithered_readback_dev(None, None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0,
                                                8, flags, C.byref(done), None, None),
            lib.svs_embed_dithered_readback(None, None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0, 8,
                                            flags, C.byref(done), C.byref(counts)))


def _error():
    return native.load().svs_last_error().decode()


def test_new_calls_check_their_arguments():
    good = native.Dither(KEY, 5, 0)
    sel = native.Coeffs(3, (C.c_uint8 * 63)(9, 2, 17))
    assert _calls() == (0, 0)                                              # order, coeffs and dither may each be NULL
    assert _calls(good) == (0, 0) and _calls(coeffs=sel) == (0, 0) and _calls(good, coeffs=sel) == (0, 0)
    assert _calls(good, order=native.BlockOrder(9, 5, 0), coeffs=sel) == (0, 0)
    assert _calls(order=native.BlockOrder(9, 4, 0)) == (0, 0)               # no dither: no first_frame to agree with
    assert _calls(native.Dither(KEY, 5, 1)) == (INVALID,) * 2 and "reserved" in _error()
    assert _calls(good, order=native.BlockOrder(9, 4, 0)) == (INVALID,) * 2 and "first_frame" in _error()
    assert _calls(good, order=native.BlockOrder(9, 5, 1)) == (INVALID,) * 2
    for bad in (native.Coeffs(2, (C.c_uint8 * 63)(9, 9)), native.Coeffs(1, (C.c_uint8 * 63)(0,)),
                native.Coeffs(64, (C.c_uint8 * 63)(*range(1, 64))), native.Coeffs(1, (C.c_uint8 * 63)(5, 6))):
        assert _calls(good, coeffs=bad) == (INVALID,) * 2 and "svs_coeffs" in _error()
        assert _calls(coeffs=bad) == (INVALID,) * 2
    # with a frame to work on the checks still come first: no pointer is looked at, no device is needed
    assert _calls(native.Dither(KEY, 5, 7), n_frames=1) == (INVALID,) * 2 and "reserved" in _error()


def test_new_calls_flags():
    good = native.Dither(KEY, 0, 0)
    for flags in (0, 1, 2, 3, native.SVS_NEAREST, native.SVS_MINMOVE, native.SVS_READBACK,
                  native.SVS_READBACK | native.SVS_NEAREST | native.SVS_MINMOVE | 1):
        assert _calls(good, flags=flags) == (0, 0), hex(flags)
        assert _calls(flags=flags) == (0, 0), hex(flags)
    for flags in (native.SVS_KEEP_COLOUR, 0x400, 0x2000, 0x80000000, native.SVS_KEEP_COLOUR | native.SVS_READBACK):
        assert _calls(good, flags=flags) == (INVALID,) * 2, hex(flags)
        assert _calls(good, flags=flags, n_frames=1) == (INVALID,) * 2 and "flags" in _error()   # before any device work
        assert _calls(coeffs=native.Coeffs(3, (C.c_uint8 * 63)(9, 2, 17)), flags=flags) == (INVALID,) * 2


def test_old_calls_still_refuse_the_flag():
    lib = native.load()
    planes = native.Planes.contiguous(0, 8, 8)
    done = C.c_uint64(0)
    sel = native.Coeffs(3, (C.c_uint8 * 63)(9, 2, 17))
    dith = native.Dither(KEY, 0, 0)
    P, S, D = C.byref(planes), C.byref(sel), C.byref(dith)
    for flags in (native.SVS_READBACK, native.SVS_READBACK | native.SVS_MINMOVE):
        assert lib.svs_embed_select_dev(None, None, P, None, S, 8.0, None, 0, 8, flags, C.byref(done), None) == INVALID
        assert lib.svs_embed_select(None, None, P, None, S, 8.0, None, 0, 8, flags, C.byref(done)) == INVALID
        assert lib.svs_embed_dithered_dev(None, None, P, None, None, D, 8.0, 3, None, 0, 8, flags, C.byref(done), None) == INVALID
        assert lib.svs_embed_dithered(None, None, P, None, S, D, 8.0, 3, None, 0, 8, flags, C.byref(done)) == INVALID


def test_header_binding_and_exports_agree():
    raw = open(os.path.join(REPO, "include", "svsdct.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(svs_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared and declared == set(native.SIGNATURES)
    lib = native.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert "#define SVS_ABI_VERSION 4" in text and native.ABI_VERSION == 4
    dev, host = native.SIGNATURES[NEW[0]][1], native.SIGNATURES[NEW[1]][1]
    assert dev[:13] == native.SIGNATURES["svs_embed_dithered_dev"][1][:13] and len(dev) == 15   # + d_counts before stream
    assert host[:13] == native.SIGNATURES["svs_embed_dithered"][1] and host[13] is C.POINTER(native.ReadbackCounts)
    assert raw.count("svs_embed_dithered_readback") >= 4                     # the select / dithered texts point to the new calls
    assert "There is no read-back" not in raw


# ---- the Python layers ----------------------------------------------------------------------------------------------------
class RecordingLibrary:
    """stands in for the loaded library: every entry point returns SVS_OK and is noted"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("svs_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def names(self):
        return [n for n, _ in self.calls if "embed" in n or "extract" in n]


@pytest.fixture
def recorded(monkeypatch):
    lib = RecordingLibrary()
    monkeypatch.setattr(native, "load", lambda: lib)
    monkeypatch.setattr(native, "ensure_device", lambda device=0: None)
    monkeypatch.setattr(batch, "pinned_empty", lambda shape, dtype=np.uint8: np.zeros(shape, dtype))
    monkeypatch.setattr(pipeline, "_pinned", lambda n: (C.c_void_p(1), np.zeros(n, np.uint8)))
    monkeypatch.setattr(pipeline, "_device", lambda n: C.c_void_p(1))
    return lib


def test_python_surface_and_value_errors(monkeypatch):
    for fn in (batch.embed_frames, batch.embed_device, pipeline.FramePipeline.__init__):
        assert inspect.signature(fn).parameters["readback_keyed"].default is False

    def no_library():
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(native, "load", no_library)
    frames, three = np.zeros((1, 8, 8), np.uint8), np.zeros(3, np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    with pytest.raises(ValueError, match="readback_keyed"):
        batch.embed_frames(frames, 8, 3, three, readback=True, readback_keyed=True)
    with pytest.raises(ValueError, match="readback_keyed"):
        batch.embed_device(0, 0, planes, 8, 3, 0, 0, 3, readback=True, readback_keyed=True)
    with pytest.raises(ValueError, match="readback_keyed"):
        pipeline.FramePipeline(8, 8, 1, 8, 3, readback=True, readback_keyed=True)
    # every existing refusal stays
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_frames(frames, 8, 3, three, dither_key=KEY, readback=True)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_device(0, 0, planes, 8, 3, 0, 0, 3, coeffs="zigzag", readback=True)
    with pytest.raises(ValueError, match="read-back"):
        pipeline.FramePipeline(8, 8, 1, 8, 3, coeffs="zigzag", readback=True)


def test_batch_calls(recorded):
    frames, bits = np.zeros((2, 8, 8), np.uint8), np.zeros(6, np.uint8)
    planes = native.Planes.contiguous(2, 8, 8)
    odr = batch.block_order(9, 4)

    def host_call(*a):                                                            # the host call reports its counts
        recorded.calls.append(("svs_embed_dithered_readback", a))
        a[13]._obj.repaired, a[13]._obj.unrepaired = 3, 1
        return 0
    recorded.svs_embed_dithered_readback = host_call
    out = batch.embed_frames(frames, 8, 3, bits, readback_keyed=True, dither_key=KEY, first_frame=4, block_key=9, minmove=True)
    assert out[2] == batch.ReadbackCounts(3, 1) and len(out) == 3
    batch.embed_frames(frames, 8, 3, bits, readback_keyed=True, coeffs=[9, 2, 17])
    batch.embed_frames(frames, 8, 3, bits, readback_keyed=True)                   # neither: the readback call
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, readback_keyed=True, dither_key=KEY, order=odr, d_counts=64)
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, readback_keyed=True, coeffs="zigzag")
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, readback_keyed=True, order=odr)
    assert recorded.names() == ["svs_embed_dithered_readback", "svs_embed_dithered_readback", "svs_embed_readback",
                                "svs_embed_dithered_readback_dev", "svs_embed_dithered_readback_dev", "svs_embed_readback_dev"]
    (_, e), (_, s), _, (_, ed), (_, sd), _ = recorded.calls
    d = e[5]._obj
    assert (d.key, d.first_frame, d.reserved) == (KEY, 4, 0) and e[3]._obj.first_frame == 4 and e[4] is None
    assert e[11] & native.SVS_MINMOVE
    assert s[5] is None and s[3] is None and (s[4]._obj.count, list(s[4]._obj.index[:3])) == (3, [9, 2, 17])
    assert ed[5]._obj.first_frame == 4 and ed[13] == 64 and sd[5] is None and sd[13] is None


def test_pipeline_calls(recorded):
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1, block_key=9, dither_key=KEY, coeffs="zigzag", readback_keyed=True) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0, first_frame=0)
        pipe.submit_embed(0, 2, 6, first_frame=2)
        assert pipe.readback_counts() == batch.ReadbackCounts(0, 0)
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1, readback_keyed=True) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0)
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0)
        with pytest.raises(RuntimeError):
            pipe.readback_counts()
    calls = [(n, a) for n, a in recorded.calls if "embed" in n]
    assert [n for n, _ in calls] == ["svs_embed_dithered_readback_dev"] * 2 + ["svs_embed_readback_dev", "svs_embed_dev"]
    assert [(a[3]._obj.first_frame, a[5]._obj.first_frame) for _, a in calls[:2]] == [(0, 0), (2, 2)]
    assert all(a[13] for _, a in calls[:2]) and calls[2][1][11]                 # the counts buffer goes along


# ---- the drop-in loop ---------------------------------------------------------------------------------------------------------
class _RecordingPipeline(fakes.EmuFramePipeline):
    """the emulated pipeline of tests/fakes.py; it notes the keywords it was built with"""
    built = []

    def __init__(self, *a, **kw):
        known = {k: kw.pop(k) for k in ("block_key", "dither_key", "coeffs", "nearest", "minmove", "readback", "readback_keyed")
                 if k in kw}
        super().__init__(*a, **kw)
        _RecordingPipeline.built.append(known)

    def submit_embed(self, slot, n_frames, bit_offset, **kw):
        return super().submit_embed(slot, n_frames, bit_offset)

    def readback_counts(self):
        return batch.ReadbackCounts(7, 0)


def test_drop_in_switch(monkeypatch, tmp_path, capsys):
    emb, _ = _install(monkeypatch, "emu")
    monkeypatch.setattr(emb, "FramePipeline", _RecordingPipeline)
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY"):
        monkeypatch.delenv(name, raising=False)
    for name in ("READBACK", "READBACK_COLOUR", "FUSED_COLOUR", "KEEP_COLOUR"):
        monkeypatch.setattr(emb, name, False)
    _, _, secret_path = _make_inputs(tmp_path, n_frames=5, size=(64, 96))
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())

    def run():
        _RecordingPipeline.built = []
        capsys.readouterr()
        assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)[0]
        return _RecordingPipeline.built, capsys.readouterr().out

    assert emb.READBACK_KEYED is False
    built, out = run()
    assert built == [{}] and "Read-back" not in out                          # unset: today's calls
    monkeypatch.setattr(emb, "READBACK_KEYED", True)
    monkeypatch.setenv("SVS_DITHER_KEY", "0x10")
    monkeypatch.setenv("SVS_COEFFS", "zigzag")
    monkeypatch.setenv("SVS_BLOCK_KEY", "7")
    monkeypatch.setattr(emb, "MINMOVE", True)
    built, out = run()
    assert built[0]["readback_keyed"] is True and "readback" not in built[0]
    assert built[0]["dither_key"] == 16 and built[0]["block_key"] == 7 and len(built[0]["coeffs"]) == 10 and built[0]["minmove"]
    assert "Read-back: 7 blok diperbaiki, 0 blok tidak dapat diperbaiki." in out   # lapor_readback
    for other in ("READBACK", "READBACK_COLOUR"):
        monkeypatch.setattr(emb, other, True)
        for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY"):
            monkeypatch.delenv(name, raising=False)
        with pytest.raises(ValueError, match="SVS_READBACK_KEYED"):
            emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "y"), 20, 10, pub)
        monkeypatch.setattr(emb, other, False)
    # the existing refusals stay: a dither key with SVS_READBACK
    monkeypatch.setattr(emb, "READBACK_KEYED", False)
    monkeypatch.setattr(emb, "READBACK", True)
    monkeypatch.setenv("SVS_DITHER_KEY", "0x10")
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "z"), 20, 10, pub) == (False, None, None)
    assert "SVS_DITHER_KEY tidak dapat dipakai bersama" in capsys.readouterr().out


# ---- registers ------------------------------------------------------------------------------------------------------------------
def test_resources_file():
    """profiles/keyed_readback_resources.txt (cross-compiled): every readback_kernel instantiation, before -> after"""
    text = open(os.path.join(REPO, "profiles", "keyed_readback_resources.txt")).read()
    rows = re.findall(r"^(readback_kernel<[^>]*>)\s+(\d+) ->\s+(\d+)\s+(\d+) ->\s+(\d+)\s+(\d+) ->\s+(\d+)\s+(\d+) ->\s+(\d+)\s+(\d+) ->\s+(\d+)$",
                      text, flags=re.M)
    names = {r[0] for r in rows}
    want = {f"readback_kernel<{u}, {qm}, {k}>" for u in (1, 2, 8) for qm in (0, 1, 2) for k in ("false", "true, svs::BlockOrderArgs")}
    assert names == want and len(rows) == 18
    for name, v0, v1, s0, s1, sc0, sc1, w0, w1, l0, l1 in rows:
        assert int(sc0) == 0 and int(sc1) == 0, name                           # no scratch
        assert int(w1) == int(w0), name                                        # the waves per SIMD of the parent
        assert int(l1) <= 20 * 1024, name                                      # eight workgroups per CU of 160 KB
        assert int(w1) == min(8, 512 // (-(-int(v1) // 8) * 8)), name          # the table is consistent with itself
