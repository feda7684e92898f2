"""SVS_READBACK, CPU tier: the reference's own stego fails to read back on clipping content (the motivating failure), a NumPy
model of the repair fixes it, and the host build of csrc/svs_readback.hpp - the arithmetic readback_kernel runs - equals that
model byte for byte and keeps the flag's contract on the content classes, the guard corpus and a keyed order.  The flag is
routed by the gray embed calls only: extract and colour calls refuse it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fakes
from oracle import qim_dct_oracle as orc
from readback_lib import (CLIPPING, KINDS, SETTINGS, content, failing_blocks, host_readback, model_repair, oracle_stego,
                          payload)
from testlib import REPO, guard_corpus_case
from test_pipeline import _install, _make_inputs
from svsdct import batch, native, order
from svsdct.pipeline import FramePipeline

GOLDEN = os.path.join(REPO, "tests", "golden")


def _case(kind, delta, n_ac, fill=1.0):
    g = content(kind)
    cap = (g.shape[0] // 8) * (g.shape[1] // 8) * n_ac
    bits = payload(int(cap * fill))
    return g, bits, oracle_stego(g, delta, n_ac, bits)


def test_motivating_failure_letterbox_does_not_read_back():
    """the oracle's stego of a letterboxed frame at the GUI's default (delta 20, n 10) loses bits in its bars"""
    g, bits, stego = _case("letterbox", 20, 10)
    assert failing_blocks(stego, bits, 20, 10).sum() > 300
    assert not np.array_equal(orc.frame_extract_bits(stego, 20, 10)[: bits.size], bits)


@pytest.mark.parametrize("delta,n_ac", [(20, 10), (8, 3), (16, 10)])
def test_numpy_model_repairs_clipping_classes(delta, n_ac):
    for kind in CLIPPING:
        g, bits, stego = _case(kind, delta, n_ac)
        out, (rep, left) = model_repair(stego, bits, delta, n_ac)
        assert left == 0, kind
        assert rep == failing_blocks(stego, bits, delta, n_ac).sum()
        assert np.array_equal(orc.frame_extract_bits(out, delta, n_ac)[: bits.size], bits), kind


def _check_contract(stego, out, counts, status, bits, delta, n_ac, blocks_of=lambda a: orc._blocks_view(a).reshape(-1, 8, 8),
                    bad_of=None):
    """the flag's contract, block by block, on one frame (status: 0 reads back, 1 repaired, 2 left, 3 no payload)"""
    bad0 = (bad_of or failing_blocks)(stego, bits, delta, n_ac)
    bad1 = (bad_of or failing_blocks)(out, bits, delta, n_ac)
    b0, b1 = blocks_of(stego), blocks_of(out)
    nblk = bad0.size
    same = np.all(b0 == b1, axis=(1, 2))
    assert np.array_equal(status[:nblk] == 0, ~bad0)                    # what reads back is recognised as such ...
    assert same[:nblk][~bad0].all() and same[nblk:].all()               # ... and untouched; no byte past the budget moves
    assert (status[nblk:] == 3).all()
    assert not bad1[status[:nblk] == 1].any()                           # every repaired block reads back under the oracle
    assert same[:nblk][status[:nblk] == 2].all()                        # unrepaired blocks are the oracle's stego
    assert counts == (int((status == 1).sum()), int((status == 2).sum()))
    assert counts[0] + counts[1] == int(bad0.sum())
    assert np.array_equal(bad1, status[:nblk] == 2)


@pytest.mark.parametrize("delta,n_ac", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_readback_keeps_the_contract(kind, delta, n_ac):
    g, bits, stego = _case(kind, delta, n_ac)
    out, counts, status = host_readback(stego, delta, n_ac, bits)
    _check_contract(stego, out, counts, status, bits, delta, n_ac)
    model, model_counts = model_repair(stego, bits, delta, n_ac)
    assert np.array_equal(out, model) and counts == model_counts     # the compiled search is the NumPy model's, bit for bit
    if kind in CLIPPING and delta >= 8 and n_ac <= 15:
        assert counts[1] == 0
    if kind in ("noise", "natural") and (delta, n_ac) in ((20, 10), (8, 3), (16, 10)):
        assert counts == (0, 0) and np.array_equal(out, stego)


@pytest.mark.parametrize("kind", ["letterbox", "noise"])
def test_host_readback_budget_ends_inside_a_block(kind):
    """a budget that ends inside a block: only that block's first bits are checked, blocks past it are not touched"""
    delta, n_ac = 20, 10
    g = content(kind)
    bits = payload(4567)
    stego = oracle_stego(g, delta, n_ac, bits)
    out, counts, status = host_readback(stego, delta, n_ac, bits)
    _check_contract(stego, out, counts, status, bits, delta, n_ac)
    assert (status == 3).sum() == status.size - 457


def test_host_readback_on_the_guard_corpus():
    arrays = np.load(os.path.join(GOLDEN, "guard_corpus.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "guard_corpus.json")))
    assert meta["embed"]
    for name, m in meta["embed"].items():
        case = guard_corpus_case(arrays, meta, name)
        frame, bits, delta, n_ac = case["frame"], case["bits"], m["delta"], m["n_ac"]
        stego = oracle_stego(frame, delta, n_ac, bits)
        out, counts, status = host_readback(stego, delta, n_ac, bits)
        _check_contract(stego, out, counts, status, bits, delta, n_ac)


def test_host_readback_keyed_order():
    """slot j of frame t is block sigma_t(j): the read-back checks each block against its slot's bits"""
    delta, n_ac, key, first = 20, 10, 0x0123456789ABCDEF, 5
    g = content("letterbox")[None]
    cap = (g.shape[1] // 8) * (g.shape[2] // 8) * n_ac
    bits = payload(cap // 2)
    stego, _ = orc.batch_embed(order.permute_blocks(g, key, first), delta, bits, n_ac)
    stego = order.unpermute_blocks(stego, key, first)
    out, counts, status = host_readback(stego, delta, n_ac, bits, block_key=key, first_frame=first)
    assert counts[0] > 50 and counts[1] == 0
    perm = lambda a: order.permute_blocks(a[None], key, first)[0]
    status_slots = status[order.slot_to_block(key, first, status.size)]
    _check_contract(perm(stego[0]), perm(out[0]), counts, status_slots, bits, delta, n_ac)


# ---- routing and validation ---------------------------------------------------------------------------------------------
def test_flag_value_header_and_binding():
    text = open(os.path.join(REPO, "include", "svsdct.h")).read()
    assert "#define SVS_READBACK 0x200u" in text and native.SVS_READBACK == 0x200
    assert native.SVS_READBACK & (native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED | native.SVS_KEEP_COLOUR) == 0
    assert "typedef struct svs_readback_counts" in text
    lib = native.load()
    for name in ("svs_embed_readback_dev", "svs_embed_readback"):
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert native.SIGNATURES["svs_embed_readback"][1][-1] is C.POINTER(native.ReadbackCounts)


def test_extract_and_colour_calls_refuse_the_flag():
    """refused before any device work, so this runs without a GPU"""
    lib = native.load()
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    gray = np.zeros((f, h, w), np.uint8)
    bgr = np.zeros((f, h, w, 3), np.uint8)
    out = np.zeros(64, np.uint8)
    got = C.c_uint64(0)
    flag = native.SVS_READBACK | native.SVS_EXACT_GUARDED
    P = C.byref(planes)
    bad = native.SVS_ERR_INVALID_ARG
    assert lib.svs_extract(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)) == bad
    assert lib.svs_extract_dev(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None) == bad
    assert lib.svs_extract_ordered(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)) == bad
    assert lib.svs_extract_ordered_dev(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got),
                                       None) == bad
    chars = np.zeros(64, np.uint8)
    assert lib.svs_extract_str(gray.ctypes.data, P, 8.0, n_ac, chars.ctypes.data, chars.size, flag, C.byref(got)) == bad
    bits = np.zeros(16, np.uint8)
    assert lib.svs_embed_bgr(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8, flag,
                             C.byref(got)) == bad
    assert lib.svs_embed_bgr_dev(bgr.ctypes.data, 3 * w, 3 * w * h, bgr.ctypes.data, 3 * w, 3 * w * h, None, P, None, 8.0,
                                 n_ac, bits.ctypes.data, 0, 8, flag, C.byref(got), None) == bad
    assert b"SVS_READBACK" in lib.svs_last_error() or b"unknown flags" in lib.svs_last_error()


def test_python_surface():
    import inspect
    assert inspect.signature(batch.embed_frames).parameters["readback"].default is False
    assert inspect.signature(batch.embed_device).parameters["readback"].default is False
    assert inspect.signature(FramePipeline).parameters["readback"].default is False
    assert batch.ReadbackCounts(1, 2).repaired == 1


def test_drop_in_refuses_readback_with_fused_colour(monkeypatch, tmp_path):
    emb, _ = _install(monkeypatch, "emu")
    _, _, secret_path = _make_inputs(tmp_path, n_frames=2, size=(16, 16))
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    monkeypatch.setattr(emb, "READBACK", True)
    for name in ("FUSED_COLOUR", "KEEP_COLOUR"):
        monkeypatch.setattr(emb, name, True)
        with pytest.raises(ValueError, match="SVS_READBACK"):
            emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)
        monkeypatch.setattr(emb, name, False)


def _ac_rms_change(a, b):
    d = (orc._blocks_view(a.astype(np.float64)) - orc._blocks_view(b.astype(np.float64))).reshape(-1, 64)
    return np.sqrt(((d - d.mean(1, keepdims=True)) ** 2).mean(1))


@pytest.mark.parametrize("delta,n_ac", SETTINGS)
def test_distortion_of_accepted_repairs(delta, n_ac):
    """what the repair costs in the AC of a block (the DC shift off 0 / 255 excluded): at delta >= 8 every accepted block
    stays within 12 grey levels RMS of the reference's; at delta = 4 the over-relaxed search can overshoot and a few accepted
    blocks per frame are far from it - the residual class the documentation names"""
    far = 0
    for kind in KINDS:
        g, bits, stego = _case(kind, delta, n_ac)
        out, counts, status = host_readback(stego, delta, n_ac, bits)
        ac = _ac_rms_change(out, stego)[status == 1]
        if delta >= 8:
            assert ac.size == 0 or ac.max() < 12, kind
        far += int((ac > 10).sum())
    assert far <= (40 if delta < 8 else 25)
