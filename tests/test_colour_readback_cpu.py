"""Read-back and repair for the fused colour embed (svs_embed_bgr_readback*, include/svsdct.h), CPU tier: the two calls exist
in header, binding and library and validate their arguments before any device work; the Python surface and the drop-in's
SVS_READBACK_COLOUR switch; and the NumPy model of the contract (tests/colour_readback_lib.py) - the GPU tier's expectation -
keeps the contract's own properties on colour covers of the content classes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fakes
from colour_readback_lib import (CLIPPING, KINDS, MAIN_SETTINGS, SETTINGS, W14, W15, colour_content, colour_frames, model)
from oracle import qim_dct_oracle as orc
from readback_lib import host_readback, payload
from test_keep_colour_cpu import gray_of, keep_colour_rule
from test_pipeline import _install, _make_inputs
from testlib import REPO
from svsdct import batch, native

NEW_CALLS = ("svs_embed_bgr_readback_dev", "svs_embed_bgr_readback")


# ---- header, binding, library, validation ---------------------------------------------------------------------------
def test_header_binding_and_library_carry_both_calls():
    text = open(os.path.join(REPO, "include", "svsdct.h")).read()
    lib = native.load()
    for name in NEW_CALLS:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert native.SIGNATURES["svs_embed_bgr_readback"][1][-1] is C.POINTER(native.ReadbackCounts)
    assert len(native.SIGNATURES["svs_embed_bgr_readback_dev"][1]) == len(native.SIGNATURES["svs_embed_bgr_dev"][1]) + 1
    assert "colour support is follow-up work" not in text
    assert native.ABI_VERSION == 4 and "#define SVS_ABI_VERSION 4" in text


def test_arguments_refused_before_any_device_work():
    lib = native.load()
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    P = C.byref(planes)
    bgr = np.zeros((f, h, w, 3), np.uint8)
    bits = np.zeros(16, np.uint8)
    got = C.c_uint64(0)
    counts = native.ReadbackCounts()
    bad = native.SVS_ERR_INVALID_ARG
    rp, fp = 3 * w, 3 * w * h
    ok_flags = native.SVS_READBACK | native.SVS_KEEP_COLOUR | native.SVS_EXACT_GUARDED

    def dev(in_ptr=bgr.ctypes.data, out_ptr=bgr.ctypes.data, rp_in=rp, rp_out=rp, flags=ok_flags):
        return lib.svs_embed_bgr_readback_dev(in_ptr, rp_in, fp + 64, out_ptr, rp_out, fp + 64, None, P, None, 8.0, n_ac,
                                              bits.ctypes.data, 0, 8, flags, C.byref(got), None, None)

    def host(in_ptr=bgr.ctypes.data, out_ptr=bgr.ctypes.data, flags=ok_flags):
        return lib.svs_embed_bgr_readback(in_ptr, out_ptr, None, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8, flags,
                                          C.byref(got), C.byref(counts))

    assert dev(in_ptr=None) == bad and dev(out_ptr=None) == bad                  # NULL planes
    assert host(in_ptr=None) == bad and host(out_ptr=None) == bad
    for flags in (0x4, ok_flags | 0x400, 0x80000000):                            # unknown flag bits
        assert dev(flags=flags) == bad and host(flags=flags) == bad, hex(flags)
        assert b"unknown flags" in lib.svs_last_error()
    assert dev(rp_in=rp + 4) == bad and dev(rp_out=rp + 12) == bad               # BGR pitches that are no multiples of 8
    assert b"multiples of 8" in lib.svs_last_error()
    assert lib.svs_embed_bgr_readback_dev(bgr.ctypes.data, rp, fp, bgr.ctypes.data, rp, fp, None, None, None, 8.0, n_ac,
                                          bits.ctypes.data, 0, 8, 0, C.byref(got), None, None) == bad   # no planes at all
    # the plain colour calls still refuse the flag (tests/test_readback_cpu.py pins it too)
    assert lib.svs_embed_bgr(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8,
                             native.SVS_READBACK, C.byref(got)) == bad


def test_python_surface():
    for name in ("embed_bgr_frames", "embed_bgr_device"):
        params = inspect.signature(getattr(batch, name)).parameters
        assert params["readback"].default is False, name
    assert inspect.signature(batch.embed_bgr_device).parameters["d_counts"].default == 0
    import embed_process
    assert embed_process.READBACK_COLOUR is (os.environ.get("SVS_READBACK_COLOUR", "0") == "1")


# ---- the drop-in's switch (frame loop under the CPU emulation) -------------------------------------------------------
class _ReadbackPipeline(fakes.EmuFramePipeline):
    """the emulated pipeline with the `readback` parameter of svsdct.pipeline.FramePipeline; it records how it was built"""
    built = []

    def __init__(self, *a, readback=False, **kw):
        super().__init__(*a, **kw)
        _ReadbackPipeline.built.append(readback)

    def readback_counts(self):
        return batch.ReadbackCounts(0, 0)


def _drop_in(monkeypatch, tmp_path):
    emb, _ = _install(monkeypatch, "emu")
    _ReadbackPipeline.built = []
    monkeypatch.setattr(emb, "FramePipeline", _ReadbackPipeline)
    _, _, secret_path = _make_inputs(tmp_path, n_frames=3, size=(64, 96))
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    return emb, secret_path, pub


def test_drop_in_switch_off_makes_todays_calls(monkeypatch, tmp_path, capsys):
    emb, secret_path, pub = _drop_in(monkeypatch, tmp_path)
    assert emb.READBACK_COLOUR is False
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)[0]
    assert _ReadbackPipeline.built == [False]
    assert "Read-back" not in capsys.readouterr().out


def test_drop_in_refuses_block_key_and_gray_switch(monkeypatch, tmp_path):
    emb, secret_path, pub = _drop_in(monkeypatch, tmp_path)
    monkeypatch.setattr(emb, "READBACK_COLOUR", True)
    monkeypatch.setattr(emb, "READBACK", True)
    with pytest.raises(ValueError, match="SVS_READBACK"):
        emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)
    monkeypatch.setattr(emb, "READBACK", False)
    monkeypatch.setenv("SVS_BLOCK_KEY", "0x1234")
    with pytest.raises(ValueError, match="SVS_BLOCK_KEY"):
        emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)
    assert _ReadbackPipeline.built == []


def test_drop_in_mismatching_cv2_takes_the_gray_read_back_route(monkeypatch, tmp_path, capsys):
    emb, secret_path, pub = _drop_in(monkeypatch, tmp_path)
    from svsdct import colour

    def no_table(cv2):       # the verdict on a cv2 whose conversion matches no table (the comparison itself runs on the device)
        raise colour.ColourMismatch("cv2.cvtColor matches no known weight table")
    monkeypatch.setattr(colour, "weights_matching_cv2", no_table)
    monkeypatch.setattr(emb, "READBACK_COLOUR", True)
    monkeypatch.setattr(emb, "KEEP_COLOUR", True)
    monkeypatch.setattr(batch, "embed_bgr_frames", lambda *a, **k: pytest.fail("the fused colour path must not run"))
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)[0]
    said = capsys.readouterr().out
    assert _ReadbackPipeline.built == [True]
    assert "jalur warna terfusi tidak dipakai" in said and "read-back dijalankan pada jalur abu-abu" in said
    assert "Read-back: 0 blok diperbaiki" in said


def test_drop_in_switch_on_sums_the_counts_of_every_batch(monkeypatch, tmp_path, capsys):
    """switch on and a matching table: every batch goes through embed_bgr_frames(readback=True), the 4-tuple is unpacked and
    the counts of all batches are summed into one "Read-back:" line (a stand-in embed: B = G = R = the emulated stego)"""
    emb, secret_path, pub = _drop_in(monkeypatch, tmp_path)
    from svsdct import colour
    monkeypatch.setattr(colour, "weights_matching_cv2", lambda cv2: (3735, 19235, 9798, 15))
    monkeypatch.setattr(emb, "READBACK_COLOUR", True)
    monkeypatch.setattr(emb, "BATCH_FRAMES", 1)
    seen = []

    def fake(frames_bgr, delta, n_ac, bits, bit_offset=0, n_bits=None, weights=None, keep_colour=False, readback=False):
        seen.append((readback, keep_colour, tuple(weights)))
        gray = np.ascontiguousarray(frames_bgr[..., 1])
        stego, used = batch.embed_frames(gray, delta, n_ac, bits, bit_offset=bit_offset, n_bits=n_bits)
        return np.repeat(np.asarray(stego)[..., None], 3, axis=-1), gray, used, batch.ReadbackCounts(3, len(seen) - 1)
    monkeypatch.setattr(batch, "embed_bgr_frames", fake)
    assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)[0]
    said = capsys.readouterr().out
    assert len(seen) == 2 and all(s == (True, False, (3735, 19235, 9798, 15)) for s in seen)
    assert _ReadbackPipeline.built == []
    assert "Read-back: 6 blok diperbaiki, 1 blok tidak dapat diperbaiki." in said and "Warning: 1 blok" in said


# ---- the model of the contract ----------------------------------------------------------------------------------------
def _blocks(a):
    f, h, w = a.shape[:3]
    return a.reshape(f, h // 8, 8, w // 8, 8, -1).transpose(0, 1, 3, 2, 4, 5).reshape(f * (h // 8) * (w // 8), 8, 8, -1)


@pytest.mark.parametrize("weights", [W15, W14], ids=["15-bit", "14-bit"])
@pytest.mark.parametrize("delta,n_ac", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_model_keeps_the_contract(kind, delta, n_ac, weights):
    f, h, w = 2, 64, 96
    cover = colour_frames(kind, f, h, w, seed=3)
    cap = f * (h // 8) * (w // 8) * n_ac
    bits = payload(cap - cap // 5 - 3)                                        # ends inside the second frame, inside a block
    gray = gray_of(cover, weights)
    for keep in (False, True):
        out, planes, counts, status, before = model(cover, delta, n_ac, bits, weights, keep)
        assert np.array_equal(gray_of(out, weights), planes)                  # gray(output) == the gray read-back's planes
        assert np.array_equal(gray_of(before, weights), orc.batch_embed(gray, delta, bits, n_ac)[0])
        changed = gray_of(before, weights) != planes
        assert np.array_equal(out[~changed], before[~changed])                # a pixel whose gray did not change keeps its bytes
        same = (_blocks(out) == _blocks(before)).all(axis=(1, 2, 3))
        assert same[status != 1].all()                                        # only repaired blocks move
        assert counts == (int((status == 1).sum()), int((status == 2).sum()))
        if keep:
            rep = status == 1
            want = keep_colour_rule(_blocks(before)[rep], _blocks(planes[..., None])[rep][..., 0], weights)
            assert np.array_equal(_blocks(out)[rep], want)
        else:
            assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
        # counts are the gray pass's on the same planes, never a constant
        _, want_counts, _ = host_readback(orc.batch_embed(gray, delta, bits, n_ac)[0], delta, n_ac, bits)
        assert counts == want_counts
        got = orc.batch_extract_bits(gray_of(out, weights), delta, n_ac)[: bits.size]
        if counts[1] == 0:
            assert np.array_equal(got, bits)                                  # the oracle's extraction: zero bit errors
        if kind in CLIPPING and (delta, n_ac) in MAIN_SETTINGS:
            assert counts[1] == 0, (kind, delta, n_ac)
            if kind != "bright" or delta >= 16:                               # (the bright covers lose nothing at delta = 8)
                assert counts[0] > 0, (kind, delta, n_ac)
        if kind == "noise" and (delta, n_ac) in MAIN_SETTINGS:
            assert counts == (0, 0) and np.array_equal(out, before)           # without failures: the call without read-back


def test_colour_covers_fall_in_the_classes():
    bars = colour_content("letterbox", 64, 96)
    assert (bars[:8] == 0).all() and (bars[-8:] == 0).all()
    inner = bars[8:-8].astype(int)
    assert (np.abs(inner[..., 0] - inner[..., 1]) > 8).mean() > 0.5           # a coloured interior
    assert colour_content("bright", 64, 96).min() >= 223
    assert not colour_content("flat0", 64, 96).any()
    noise = colour_content("noise", 64, 96)
    assert (noise[..., 0] != noise[..., 2]).mean() > 0.9
