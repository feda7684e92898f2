"""Keyed dither modulation (svs_embed_dithered* / svs_extract_dithered*, include/svsdct.h) without a GPU: the hash pinned in
three restatements, the host build of the dithered block bodies against the NumPy model, what the dither buys (no keyless comb
test, no keyless read) and what it must not cost (distortion, robustness), the argument checks of the C ABI on empty batches,
and the Python layers' refusals and unchanged routes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import dither_lib as dl
import fakes
from coeff_select_lib import zigzag
from oracle import qim_dct_oracle as orc
from oracle.qim_dct_oracle import _blocks_view, _fwd
from svsdct import batch, dither, native, pipeline
from test_pipeline import _install, _make_inputs
from testlib import REPO

INVALID = native.SVS_ERR_INVALID_ARG
KEY = 0x0123456789ABCDEF         # hi32 != 0
OTHER_KEY = 0x0123456789ABCDEE
NEW = ("svs_embed_dithered_dev", "svs_extract_dithered_dev", "svs_embed_dithered", "svs_extract_dithered")


# ---- the hash ----------------------------------------------------------------------------------------------------------
N_TABLE = 1200
# (key, t, i, k) -> h: the format, pinned as literals (worked out once with Python integers from the rule in include/svsdct.h)
PINNED = {(0, 0, 0, 1): 0x4D436735,
          (0, 0, N_TABLE - 1, 63): 0xAE5FAD7A,
          (KEY, 5, 0, 1): 0x9FFF75BD,
          (KEY, 2 ** 32 - 1, N_TABLE - 1, 63): 0x0FD6168F,
          (2 ** 64 - 1, 2 ** 32 - 1, 7, 10): 0x6EBCD86A,
          (0xFFFFFFFF, 1, 1, 1): 0x52BE8B87}


def test_hash_agrees_in_the_model_the_package_and_the_product_header():
    for (key, t, i, k), h in PINNED.items():
        assert dl.hash_of(key, t, i, k) == h
        assert int(dl.hash_table(key, t, N_TABLE)[i, k]) == h
        assert int(dither.hashes(key, t, N_TABLE)[i, k]) == h
        seed, s_b, h_host, d_host = dl.host_hash(key, t, i, k, 20.0)
        assert seed == dl.seed_of(key) == dither.seed(key) and h_host == h
        d = dither.dither(key, t, N_TABLE, 20)
        assert d.dtype == np.float32 and d.shape == (N_TABLE, 64)
        assert d[i, k].view(np.uint32) == d_host.view(np.uint32) == dl.dither_table(key, t, N_TABLE, 20)[i, k].view(np.uint32)
    # whole tables, and the seed is not the block order's (one key may serve both)
    for key, t in ((0, 0), (KEY, 5), (KEY, 2 ** 32 - 1)):
        assert np.array_equal(dl.hash_table(key, t, N_TABLE), dither.hashes(key, t, N_TABLE))
    assert dl.seed_of(KEY) != dl.lb(dl.lb((KEY >> 32) ^ 0x9E3779B9) ^ (KEY & dl.M32))


def test_hash_steps():
    """the steps of the rule, spelled out for the simplest case, and every argument reaches the hash"""
    assert dl.lb(0) == 0 and len(set(PINNED.values())) == len(PINNED)
    # t and i reach the hash: neighbours differ
    assert dl.hash_of(KEY, 5, 0, 1) != dl.hash_of(KEY, 6, 0, 1) != dl.hash_of(KEY, 6, 1, 1)
    assert dl.hash_of(KEY, 5, 0, 1) != dl.hash_of(OTHER_KEY, 5, 0, 1)
    # (0, 0, 0, k): seed = lb(lb(0x85EBCA6B)), s_t = lb(seed), s_b = lb(s_t), h = lb(s_b ^ k * 0x632BE5AB)
    s = dl.lb(dl.lb(dl.lb(dl.lb(0x85EBCA6B))))
    assert dl.hash_of(0, 0, 0, 1) == dl.lb(s ^ 0x632BE5AB) and dl.hash_of(0, 0, 0, 63) == dl.lb(s ^ ((63 * 0x632BE5AB) & dl.M32))


def test_range_is_exact_and_half_open():
    h = dl.hash_table(KEY, 3, 4096)
    r = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    exact = [(int(x) >> 8) - 2 ** 23 for x in h.reshape(-1)[:5000]]              # r * 2^23 as Python integers
    assert [int(x) for x in (r.reshape(-1)[:5000].astype(np.float64) * 2 ** 23)] == exact
    assert r.min() >= -1.0 and r.max() < 1.0
    for top in (0, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000):                          # the ends of the range
        v = np.float32(top >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)
        assert float(v) == ((top >> 8) - 2 ** 23) / 2 ** 23 and -1.0 <= float(v) < 1.0
    d = dl.dither_table(KEY, 3, 64, 20)
    assert d.min() >= -20 and d.max() < 20 and abs(float(d[:, 1:].mean())) < 0.6   # 4032 uniform draws: sigma of the mean 0.18


# ---- the host build of the block bodies against the model -------------------------------------------------------------
FRAMES = dl.noise((2, 32, 48), 16, 240, seed=4)          # 24 blocks per frame


@pytest.mark.parametrize("rule", dl.RULES)
@pytest.mark.parametrize("n", (3, 10, 63))
@pytest.mark.parametrize("delta", (20, 8, 12.5, 0.1))
def test_host_bodies_equal_the_model(rule, n, delta):
    cap = 48 * n
    bits = dl.payload(cap - n - 2, seed=n)                # the budget ends inside the last block but one
    want, used = dl.model_batch_embed(FRAMES, delta, bits, n, rule, key=KEY, first_frame=5)
    got, done, info = dl.host_embed(FRAMES, delta, n, bits, KEY, 5, rule)
    assert info["dithered"] == 1 and info["rows"] == 8 and info["path"] == 2      # EmbedPath::EXACT with all eight rows
    assert done == used == bits.size and np.array_equal(got, want)
    assert np.array_equal(got[1, 24:, 40:], FRAMES[1, 24:, 40:])                  # the block past the budget: the cover's bytes
    bits_want = dl.model_batch_extract(want, delta, n, key=KEY, first_frame=5)
    bits_got, xinfo = dl.host_extract(want, delta, n, KEY, 5)
    assert xinfo["dithered"] == 1 and xinfo["rows"] == 8 and xinfo["path"] == 1   # ExtractPath::EXACT
    assert np.array_equal(bits_got, bits_want)
    # the model without a key is the oracle (the reference rule): what the three changes were made to
    if rule == "reference":
        ref, ref_used = orc.batch_embed(FRAMES, delta, bits, n)
        plain, plain_used = dl.model_batch_embed(FRAMES, delta, bits, n)
        assert np.array_equal(plain, ref) and plain_used == ref_used
        assert np.array_equal(dl.model_batch_extract(ref, delta, n), orc.batch_extract_bits(ref, delta, n))


@pytest.mark.parametrize("rule", dl.RULES)
def test_model_with_a_selection_and_a_partial_budget_reads_back(rule):
    """a selection (zigzag:6, count 3) with a budget that ends inside a block: the model reads its own bits back, and the host
    build of the block bodies gives the model's bytes and bits"""
    index = zigzag(3, first=6)
    frames = dl.noise((2, 32, 48), 64, 192, seed=4)
    bits = dl.payload(48 * 3 - 4, seed=9)                 # ends inside a block: only its first coefficients, in selection order
    want, used = dl.model_batch_embed(frames, 20, bits, 3, rule, index=index, key=KEY)
    assert used == bits.size
    want_bits = dl.model_batch_extract(want, 20, 3, index=index, key=KEY)
    assert np.array_equal(want_bits[:used], bits)
    host, host_used, info = dl.host_embed(frames, 20, 3, bits, KEY, 0, rule, index=index)
    assert host_used == used and info["selected"] == 1 and info["dithered"] == 1
    assert np.array_equal(host, want), np.argwhere(host != want)[:4]
    assert np.array_equal(dl.host_extract(want, 20, 3, KEY, 0, index=index)[0], want_bits)
    # the prefix as a selection is the call without one
    prefix, _, info = dl.host_embed(frames, 20, 3, bits, KEY, 0, rule, index=[1, 2, 3])
    assert info["selected"] == 0 and np.array_equal(prefix, dl.model_batch_embed(frames, 20, bits, 3, rule, key=KEY)[0])


def test_minmove_leaves_a_coefficient_inside_its_band_exactly_alone():
    stats = {}
    g = dl.noise((64, 64), 64, 192, seed=2)
    dl.model_embed(g, 40, dl.payload(64 * 10), 10, "minmove", key=KEY, stats=stats)
    same = stats["new"].view(np.uint32) == stats["c"].view(np.uint32)
    assert 0.2 < same.mean() < 0.9                       # a band of half-width 16 in a cell of 40: many stay, many move
    host, _, _ = dl.host_embed(g, 40, 10, dl.payload(64 * 10), KEY, 0, "minmove")
    assert np.array_equal(host[0], dl.model_embed(g, 40, dl.payload(64 * 10), 10, "minmove", key=KEY)[0])


def test_pass_through_routes_are_the_call_without_a_dither():
    bits = dl.payload(100)
    for delta, n, b in ((0, 10, bits), (-1.5, 10, bits), (20, 0, bits), (20, 10, bits[:0])):
        got, done, info = dl.host_embed(FRAMES, delta, n, b, KEY, 3)
        ref, _ = orc.batch_embed(FRAMES, delta, b, n)
        assert done == 0 and info["dithered"] == 0 and np.array_equal(got, ref), (delta, n, b.size)
    zeros, info = dl.host_extract(FRAMES, 0, 10, KEY, 3)
    assert info["path"] == 0 and zeros.size == 480 and not zeros.any()


# ---- what the dither buys, and what it must not cost --------------------------------------------------------------------
GRAY = dl.noise((240, 320), 64, 192, seed=1)             # [64, 192) cannot clip at delta = 20, n = 10: 10 * 1.5 * 20 * 0.177 = 53 < 64
BITS = dl.payload(1200 * 10, seed=7)


def _payload_coefficients(stego, n=10):
    coef = _fwd(_blocks_view(np.float32(stego)).reshape(1, -1, 8, 8)).reshape(-1, 64)
    return coef[:, 1:n + 1].reshape(-1)


def _near_lattice(c, delta):
    return float((np.abs(c - delta * np.rint(c / delta)) < delta / 4).mean())


def test_keyless_comb_test_is_gone():
    plain, _ = dl.model_embed(GRAY, 20, BITS, 10)
    dithered, _ = dl.model_embed(GRAY, 20, BITS, 10, key=KEY)
    assert not (dithered == 0).any() and not (dithered == 255).any() and not (plain == 0).any() and not (plain == 255).any()
    a, b = _near_lattice(_payload_coefficients(plain), 20), _near_lattice(_payload_coefficients(dithered), 20)
    print(f"share within delta/4 of the lattice: {a:.4f} without a dither, {b:.4f} with one")
    assert a == 1.0                                      # truncation error <= 4.0 < 5
    assert 0.45 <= b <= 0.55                             # 12 000 coefficients: binomial sigma 0.0046, 10 sigma


def test_the_key_is_needed():
    dithered, used = dl.model_embed(GRAY, 20, BITS, 10, key=KEY)
    assert used == BITS.size
    right = dl.model_extract(dithered, 20, 10, key=KEY)
    wrong = dl.model_extract(dithered, 20, 10, key=OTHER_KEY)
    keyless = dl.model_extract(dithered, 20, 10)
    assert np.array_equal(keyless, orc.frame_extract_bits(dithered, 20, 10))
    ber_wrong, ber_keyless = float((wrong != BITS).mean()), float((keyless != BITS).mean())
    print(f"bit error rate: right key {int((right != BITS).sum())} errors, other key {ber_wrong:.4f}, no dither {ber_keyless:.4f}")
    assert np.array_equal(right, BITS)
    assert 0.45 <= ber_wrong <= 0.55 and 0.45 <= ber_keyless <= 0.55


@pytest.mark.parametrize("rule", dl.RULES)
def test_no_distortion_cost(rule):
    plain, _ = dl.model_embed(GRAY, 20, BITS, 10, rule)
    dithered, _ = dl.model_embed(GRAY, 20, BITS, 10, rule, key=KEY)
    a, b = dl.psnr(GRAY, plain), dl.psnr(GRAY, dithered)
    print(f"{rule}: PSNR {a:.2f} dB without a dither, {b:.2f} dB with one")
    assert abs(a - b) < 0.5


@pytest.mark.parametrize("rule,delta", (("minmove", 20), ("nearest", 8)))
def test_robustness_is_kept(rule, delta):
    """delta = 20: derived for blocks that do not clip, 4.0 + 1/16 < 10.  delta = 8: confirmed with the model (0 errors on this
    frame), as for the rule without a dither: the truncation error 4.0 reaches delta / 2 only in its worst case."""
    stego, used = dl.model_embed(GRAY, delta, BITS, 10, rule, key=KEY)
    assert not (stego == 0).any() and not (stego == 255).any()
    got = dl.model_extract(stego, delta, 10, key=KEY)
    print(f"{rule}, delta = {delta}: {int((got != BITS).sum())} bit errors")
    assert used == BITS.size and np.array_equal(got, BITS)


# ---- the C ABI's argument checks (no GPU: empty batches, NULL pointers) --------------------------------------------------
def _calls(dith, order=None, coeffs=None, embed_flags=0, extract_flags=0, n_frames=0):
    lib = native.load()
    planes = native.Planes.contiguous(n_frames, 8, 8)
    done = C.c_uint64(7)
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    return (lib.svs_embed_dithered_dev(None, None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0, 8,
                                       embed_flags, C.byref(done), None),
            lib.svs_embed_dithered(None, None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0, 8,
                                   embed_flags, C.byref(done)),
            lib.svs_extract_dithered_dev(None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0,
                                         extract_flags, C.byref(done), None),
            lib.svs_extract_dithered(None, C.byref(planes), ref(order), ref(coeffs), ref(dith), 8.0, 3, None, 0, extract_flags,
                                     C.byref(done)))


def test_dither_argument_checks():
    good = native.Dither(KEY, 5, 0)
    assert _calls(good) == (0,) * 4
    assert _calls(None) == (INVALID,) * 4
    assert "dither is NULL" in native.load().svs_last_error().decode()
    assert _calls(native.Dither(KEY, 5, 1)) == (INVALID,) * 4
    assert "reserved" in native.load().svs_last_error().decode()
    # with a frame to work on the checks still come first: no pointer is looked at, no device is needed
    assert _calls(None, n_frames=1) == (INVALID,) * 4 and _calls(native.Dither(KEY, 5, 7), n_frames=1) == (INVALID,) * 4
    # an order and a dither share first_frame
    assert _calls(good, order=native.BlockOrder(9, 5, 0)) == (0,) * 4
    assert _calls(good, order=native.BlockOrder(9, 4, 0)) == (INVALID,) * 4
    assert "first_frame" in native.load().svs_last_error().decode()
    assert _calls(good, order=native.BlockOrder(9, 5, 1)) == (INVALID,) * 4          # the order's own check still holds
    # a selection is checked as in the select calls
    for sel in (native.Coeffs(3, (C.c_uint8 * 63)(9, 2, 17)), native.Coeffs(3, (C.c_uint8 * 63)(1, 2, 3))):
        assert _calls(good, coeffs=sel) == (0,) * 4
    for sel in (native.Coeffs(2, (C.c_uint8 * 63)(9, 9)), native.Coeffs(1, (C.c_uint8 * 63)(0,)),
                native.Coeffs(64, (C.c_uint8 * 63)(*range(1, 64))), native.Coeffs(1, (C.c_uint8 * 63)(5, 6))):
        assert _calls(good, coeffs=sel) == (INVALID,) * 4
        assert "svs_coeffs" in native.load().svs_last_error().decode()
    assert _calls(None, coeffs=native.Coeffs(2, (C.c_uint8 * 63)(9, 9))) == (INVALID,) * 4   # the dither's check comes first
    assert "dither is NULL" in native.load().svs_last_error().decode()


def test_rejected_flags():
    good = native.Dither(KEY, 0, 0)
    for flag in (native.SVS_READBACK, native.SVS_KEEP_COLOUR, 0x400, 0x2000, 0x80000000, native.SVS_READBACK | native.SVS_NEAREST,
                 native.SVS_KEEP_COLOUR | 1):
        assert _calls(good, embed_flags=flag, extract_flags=flag) == (INVALID,) * 4, hex(flag)
    for flags in (0, 1, 2, 3, native.SVS_NEAREST, native.SVS_MINMOVE, native.SVS_NEAREST | native.SVS_MINMOVE | 1):
        rc = _calls(good, embed_flags=flags, extract_flags=flags & 3)
        assert rc == (0,) * 4, hex(flags)
    for flag in (native.SVS_NEAREST, native.SVS_MINMOVE):                            # embed flags: refused on extract
        assert _calls(good, embed_flags=flag, extract_flags=flag)[2:] == (INVALID, INVALID)


def test_header_binding_and_exports_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "svsdct.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(svs_[a-z0-9_]+)\s*\(", text))
    assert set(NEW) <= declared and set(NEW) <= set(native.SIGNATURES)
    assert declared == set(native.SIGNATURES)
    lib = native.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert "#define SVS_ABI_VERSION 4" in text
    assert C.sizeof(native.Dither) == 16
    assert re.search(r"typedef struct svs_dither \{\s*uint64_t key;\s*uint32_t first_frame;\s*uint32_t reserved;\s*\} svs_dither;", text)
    assert len(native.SIGNATURES["svs_embed_dithered_dev"][1]) == 14 and len(native.SIGNATURES["svs_extract_dithered_dev"][1]) == 12
    assert len(native.SIGNATURES["svs_embed_dithered"][1]) == 13 and len(native.SIGNATURES["svs_extract_dithered"][1]) == 11


# ---- the Python layers ---------------------------------------------------------------------------------------------------
def test_check_key_and_key_from_env():
    assert dither.check_key(0) == 0 and dither.check_key(2 ** 64 - 1) == 2 ** 64 - 1 and dither.check_key(np.uint64(7)) == 7
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            dither.check_key(bad)
    for bad in (1.5, "7", True, None):
        with pytest.raises(TypeError):
            dither.check_key(bad)
    assert dither.key_from_env({}) is None and dither.key_from_env({"SVS_DITHER_KEY": "  "}) is None
    assert dither.key_from_env({"SVS_DITHER_KEY": "0x10"}) == 16 and dither.key_from_env({"SVS_DITHER_KEY": " 0 "}) == 0
    assert dither.key_from_env({"SVS_DITHER_KEY": "0b101"}) == 5
    for bad in ("-1", str(2 ** 64), "key", "1.5"):
        with pytest.raises(ValueError):
            dither.key_from_env({"SVS_DITHER_KEY": bad})


def test_value_errors_come_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(native, "load", no_library)
    frames = np.zeros((1, 8, 8), np.uint8)
    bgr = np.zeros((1, 8, 8, 3), np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    three = np.zeros(3, np.uint8)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_frames(frames, 8, 3, three, dither_key=KEY, readback=True)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_device(0, 0, planes, 8, 3, 0, 0, 3, dither_key=KEY, readback=True)
    with pytest.raises(ValueError, match="read-back"):
        pipeline.FramePipeline(8, 8, 1, 8, 3, dither_key=KEY, readback=True)
    with pytest.raises(ValueError, match="read-back"):
        batch.embed_frames(frames, 8, 3, three, dither_key=KEY, coeffs="zigzag", readback=True)
    with pytest.raises(ValueError, match="colour"):
        batch.embed_bgr_frames(bgr, 8, 3, three, dither_key=KEY)
    with pytest.raises(ValueError, match="colour"):
        batch.extract_bgr_frames(bgr, 8, 3, dither_key=KEY)
    with pytest.raises(ValueError, match="colour"):
        batch.embed_bgr_device(0, 0, 0, planes, 8, 3, 0, 0, 3, dither_key=KEY)
    with pytest.raises(ValueError, match="colour"):
        batch.extract_bgr_device(0, planes, 8, 3, 0, 0, dither_key=KEY)
    with pytest.raises(ValueError, match="_str"):
        batch.embed_frames_str(frames, 8, 3, "010", dither_key=KEY)
    with pytest.raises(ValueError, match="_str"):
        batch.extract_frames_str(frames, 8, 3, dither_key=KEY)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            batch.embed_frames(frames, 8, 3, three, dither_key=bad)
        with pytest.raises(ValueError):
            batch.extract_device(0, planes, 8, 3, 0, 0, dither_key=bad)
    with pytest.raises(ValueError, match="first_frame"):
        batch.extract_frames(frames, 8, 3, dither_key=KEY, first_frame=2 ** 32)
    for name in ("embed_frames", "extract_frames", "embed_device", "extract_device"):
        assert inspect.signature(getattr(batch, name)).parameters["dither_key"].default is None
    assert inspect.signature(pipeline.FramePipeline.__init__).parameters["dither_key"].default is None


def test_drop_in_refusals(monkeypatch, capsys):
    import embed_process as emb
    import extract_process as ext
    monkeypatch.delenv("SVS_BLOCK_KEY", raising=False)
    monkeypatch.delenv("SVS_COEFFS", raising=False)
    monkeypatch.setenv("SVS_DITHER_KEY", "0x10")
    for switch in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
        for other in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
            monkeypatch.setattr(emb, other, other == switch)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        out = capsys.readouterr().out
        assert "Error: SVS_DITHER_KEY tidak dapat dipakai bersama" in out and "SVS_" + switch in out
    for other in ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR"):
        monkeypatch.setattr(emb, other, False)
    for value in ("key", "-1", str(2 ** 64)):
        monkeypatch.setenv("SVS_DITHER_KEY", value)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        assert "Error: SVS_DITHER_KEY tidak valid" in capsys.readouterr().out
        assert ext.ekstraksi_gambar_video_final("stego.avi", "out.png", 20, 10, None) is False
        assert "Error: SVS_DITHER_KEY tidak valid" in capsys.readouterr().out


# ---- the drop-in loops with the variable unset and set (frame loop under the CPU emulation, tests/fakes.py) ---------------
class _RecordingPipeline(fakes.EmuFramePipeline):
    """the emulated pipeline of tests/fakes.py; it notes the keywords it was built with and those of every submit"""
    built, submits = [], []

    def __init__(self, *a, **kw):
        known = {k: kw.pop(k) for k in ("block_key", "dither_key", "coeffs", "nearest", "minmove", "readback") if k in kw}
        super().__init__(*a, **kw)
        _RecordingPipeline.built.append(known)

    def submit_embed(self, slot, n_frames, bit_offset, **kw):
        _RecordingPipeline.submits.append(("embed", kw))
        return super().submit_embed(slot, n_frames, bit_offset)

    def submit_extract(self, slot, n_frames, **kw):
        _RecordingPipeline.submits.append(("extract", kw))
        return super().submit_extract(slot, n_frames)


def test_drop_in_routes_with_the_variable_unset_and_set(monkeypatch, tmp_path):
    emb, _ = _install(monkeypatch, "emu")
    monkeypatch.setattr(emb, "FramePipeline", _RecordingPipeline)
    monkeypatch.setattr(emb, "BATCH_FRAMES", 1)
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY"):
        monkeypatch.delenv(name, raising=False)
    _, _, secret_path = _make_inputs(tmp_path, n_frames=5, size=(64, 96))
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())

    def run():
        _RecordingPipeline.built, _RecordingPipeline.submits = [], []
        assert emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "x"), 20, 10, pub)[0]
        return _RecordingPipeline.built, _RecordingPipeline.submits

    built, submits = run()                                # unset: no dither keyword, no first_frame keyword - today's calls
    assert built == [{}] and len(submits) >= 2 and all(s == ("embed", {}) for s in submits)
    monkeypatch.setenv("SVS_DITHER_KEY", "0x10")
    built, submits = run()                                # set: the key reaches the pipeline, every submit names its first frame
    assert built == [{"dither_key": 16}]
    assert [kw for _, kw in submits] == [{"first_frame": k} for k in range(len(submits))] and len(submits) >= 2
    monkeypatch.setenv("SVS_BLOCK_KEY", "7")
    monkeypatch.setenv("SVS_COEFFS", "zigzag")
    built, submits = run()                                # allowed with a block key and a selection: one index feeds both
    assert built[0]["dither_key"] == 16 and built[0]["block_key"] == 7 and len(built[0]["coeffs"]) == 10
    assert [kw for _, kw in submits] == [{"first_frame": k} for k in range(len(submits))]
    monkeypatch.delenv("SVS_DITHER_KEY")
    built, submits = run()                                # the block key alone: the call it made before the dither
    assert "dither_key" not in built[0] and [kw for _, kw in submits] == [{"first_frame": k} for k in range(len(submits))]


# ---- nothing moved: without a dither key the layers make the calls they made ---------------------------------------------
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


def test_batch_calls_without_and_with_a_dither_key(recorded):
    frames, bits = np.zeros((2, 8, 8), np.uint8), np.zeros(6, np.uint8)
    planes = native.Planes.contiguous(2, 8, 8)
    order = batch.block_order(9, 4)
    batch.embed_frames(frames, 8, 3, bits)
    batch.embed_frames(frames, 8, 3, bits, block_key=9)
    batch.embed_frames(frames, 8, 3, bits, coeffs="zigzag")
    batch.embed_frames(frames, 8, 3, bits, readback=True)
    batch.extract_frames(frames, 8, 3)
    batch.extract_frames(frames, 8, 3, block_key=9)
    batch.extract_frames(frames, 8, 3, coeffs="zigzag")
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6)
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, order=order)
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, coeffs="zigzag")
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, readback=True)
    batch.extract_device(0, planes, 8, 3, 0, 8)
    batch.extract_device(0, planes, 8, 3, 0, 8, order=order)
    batch.extract_device(0, planes, 8, 3, 0, 8, coeffs="zigzag")
    assert recorded.names() == ["svs_embed", "svs_embed_ordered", "svs_embed_select", "svs_embed_readback", "svs_extract",
                                "svs_extract_ordered", "svs_extract_select", "svs_embed_dev", "svs_embed_ordered_dev",
                                "svs_embed_select_dev", "svs_embed_readback_dev", "svs_extract_dev", "svs_extract_ordered_dev",
                                "svs_extract_select_dev"]
    recorded.calls.clear()
    batch.embed_frames(frames, 8, 3, bits, dither_key=KEY, first_frame=4, block_key=9, nearest=True, mode="exact")
    batch.extract_frames(frames, 8, 3, dither_key=KEY, first_frame=4)
    batch.embed_device(0, 0, planes, 8, 3, 0, 0, 6, dither_key=KEY, order=order, minmove=True)
    batch.extract_device(0, planes, 8, 3, 0, 8, dither_key=KEY, first_frame=7)
    batch.embed_frames(frames, 8, 3, bits, dither_key=KEY, coeffs=[9, 2, 17])
    batch.extract_device(0, planes, 8, 3, 0, 8, dither_key=KEY, coeffs="zigzag:6")
    assert recorded.names() == list(np.array(NEW)[[2, 3, 0, 1, 2, 1]])
    (_, e), (_, x), (_, ed), (_, xd), (_, es), (_, xs) = recorded.calls
    assert (es[4]._obj.count, list(es[4]._obj.index[:3])) == (3, [9, 2, 17]) and xs[3]._obj.count == 3   # the selection goes along
    d = e[5]._obj
    assert (d.key, d.first_frame, d.reserved) == (KEY, 4, 0) and e[3]._obj.first_frame == 4 and e[4] is None   # no selection: NULL
    assert e[11] == native.SVS_EXACT_POCKETFFT | native.SVS_NEAREST
    assert x[2] is None and x[3] is None and x[4]._obj.first_frame == 4
    assert ed[5]._obj.first_frame == 4 and ed[3]._obj.first_frame == 4 and ed[11] & native.SVS_MINMOVE   # the order's first_frame
    assert xd[4]._obj.first_frame == 7


def test_pipeline_calls_without_and_with_a_dither_key(recorded):
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0)
        pipe.submit_extract(0, 2)
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1, block_key=9) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0, first_frame=2)
        pipe.submit_extract(0, 2, first_frame=2)
    assert recorded.names() == ["svs_embed_dev", "svs_extract_dev", "svs_embed_ordered_dev", "svs_extract_ordered_dev"]
    recorded.calls.clear()
    with pipeline.FramePipeline(8, 8, 2, 8, 3, depth=1, block_key=9, dither_key=KEY) as pipe:
        pipe.set_payload(np.zeros(12, np.uint8))
        pipe.submit_embed(0, 2, 0, first_frame=0)
        pipe.submit_embed(0, 2, 6, first_frame=2)
        pipe.submit_extract(0, 2, first_frame=2)
    calls = [(n, a) for n, a in recorded.calls if "dithered" in n]
    assert [n for n, _ in calls] == ["svs_embed_dithered_dev", "svs_embed_dithered_dev", "svs_extract_dithered_dev"]
    assert [(a[3]._obj.first_frame, a[5]._obj.first_frame) for _, a in calls[:2]] == [(0, 0), (2, 2)]   # one index feeds both
    assert (calls[2][1][2]._obj.first_frame, calls[2][1][4]._obj.first_frame) == (2, 2)
    assert recorded.names() == [n for n, _ in calls]
