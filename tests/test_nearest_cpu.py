"""SVS_NEAREST, CPU tier: the NumPy model of the nearest-parity embed (nearest_lib.model_embed: the oracle's frame_embed with
one line changed) is the oracle itself with the rule off; the embed bodies of csrc/svs_block.hpp - embed_block_exact, the
one-row and the two-row guarded body with their exact replay - equal the model byte for byte with the flag set, ties and both
directions included; the model keeps the rule's properties (moves of at most delta, untouched coefficients, lower SSE, the
same receiver); and the flag is routed and validated as include/svsdct.h says."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

import fakes
import nearest_lib as nl
from oracle import qim_dct_oracle as orc
from testlib import REPO, case_inputs, guard_corpus_case, single_frame_cases
from test_pipeline import _install, _make_inputs
from svsdct import batch, native
from svsdct.pipeline import FramePipeline

GOLDEN = os.path.join(REPO, "tests", "golden")
COPY, ROUND_TRIP, EXACT, STREAMING = range(4)         # svs::EmbedPath


# ---- 1. the model's scaffold ---------------------------------------------------------------------------------------------
def test_model_with_the_rule_off_is_the_oracle_on_the_golden_cases():
    arrays = np.load(os.path.join(GOLDEN, "qim_dct_golden.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "qim_dct_golden.json")))
    names = single_frame_cases(meta)
    assert len(names) >= 5
    for name in names:
        info, gray, bits = case_inputs(arrays, meta, name)
        want = orc.frame_embed(gray, info["delta"], bits, info["n_ac"])
        got = nl.model_embed(gray, info["delta"], bits, info["n_ac"], nearest=False)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2], name


# ---- 2. the kernels' arithmetic on the host ------------------------------------------------------------------------------
def _frame(kind, seed=1):
    return nl.content(kind, 64, 96, seed=seed)


@pytest.mark.parametrize("delta", nl.DELTAS)
@pytest.mark.parametrize("kind", ["noise", "smooth", "flat", "letterbox"])
def test_host_bodies_equal_the_model(kind, delta):
    """every n of the list, a budget that ends inside a block: embed_block_exact on every block (SVS_EXACT_POCKETFFT) and the
    route of the default mode (n <= 7 the one-row guarded body, n = 8..15 the two-row one, flagged blocks replayed exactly;
    n >= 16 and the steps outside the guard's range the exact body)"""
    g = _frame(kind)
    streamed = replayed = 0
    for n in nl.N_ACS:
        cap = (g.shape[0] // 8) * (g.shape[1] // 8) * n
        bits = nl.payload(cap - 5 if n > 1 else cap - 1, seed=n)
        want = nl.model_embed(g, delta, bits, n)
        ref = orc.frame_embed(g, delta, bits, n)
        for pocketfft in (False, True):
            got, used, rep, path = nl.host_embed(g, delta, n, bits, pocketfft=pocketfft)
            assert used == want[2] == bits.size
            assert np.array_equal(got[0], want[1]), (n, pocketfft)
            assert path == (STREAMING if not pocketfft and n <= 15 and 0.25 <= delta <= 4096 else EXACT)
            streamed += path == STREAMING
            replayed += rep
            # flag clear: the reference's pixels, as before
            off = nl.host_embed(g, delta, n, bits, pocketfft=pocketfft, nearest=False)[0]
            assert np.array_equal(off[0], ref[1]), (n, pocketfft)
    if 0.25 <= delta <= 4096:
        assert streamed == 6 and replayed > 0     # n = 1, 3, 7, 8, 10, 15; some blocks went through the replay


def test_host_bodies_on_the_guard_corpus():
    arrays = np.load(os.path.join(GOLDEN, "guard_corpus.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "guard_corpus.json")))
    assert meta["embed"]
    for name, m in meta["embed"].items():
        case = guard_corpus_case(arrays, meta, name)
        frame, bits, delta, n_ac = case["frame"], case["bits"], m["delta"], m["n_ac"]
        want = nl.model_embed(frame, delta, bits, n_ac)[1]
        for pocketfft in (False, True):
            got = nl.host_embed(frame, delta, n_ac, bits, pocketfft=pocketfft)[0]
            assert np.array_equal(got[0], want), (name, pocketfft)


@pytest.mark.parametrize("delta", nl.DELTAS)
def test_tie_takes_the_reference_direction(delta):
    """constant blocks: every AC coefficient is exactly 0, q = 0, c == c0 = 0 - bit 1 must give the reference's + 1"""
    g = _frame("flat")
    for n in (3, 10, 20):
        bits = np.ones((g.shape[0] // 8) * (g.shape[1] // 8) * n, np.uint8)
        stats = {}
        want = nl.model_embed(g, delta, bits, n, stats=stats)[1]
        assert stats["tie"] == bits.size and stats["up"] == stats["down"] == 0       # the case occurs, and nothing else does
        assert np.all(stats["c"] == 0) and np.array_equal(stats["new"], stats["old"])
        assert np.array_equal(want, orc.frame_embed(g, delta, bits, n)[1])
        for pocketfft in (False, True):
            assert np.array_equal(nl.host_embed(g, delta, n, bits, pocketfft=pocketfft)[0][0], want)


@pytest.mark.parametrize("delta", nl.DELTAS)
def test_both_directions_occur(delta):
    g = _frame("noise")
    for n in (3, 10, 20):
        bits = nl.payload((g.shape[0] // 8) * (g.shape[1] // 8) * n, seed=5)
        stats = {}
        nl.model_embed(g, delta, bits, n, stats=stats)
        assert stats["up"] > 20 and stats["down"] > 20
        moved = stats["new"] != stats["old"]
        assert moved.sum() > 20 and np.all(stats["forced"][moved])   # the rule differs from the reference's, on forced coefficients only


# ---- 3. properties of the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_ac,delta", nl.MEASURED)
def test_model_properties(kind, n_ac, delta):
    g = nl.content(kind)
    bits = nl.payload((g.shape[0] // 8) * (g.shape[1] // 8) * n_ac)
    stats = {}
    stego = nl.model_embed(g, delta, bits, n_ac, stats=stats)[1]
    ref = orc.frame_embed(g, delta, bits, n_ac)[1]
    forced, c, new, old = stats["forced"], stats["c"], stats["new"], stats["old"]
    assert forced.sum() > 1000
    move = np.abs(new.astype(np.float64) - c.astype(np.float64))
    assert move[forced].max() <= delta * (1 + 2.0 ** -20)
    assert np.abs(old.astype(np.float64) - c.astype(np.float64))[forced].max() > delta * 1.4     # the reference's reach 1.5 delta
    assert np.array_equal(new[~forced], old[~forced])
    if delta >= 4:
        ratio = nl.sse(stego, g) / nl.sse(ref, g)
        print(f"{kind} n={n_ac} delta={delta}: SSE ratio {ratio:.3f}, PSNR {orc.psnr_u8(g, ref):.2f} -> {orc.psnr_u8(g, stego):.2f} dB")
        assert nl.sse(stego, g) < nl.sse(ref, g)
    if delta >= 8 and kind in ("noise", "smooth"):
        assert np.array_equal(orc.frame_extract_bits(stego, delta, n_ac), bits)


@pytest.mark.parametrize("kind,n_ac,delta", nl.MEASURED)
def test_payload_that_already_matches_gives_the_reference_stego(kind, n_ac, delta):
    g = nl.content(kind, 120, 160)
    bits = orc.frame_extract_bits(g, delta, n_ac)
    stats = {}
    stego = nl.model_embed(g, delta, bits, n_ac, stats=stats)[1]
    assert not stats["forced"].any()
    assert np.array_equal(stego, orc.frame_embed(g, delta, bits, n_ac)[1])
    assert np.array_equal(nl.host_embed(g, delta, n_ac, bits)[0][0], stego)


# ---- 4. routing and validation --------------------------------------------------------------------------------------------
def test_plan_carries_the_flag_where_coefficients_are_forced():
    total = 100
    for bgr in (False, True):
        assert nl.plan(8, 3, total, 250, bgr=bgr) == (STREAMING, 1, 250)
        assert nl.plan(20, 10, total, 5000, bgr=bgr) == (STREAMING, 1, 1000)
        assert nl.plan(8, 20, total, 250, bgr=bgr) == (EXACT, 1, 250)
        assert nl.plan(8, 3, total, 250, pocketfft=True, bgr=bgr) == (EXACT, 1, 250)
        assert nl.plan(0.1, 3, total, 250, bgr=bgr) == (EXACT, 1, 250)
        assert nl.plan(8, 3, total, 250, bgr=bgr, nearest=False) == (STREAMING, 0, 250)
        assert nl.plan(8, 20, total, 250, bgr=bgr, nearest=False) == (EXACT, 0, 250)
        assert nl.plan(8, 3, total, 0, bgr=bgr) == (COPY, 0, 0)               # an empty payload is still a copy
        assert nl.plan(0.0, 3, total, 250, bgr=bgr) == (ROUND_TRIP, 0, 0)
        assert nl.plan(-2.0, 3, total, 250, bgr=bgr) == (ROUND_TRIP, 0, 0)
        assert nl.plan(8, 0, total, 250, bgr=bgr) == (ROUND_TRIP, 0, 0)


def test_flag_has_no_effect_where_nothing_is_embedded():
    g = _frame("noise")
    bits = nl.payload(100)
    for delta, n in ((0.0, 3), (-1.0, 10), (8, 0)):
        on, off = nl.host_embed(g, delta, n, bits), nl.host_embed(g, delta, n, bits, nearest=False)
        assert np.array_equal(on[0], off[0]) and on[1] == off[1] == 0
        assert np.array_equal(on[0][0], orc.frame_embed(g, delta, bits, n)[1])
    assert np.array_equal(nl.host_embed(g, 8, 3, bits[:0])[0][0], g)


def test_flag_value_header_and_binding():
    text = open(os.path.join(REPO, "include", "svsdct.h")).read()
    assert "#define SVS_NEAREST 0x800u" in text and native.SVS_NEAREST == 0x800
    others = native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED | native.SVS_KEEP_COLOUR | native.SVS_READBACK
    assert native.SVS_NEAREST & others == 0
    assert "#define SVS_ABI_VERSION 4" in text and native.load().svs_abi_version() == 4
    assert batch.embed_flags("guarded", True) == native.SVS_EXACT_GUARDED | native.SVS_NEAREST
    assert batch.embed_flags("guarded") == native.SVS_EXACT_GUARDED


def _extract_calls(lib, flag):
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    gray = np.zeros((f, h, w), np.uint8)
    out = np.zeros(64, np.uint8)
    got = C.c_uint64(0)
    P = C.byref(planes)
    return [lib.svs_extract(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
            lib.svs_extract_dev(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None),
            lib.svs_extract_ordered(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
            lib.svs_extract_ordered_dev(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None),
            lib.svs_extract_str(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
            # delta <= 0 gives zeros whatever the mode bits say - but not with an embed flag
            lib.svs_extract_dev(gray.ctypes.data, P, 0.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None)]


def test_every_extract_call_refuses_the_flag():
    """refused before any device work, so this runs without a GPU"""
    lib = native.load()
    for flag in (native.SVS_NEAREST, native.SVS_NEAREST | native.SVS_EXACT_GUARDED, native.SVS_NEAREST | native.SVS_EXACT_POCKETFFT):
        assert _extract_calls(lib, flag) == [native.SVS_ERR_INVALID_ARG] * 6
        assert b"SVS_NEAREST" in lib.svs_last_error()


def test_unknown_flags_stay_unknown():
    """0x4, 0x400 and 0x80000000 are refused by the embed calls, alone and next to the new flag (before any device work)"""
    lib = native.load()
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    gray = np.zeros((f, h, w), np.uint8)
    bgr = np.zeros((f, h, w, 3), np.uint8)
    bits = np.zeros(16, np.uint8)
    done = C.c_uint64(0)
    counts = native.ReadbackCounts()
    P = C.byref(planes)
    bad = native.SVS_ERR_INVALID_ARG
    for unknown in (0x4, 0x400, 0x80000000):
        for flag in (unknown, unknown | native.SVS_NEAREST):
            assert lib.svs_embed(gray.ctypes.data, gray.ctypes.data, P, 8.0, n_ac, bits.ctypes.data, 0, 8, flag, C.byref(done)) == bad
            assert lib.svs_embed_dev(gray.ctypes.data, gray.ctypes.data, P, 8.0, n_ac, bits.ctypes.data, 0, 8, flag, C.byref(done),
                                     None) == bad
            assert lib.svs_embed_str(gray.ctypes.data, None, gray.ctypes.data, P, 8.0, n_ac, b"01010101", 8, flag,
                                     C.byref(done)) == bad
            assert lib.svs_embed_ordered(gray.ctypes.data, gray.ctypes.data, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8, flag,
                                         C.byref(done)) == bad
            assert lib.svs_embed_readback(gray.ctypes.data, gray.ctypes.data, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8, flag,
                                          C.byref(done), C.byref(counts)) == bad
            assert lib.svs_embed_bgr(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8, flag,
                                     C.byref(done)) == bad
            assert lib.svs_embed_bgr_readback(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, bits.ctypes.data, 0, 8,
                                              flag, C.byref(done), C.byref(counts)) == bad
            assert b"unknown flags" in lib.svs_last_error()
        got = _extract_calls(lib, unknown)     # the host-pointer extract calls check their mode bits behind the staging: GPU tier
        assert got[1] == got[3] == bad
    # SVS_KEEP_COLOUR stays a colour-only flag next to the new one
    assert lib.svs_embed(gray.ctypes.data, gray.ctypes.data, P, 8.0, n_ac, bits.ctypes.data, 0, 8,
                         native.SVS_KEEP_COLOUR | native.SVS_NEAREST, C.byref(done)) == bad


def test_python_surface():
    for fn in (batch.embed_frames, batch.embed_device, batch.embed_bgr_device, batch.embed_bgr_frames, FramePipeline.__init__):
        assert inspect.signature(fn).parameters["nearest"].default is False, fn
    for fn in (batch.extract_frames, batch.extract_device, batch.extract_bgr_frames):
        assert "nearest" not in inspect.signature(fn).parameters


def test_drop_in_parses_the_switch(monkeypatch):
    """read the way SVS_READBACK is: at import, "1" switches it on; extract_process has no such switch"""
    import importlib
    emb, ext = _install(monkeypatch, "emu")
    assert emb.NEAREST is False
    try:
        for value, want in (("1", True), ("0", False), ("yes", False)):
            monkeypatch.setenv("SVS_NEAREST", value)
            assert importlib.reload(emb).NEAREST is want
            assert emb.READBACK is False and emb.KEEP_COLOUR is False
    finally:
        monkeypatch.delenv("SVS_NEAREST")
        importlib.reload(emb)
    assert emb.NEAREST is False and not hasattr(ext, "NEAREST")


def test_drop_in_passes_the_switch_on(monkeypatch, tmp_path, capsys):
    """with the switch the frame loop asks the pipeline for the rule and says so; without it the call is what it was"""
    emb, _ = _install(monkeypatch, "emu")
    _, _, secret_path = _make_inputs(tmp_path, n_frames=3, size=(32, 32))
    pub = fakes.serialisasi_kunci_publik_ecc_compressed(fakes.FakeKey(b"bob").public())
    seen = []

    class Stop(Exception):
        pass

    def pipeline(*a, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(emb, "FramePipeline", pipeline)
    for flagged in (False, True):
        monkeypatch.setattr(emb, "NEAREST", flagged)
        with pytest.raises(Stop):
            emb.embed_gambar_ke_video_final("in.mp4", secret_path, str(tmp_path / "out"), 20, 10, pub)
        out = capsys.readouterr().out
        assert ("SVS_NEAREST" in out) is flagged
    assert "nearest" not in seen[0] and seen[1]["nearest"] is True
