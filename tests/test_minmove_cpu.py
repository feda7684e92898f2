"""SVS_MINMOVE, CPU tier: the margin table of csrc/svs_block.hpp is the derived bound and the bound is tight; the NumPy model of
the minimum-move embed (minmove_lib.model_embed: nearest_lib.model_embed with the one assignment changed to the clamp) is the
nearest rule with the clamp off; the embed bodies of csrc/svs_block.hpp - embed_block_exact in its three row counts, the
selected loop, the one-row and the two-row guarded body with their exact replay, each quantiser arm - equal the model byte for
byte under the flag; the guarded bodies equal the exact ones on 24 000 blocks; the model keeps the rule's properties (the
nearest rule's bytes at small delta, 0 bit errors through the oracle's extraction on content that does not clip, moves of at
most delta, untouched coefficients inside the band, the PSNR table of include/svsdct.h); and the flag is routed and validated
as the header says."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import coeff_select_lib as cs
import minmove_lib as ml
import nearest_lib as nl
from oracle import qim_dct_oracle as orc
from testlib import CSRC, hostemu
from test_pipeline import _install
from svsdct import batch, coeffs, native
from svsdct.pipeline import FramePipeline

COPY, ROUND_TRIP, EXACT, STREAMING = range(4)         # svs::EmbedPath
KINDS = ("noise", "smooth", "flat", "letterbox")


# ---- 1. the margin table -------------------------------------------------------------------------------------------------
def _source_table():
    text = open(os.path.join(CSRC, "svs_block.hpp")).read()
    body = re.search(r"MARGIN\[64\] = \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return np.array([np.float32(v) for v in re.findall(r"([0-9.]+)f", body)], np.float32)


def test_margin_table_is_the_recomputed_bound():
    want = ml.margin_table()
    got = _source_table()
    assert got.size == 64 and np.array_equal(got[1:], want[1:])
    assert np.array_equal(np.array([hostemu().mm_margin(k) for k in range(1, 64)], np.float32), want[1:])
    bound = want[1:].astype(np.float64) - 0.0625
    assert 3.284 < bound.min() < 3.285 and abs(bound.max() - 4.0) < 1e-6
    # every r_k is 0 up to delta = 6.69 and some r_k is positive above
    assert not ml.band(6.69).any() and ml.band(6.70)[1:].any()


def test_the_bound_is_attained():
    """e = -1 where b_k > 0, else 0 is a truncation pattern in (-1, 0]^64 whose coefficient error is 0.5 sum |b_k|"""
    x = np.arange(8)
    a = np.array([np.sqrt(1 / 8)] + [0.5] * 7)
    basis = a[:, None] * np.cos((2 * x[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)     # [u, x]
    s = ml.basis_sums()
    for k in range(1, 64):
        b = np.outer(basis[k // 8], basis[k % 8])
        assert abs(b.sum()) < 1e-12
        e = np.where(b > 0, -1.0, 0.0)
        assert abs(abs((b * e).sum()) - 0.5 * s[k // 8] * s[k % 8]) < 1e-12
        assert abs(np.abs(b).sum() - s[k // 8] * s[k % 8]) < 1e-12


# ---- 2. the model's scaffold ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta,n", [(20, 10), (8, 3), (7.3, 63)])
def test_model_with_the_clamp_off_is_the_nearest_model(delta, n):
    g = nl.content("noise", 64, 96)
    bits = nl.payload(96 * n - 5, seed=n)
    assert np.array_equal(ml.model_embed(g, delta, bits, n, minmove=False)[1], nl.model_embed(g, delta, bits, n)[1])
    idx = cs.zigzag(6)
    bits = nl.payload(96 * 6 - 5)
    assert np.array_equal(ml.model_embed(g, delta, bits, index=idx, minmove=False)[1], cs.select_embed(g, delta, bits, idx, True)[1])


# ---- 3. the kernels' arithmetic on the host ------------------------------------------------------------------------------
def _valid_arms(delta, plan_qm):
    """the plan's quantiser arm, plus every other arm that is exact for this delta: QM_F32 for any float32 step, QM_DOUBLE
    for any step"""
    arms = {plan_qm, ml.QM_DOUBLE}
    if float(np.float32(delta)) == float(delta):
        arms.add(ml.QM_F32)
    return sorted(arms)


@pytest.mark.parametrize("delta", ml.DELTAS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_bodies_equal_the_model(kind, delta):
    """every n of the list, a budget that ends inside a block: embed_block_exact on every block (SVS_EXACT_POCKETFFT, the row
    count the plan names) and the route of the default mode (n <= 7 the one-row guarded body, n = 8..15 the two-row one, flagged
    blocks replayed exactly; n >= 16 and the steps outside the guard's range the exact body), in every quantiser arm that is
    valid for the step"""
    g = nl.content(kind, 64, 96)
    streamed = replayed = 0
    arms_seen = set()
    for n in ml.N_ACS:
        cap = (g.shape[0] // 8) * (g.shape[1] // 8) * n
        bits = nl.payload(cap - 5 if n > 1 else cap - 1, seed=n)
        want = ml.model_embed(g, delta, bits, n)
        near = nl.model_embed(g, delta, bits, n)
        if kind in ("noise", "smooth") and delta >= 12:
            assert not np.array_equal(want[1], near[1])                 # neither the nearest rule's pixels
        for pocketfft in (False, True):
            got, used, info = ml.host_embed(g, delta, n, bits, pocketfft=pocketfft)
            assert used == want[2] == bits.size and info["minmove"] == 1
            assert np.array_equal(got[0], want[1]), (n, pocketfft)
            assert info["path"] == (STREAMING if (not pocketfft and n <= 15 and delta <= 4096) else EXACT)
            streamed += info["path"] == STREAMING
            replayed += info["replayed"]
            for qm in _valid_arms(delta, info["qm"]):
                arms_seen.add(qm)
                forced = ml.host_embed(g, delta, n, bits, pocketfft=pocketfft, qm=qm)[0]
                assert np.array_equal(forced[0], want[1]), (n, pocketfft, qm)
        # SVS_NEAREST next to the flag changes nothing
        assert np.array_equal(ml.host_embed(g, delta, n, bits, nearest=True)[0][0], want[1])
    if delta <= 4096:
        assert streamed == 6
    if kind == "flat" and delta <= 4096:
        assert replayed > 0                # constant blocks: the guard hands them to the exact replay
    assert ml.QM_DOUBLE in arms_seen and (ml.QM_POW2 in arms_seen) == (delta == 8)


@pytest.mark.parametrize("delta", [8, 20, 7.3, 40])
@pytest.mark.parametrize("kind", ["zigzag", "reversed", "scattered"])
def test_selected_loop_equals_the_model(kind, delta):
    """the band is that of the coefficient's flat index, whatever stream slot it carries"""
    g = nl.content("noise", 64, 96, seed=2)
    for count in (1, 6, 10, 33, 63):
        idx = cs.KINDS[kind](count)
        bits = nl.payload(96 * count - (5 if count > 1 else 1), seed=count)
        want = ml.model_embed(g, delta, bits, index=idx)
        for pocketfft in (False, True):
            got, used, info = ml.host_embed(g, delta, count, bits, pocketfft=pocketfft, index=idx)
            assert used == bits.size and info["minmove"] == 1
            assert info["path"] == (STREAMING if idx == cs.prefix(count) and not pocketfft else EXACT)
            assert np.array_equal(got[0], want[1]), (count, pocketfft)
    # the prefix as a selection is the call without one
    bits = nl.payload(96 * 10 - 5)
    assert np.array_equal(ml.host_embed(g, delta, 10, bits, index=cs.prefix(10))[0], ml.host_embed(g, delta, 10, bits)[0])


@pytest.mark.parametrize("qm,delta", [(ml.QM_POW2, 8), (ml.QM_F32, 20), (ml.QM_F32, 12.5), (ml.QM_DOUBLE, 7.3), (ml.QM_DOUBLE, 20),
                                      (ml.QM_F32, 4), (ml.QM_DOUBLE, 6.5)])
def test_one_coefficient_through_both_forms(qm, delta):
    """qim_target (the exact bodies) and qim_change (the streaming bodies, magic-constant and QM_DOUBLE arms) against the rule
    written out in NumPy float32, for every flat index; coefficients on lattice points, cell edges and band edges included"""
    rng = np.random.default_rng(5)
    d32 = np.float32(delta)
    base = rng.uniform(-1000, 1000, 4000).astype(np.float32)
    grid = (np.arange(-20, 21, dtype=np.float32) * d32)
    c_all = np.concatenate([base, grid, grid + ml.half_cell(delta), np.float32(grid + 0.25 * d32), [np.float32(0.0)]]).astype(np.float32)
    r_all = ml.band(delta)
    out = np.zeros(2, np.float32)
    lib = hostemu()
    for i, c in enumerate(c_all):
        k = 1 + i % 63
        bit = (i // 63) & 1
        q = int(orc._quant_index(np.array([c], np.float32), delta)[0])
        c0 = np.float32(orc._requantised(np.array([q]), delta)[0])
        if (q & 1) != bit:
            q += 1 if c > c0 else (-1 if c < c0 else (1 if bit else -1))
        ct = np.float32(orc._requantised(np.array([q]), delta)[0])
        want = np.minimum(np.maximum(c, np.float32(ct - r_all[k])), np.float32(ct + r_all[k]))
        lib.mm_coefficient(float(c), bit, float(delta), k, qm, out.ctypes.data)
        assert out[0] == want, (c, bit, k)
        assert out[1] == np.float32(want - c), (c, bit, k)
        if abs(float(c) - float(ct)) <= float(r_all[k]):
            assert out[0].tobytes() == c.tobytes() or c == 0    # inside the band: the forward-transform value, bit for bit
            assert out[1] == 0.0


def test_guarded_bodies_equal_the_exact_bodies_on_24000_blocks():
    frames = np.stack([nl.content(("noise", "smooth", "letterbox", "noise", "flat")[k], 480, 640, seed=10 + k) for k in range(5)])
    blocks = 5 * 60 * 80
    assert blocks >= 20000
    replayed = 0
    for n, delta in ((3, 20), (7, 8), (10, 20), (15, 7.3), (10, 40)):
        bits = nl.payload(blocks * n - 3, seed=n)
        a, used_a, info_a = ml.host_embed(frames, delta, n, bits)
        b, used_b, info_b = ml.host_embed(frames, delta, n, bits, pocketfft=True)
        assert info_a["path"] == STREAMING and info_b["path"] == EXACT and used_a == used_b == bits.size
        assert np.array_equal(a, b), (n, delta)
        assert 0 < info_a["replayed"] < blocks
        replayed += info_a["replayed"]
    assert replayed > 4800          # the constant blocks alone


# ---- 4. what the rule promises -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [4, 6.5])
@pytest.mark.parametrize("kind", KINDS)
def test_small_steps_give_the_nearest_rules_bytes(kind, delta):
    """every r_k is 0: the clamp runs and writes the lattice point"""
    assert not ml.band(delta)[1:].any()
    g = nl.content(kind, 64, 96, seed=3)
    for n in (3, 10, 20, 63):
        bits = nl.payload(96 * n - 5, seed=n)
        want = nl.model_embed(g, delta, bits, n)[1]
        assert np.array_equal(ml.model_embed(g, delta, bits, n)[1], want)
        for pocketfft in (False, True):
            got, _, info = ml.host_embed(g, delta, n, bits, pocketfft=pocketfft)
            assert info["word"] > 1                                     # the minimum-move bodies, not a re-route to the nearest ones
            assert np.array_equal(got[0], want)
            assert np.array_equal(nl.host_embed(g, delta, n, bits, pocketfft=pocketfft)[0][0], want)


def _errors(stego, delta, n, bits):
    return int((orc.frame_extract_bits(stego, delta, n)[:bits.size] != bits).sum())


@pytest.mark.parametrize("kind,n,delta", sorted(ml.MEASURED))
def test_payload_reads_back_where_nothing_clips(kind, n, delta):
    """one 480 x 640 frame at full capacity, the settings of the header's table.  On content whose model stego has no pixel at 0
    or 255 - noise in [64, 192) at delta = 40 and at n = 63 (where [16, 240) clips), in [16, 240) otherwise; the precondition is
    asserted - the oracle's extraction returns the payload; the reference's own stego does too, except at n = 63 (not
    compared).  The table's own content (it clips at n = 63) reads back without an error as well, as the table says."""
    bits = nl.payload(4800 * n)
    g = ml.noclip_content(40 if n == 63 else delta)
    _, stego, used = ml.model_embed(g, delta, bits, n)
    assert used == bits.size
    assert stego.min() > 0 and stego.max() < 255                          # the precondition
    assert _errors(stego, delta, n, bits) == 0
    assert np.array_equal(ml.host_embed(g, delta, n, bits)[0][0], stego)
    if n != 63:
        assert _errors(orc.frame_embed(g, delta, bits, n)[1], delta, n, bits) == 0
    table = nl.content(kind)
    assert _errors(ml.model_embed(table, delta, bits, n)[1], delta, n, bits) == 0


@pytest.mark.parametrize("kind,n,delta", sorted(ml.MEASURED))
def test_psnr_table_of_the_header(kind, n, delta):
    """the CPU-measured table of include/svsdct.h: reference < SVS_NEAREST < SVS_MINMOVE, each within 0.02 dB of the listed value"""
    g = nl.content(kind)
    bits = nl.payload(4800 * n)
    got = (ml.psnr(g, orc.frame_embed(g, delta, bits, n)[1]), ml.psnr(g, nl.model_embed(g, delta, bits, n)[1]),
           ml.psnr(g, ml.model_embed(g, delta, bits, n)[1]))
    print(kind, n, delta, "%.2f %.2f %.2f" % got)
    assert got[0] < got[1] < got[2]
    assert np.allclose(got, ml.MEASURED[(kind, n, delta)], atol=0.02), got
    text = open(os.path.join(CSRC, "..", "..", "include", "svsdct.h")).read()
    assert "%.2f / " % ml.MEASURED[(kind, n, delta)][2] in text


@pytest.mark.parametrize("delta", [8, 20, 40, 7.3, 12.5])
def test_move_bound_and_untouched_coefficients(delta):
    g = nl.content("noise", 128, 160, seed=4)
    for n in (3, 10, 63):
        bits = nl.payload(320 * n, seed=n)
        stats = {}
        ml.model_embed(g, delta, bits, n, stats=stats)
        c, new, ct, r = stats["c"], stats["new"], stats["ct"], stats["r"]
        move = np.abs(new.astype(np.float64) - c.astype(np.float64))
        assert move.max() <= delta + 1e-3 * delta
        inside = np.abs(c.astype(np.float64) - ct.astype(np.float64)) <= r.astype(np.float64)
        if delta >= 12:
            assert inside.mean() > 0.1
        assert np.array_equal(new[inside].view(np.uint32), c[inside].view(np.uint32))       # bit-identical
        assert np.all(np.abs(new.astype(np.float64) - ct) <= r.astype(np.float64) * (1 + 1e-6) + 1e-4)
        # never farther than the nearest rule's move
        assert np.all(move <= np.abs(ct.astype(np.float64) - c) + 1e-4)


# ---- 5. route and flags ---------------------------------------------------------------------------------------------------
def test_plan_carries_the_flag_on_streaming_and_exact_only():
    total = 96
    for bgr in (False, True):
        for pocketfft in (False, True):
            for delta, n, n_bits, path in ((20, 10, 500, EXACT if pocketfft else STREAMING), (20, 20, 500, EXACT),
                                           (5000.3, 3, 500, EXACT), (20, 10, 0, COPY), (0, 10, 500, ROUND_TRIP),
                                           (-1, 10, 500, ROUND_TRIP), (20, 0, 500, ROUND_TRIP), (20, 0, 0, COPY)):
                got = ml.plan(delta, n, total, n_bits, pocketfft, bgr)
                assert got[0] == path, (delta, n, n_bits, pocketfft, bgr)
                carried = path in (EXACT, STREAMING)
                assert got[1] == int(carried)
                assert got[3] == (ml.half_cell(delta) if carried else 0)
                assert (got[4] > 1) == carried
                assert ml.plan(delta, n, total, n_bits, pocketfft, bgr, minmove=False)[1] == 0
                assert ml.plan(delta, n, total, n_bits, pocketfft, bgr, minmove=False, nearest=True)[4] == int(carried)
    # the rule word: h as its bit pattern; a step so small that h is 0 or the smallest denormal is the nearest rule
    assert ml.plan(20, 10, total, 500)[4] == int(np.array([10.0], np.float32).view(np.uint32)[0])
    assert ml.plan(1e-46, 10, total, 500, pocketfft=True)[4] == 1


@pytest.mark.parametrize("pocketfft", [False, True])
def test_flag_has_no_effect_where_nothing_is_embedded(pocketfft):
    g = nl.content("noise", 32, 48)
    bits = nl.payload(200)
    for delta, n, n_bits in ((20, 0, 200), (0, 10, 200), (-3, 10, 200), (20, 10, 0), (20, 0, 0)):
        with_flag = ml.host_embed(g, delta, n, bits, n_bits=n_bits, pocketfft=pocketfft)
        without = ml.host_embed(g, delta, n, bits, n_bits=n_bits, pocketfft=pocketfft, minmove=False)
        assert with_flag[1] == without[1] == 0 and with_flag[2]["minmove"] == 0
        assert np.array_equal(with_flag[0], without[0])
        assert np.array_equal(with_flag[0][0], orc.frame_embed(g, delta, bits[:n_bits], n)[1])
        assert np.array_equal(ml.model_embed(g, delta, bits[:n_bits], n)[1], with_flag[0][0])


def _extract_calls(lib, flag):
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    gray = np.zeros((f, h, w), np.uint8)
    out = np.full(64, 0xAB, np.uint8)
    got = C.c_uint64(77)
    P = C.byref(planes)
    sel = coeffs.native_coeffs((9, 2, 17))
    rcs = [lib.svs_extract(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
           lib.svs_extract_dev(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None),
           lib.svs_extract_ordered(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
           lib.svs_extract_ordered_dev(gray.ctypes.data, P, None, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None),
           lib.svs_extract_str(gray.ctypes.data, P, 8.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got)),
           # delta <= 0 gives zeros whatever the mode bits say - but not with an embed flag
           lib.svs_extract_dev(gray.ctypes.data, P, 0.0, n_ac, out.ctypes.data, out.size, flag, C.byref(got), None)]
    rcs += [lib.svs_extract_select_dev(gray.ctypes.data, P, None, C.byref(sel), 8.0, out.ctypes.data, out.size, flag, C.byref(got), None),
            lib.svs_extract_select(gray.ctypes.data, P, None, C.byref(sel), 8.0, out.ctypes.data, out.size, flag, C.byref(got))]
    assert np.all(out == 0xAB)                                     # nothing written
    return rcs


def test_every_extract_call_refuses_the_flag():
    """refused before any device work, so this runs without a GPU"""
    lib = native.load()
    for flag in (native.SVS_MINMOVE, native.SVS_MINMOVE | native.SVS_EXACT_GUARDED, native.SVS_MINMOVE | native.SVS_EXACT_POCKETFFT,
                 native.SVS_MINMOVE | native.SVS_NEAREST):
        rcs = _extract_calls(lib, flag)
        assert len(rcs) == 8 and rcs == [native.SVS_ERR_INVALID_ARG] * len(rcs)


def test_embed_calls_accept_the_flag_and_unknown_flags_stay_unknown():
    """without a GPU: an in-place device-pointer call with an empty payload passes every check and returns SVS_OK before any
    device work (the COPY route in place) - with the flag, alone and with the flags it combines with; 0x4, 0x400 and 0x80000000
    next to it are refused by every embed call"""
    lib = native.load()
    assert native.SVS_MINMOVE == 0x1000
    f, h, w, n_ac = 1, 16, 16, 3
    planes = native.Planes.contiguous(f, h, w)
    gray = np.zeros((f, h, w), np.uint8)
    bgr = np.zeros((f, h, w, 3), np.uint8)
    bits = np.zeros(16, np.uint8)
    P = C.byref(planes)
    done = C.c_uint64(7)
    counts = native.ReadbackCounts()
    bad = native.SVS_ERR_INVALID_ARG
    mm = native.SVS_MINMOVE
    sel = coeffs.native_coeffs((9, 2, 17))
    G, B = gray.ctypes.data, bits.ctypes.data

    def in_place_empty(flag):
        return [lib.svs_embed_dev(G, G, P, 8.0, n_ac, B, 0, 0, flag, C.byref(done), None),
                lib.svs_embed_ordered_dev(G, G, P, None, 8.0, n_ac, B, 0, 0, flag, C.byref(done), None),
                lib.svs_embed_readback_dev(G, G, P, None, 8.0, n_ac, B, 0, 0, flag, C.byref(done), None, None),
                lib.svs_embed_select_dev(G, G, P, None, C.byref(sel), 8.0, B, 0, 0, flag & ~native.SVS_READBACK, C.byref(done), None)]

    for extra in (0, native.SVS_EXACT_GUARDED, native.SVS_EXACT_POCKETFFT, native.SVS_NEAREST, native.SVS_READBACK):
        assert in_place_empty(mm | extra) == [0] * 4, hex(extra)
    assert not gray.any()
    for unknown in (0x4, 0x400, 0x80000000):
        flag = mm | unknown
        assert in_place_empty(flag) == [bad] * 4, hex(unknown)
        assert lib.svs_embed(G, G, P, 8.0, n_ac, B, 0, 8, flag, C.byref(done)) == bad
        assert lib.svs_embed_str(G, None, G, P, 8.0, n_ac, b"01010101", 8, flag, C.byref(done)) == bad
        assert lib.svs_embed_ordered(G, G, P, None, 8.0, n_ac, B, 0, 8, flag, C.byref(done)) == bad
        assert lib.svs_embed_readback(G, G, P, None, 8.0, n_ac, B, 0, 8, flag, C.byref(done), C.byref(counts)) == bad
        assert lib.svs_embed_select(G, G, P, None, C.byref(sel), 8.0, B, 0, 8, flag, C.byref(done)) == bad
        assert lib.svs_embed_bgr(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, B, 0, 8, flag, C.byref(done)) == bad
        assert lib.svs_embed_bgr_readback(bgr.ctypes.data, bgr.ctypes.data, None, P, None, 8.0, n_ac, B, 0, 8, flag, C.byref(done),
                                          C.byref(counts)) == bad
    # SVS_KEEP_COLOUR stays a colour-only flag next to the new one
    assert lib.svs_embed_dev(G, G, P, 8.0, n_ac, B, 0, 0, native.SVS_KEEP_COLOUR | mm, C.byref(done), None) == bad


def test_python_surface():
    for fn in (batch.embed_frames, batch.embed_device, batch.embed_bgr_device, batch.embed_bgr_frames, FramePipeline.__init__):
        assert inspect.signature(fn).parameters["minmove"].default is False, fn
    for fn in (batch.extract_frames, batch.extract_device, batch.extract_bgr_frames):
        assert "minmove" not in inspect.signature(fn).parameters
    assert batch.embed_flags("guarded", minmove=True) == native.SVS_EXACT_GUARDED | 0x1000
    assert batch.embed_flags("guarded", nearest=True, minmove=True) == native.SVS_EXACT_GUARDED | 0x1800
    assert batch.embed_flags("guarded") == native.SVS_EXACT_GUARDED


def test_drop_in_parses_the_switch(monkeypatch):
    """read the way SVS_NEAREST is: at import, "1" switches it on; extract_process has no such switch"""
    import importlib
    emb, ext = _install(monkeypatch, "emu")
    assert emb.MINMOVE is False
    try:
        for value, want in (("1", True), ("0", False), ("yes", False)):
            monkeypatch.setenv("SVS_MINMOVE", value)
            assert importlib.reload(emb).MINMOVE is want
            assert emb.NEAREST is False and emb.READBACK is False
    finally:
        monkeypatch.delenv("SVS_MINMOVE")
        importlib.reload(emb)
    assert emb.MINMOVE is False and not hasattr(ext, "MINMOVE")
