"""CPU tier of the soft-margin pass (svs_stepped_embed_readback_margin*, include/svsdct.h): the one-lane forms of
csrc/svs_readback.hpp, built for the host (tests/hostemu/readback_margin_emu.cpp),
  (a) at gate 0 are the stepped read-back: stepped_readback_lib.host_readback's bytes, statuses and counts;
  (b) report strong only what the receiver's NumPy soft bytes (stepped_soft_lib) find strong, leave every weak block on the
      read-back's bytes, and touch nothing else; the read-back's counts do not depend on the gate, and the pass never adds a
      wrong bit;
  (c) the library exports the two calls and refuses what the header says, the Python switches and the drop-in loop likewise;
  (d) and the README's experiment table is the one computed here."""
import functools
import os

import numpy as np
import pytest

import readback_margin_lib as rml
import stepped_lib as stl
import stepped_readback_lib as srl
from svsdct import batch, native
from svsdct import steps as steps_mod


@pytest.fixture(scope="module", autouse=True)
def _emu(tmp_path_factory):
    rml.emu(tmp_path_factory.mktemp("readback_margin_emu"))
    srl.emu(tmp_path_factory.mktemp("stepped_readback_emu"))


# every option set with every content; the tables rotate (5 and 32 share no factor with the stride)
CASES = [(list(rml.TABLES)[(3 * i + j) % len(rml.TABLES)], kind) + opt
         for i, opt in enumerate(rml.OPTION_SETS) for j, kind in enumerate(rml.CONTENTS)]


def _id(case):
    tname, kind, index, dither, order, rule = case
    return f"{tname}-{kind}-n{len(index)}k{index[0]}-{'d' if dither else 'p'}{'o' if order else 'r'}-{rule}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """-> the case's plain stego, payload, keywords, and its gate-0 result (computed once, never written to)"""
    tname, kind, index, dither, order, rule = case
    s0, bits, kw, opts = rml.case_stego(tname, kind, index, dither, order, rule)
    return s0, bits, kw, opts, rml.host_margin(s0, rml.TABLES[tname], len(index), bits, 0, **kw)


# ---- (a) gate 0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gate_0_is_the_stepped_read_back(case):
    tname, index = case[0], case[2]
    s0, bits, kw, _, (out, counts, st1, st2) = _case(case)
    want, want_counts, want_status = srl.host_readback(s0, rml.TABLES[tname], len(index), bits, **kw)
    assert counts == want_counts + (0, 0)
    assert np.array_equal(st1, want_status)
    assert np.array_equal(out, want)
    assert np.array_equal(st2 == 3, want_status == 3) and not st2[st2 != 3].any()


# ---- (b) the independent verdict and the invariants ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_receivers_soft_bytes_confirm_every_verdict(case):
    """for every gate: a block reported strong (pass-2 status 0) or strengthened (1) has every hard bit right and every m >= g in
    the NumPy soft bytes of the output; a weak block (2) decodes, has some m < g and keeps the read-back's bytes; a skipped block
    (4) has a wrong bit, is the read-back's unrepaired block and keeps its bytes; a block outside the budget (3) keeps the plain
    stego's; only strengthened blocks differ from the read-back's output.  repaired / unrepaired are the gate-0 call's, and the
    payload read directly has no more wrong bits than after the gate-0 call."""
    tname, kind, index, dither, order, rule = case
    table, n = rml.TABLES[tname], len(index)
    s0, bits, kw, opts, (p1, c1, s1, _) = _case(case)
    slot = rml.slot_of_block(s0.shape, bits.size, n, opts[2], opts[1])
    carries = slot >= 0
    blocks0 = np.concatenate([stl._to_blocks(f) for f in s0])
    blocks1 = np.concatenate([stl._to_blocks(f) for f in p1])
    errors1 = srl.bit_errors(p1, table, bits, index, *opts)
    for g in rml.GATES:
        out, counts, st1, st2 = rml.host_margin(s0, table, n, bits, g, **kw)
        wrong, m_min = rml.soft_slots(out, table, bits, index, *opts)
        print(f"{_id(case)}, g = {g}: counts {counts}, smallest m of a strong block "
              f"{m_min[slot[carries & (st2 <= 1)]].min() if (carries & (st2 <= 1)).any() else '-'}")
        assert np.array_equal(st1, s1) and counts[:2] == c1[:2]
        assert counts == (int((st1 == 1).sum()), int((st1 == 2).sum()), int((st2 == 1).sum()), int((st2 == 2).sum()))
        assert np.array_equal(st2 == 3, ~carries) and np.array_equal(st2 == 4, st1 == 2)
        blocks = np.concatenate([stl._to_blocks(f) for f in out])
        strong = carries & (st2 <= 1)
        assert not wrong[slot[strong]].any() and (m_min[slot[strong]] >= g).all()
        weak = st2 == 2
        assert not wrong[slot[weak]].any() and (m_min[slot[weak]] < g).all()
        assert wrong[slot[st2 == 4]].all()
        assert np.array_equal(blocks[st2 != 1], blocks1[st2 != 1])
        assert np.array_equal(blocks[~carries], blocks0[~carries])
        assert srl.bit_errors(out, table, bits, index, *opts) <= errors1


def test_a_high_gate_finds_work_and_a_low_one_little():
    """the cases are not vacuous: over all of them gate 64 strengthens blocks, gate 127 leaves weak ones, and gate 1 finds fewer
    blocks to look at than gate 64"""
    total = {g: np.zeros(4, np.int64) for g in (1, 64, 127)}
    for case in CASES[::5]:
        tname, index = case[0], case[2]
        s0, bits, kw, _, _ = _case(case)
        for g in total:
            total[g] += rml.host_margin(s0, rml.TABLES[tname], len(index), bits, g, **kw)[1]
    print({g: tuple(int(v) for v in c) for g, c in total.items()})
    assert total[64][2] > 0 and total[127][3] > 0
    assert total[1][2] + total[1][3] < total[64][2] + total[64][3]


# ---- (c) symbols and refusals ----------------------------------------------------------------------------------------------
def test_the_library_exports_the_calls_and_refuses_as_the_header_says():
    rml.check_refusals(native.load())


def test_python_switch_refusals():
    frames = np.zeros((1, 8, 8), np.uint8)
    bits = np.zeros(3, np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    table = stl.uniform(20)
    for g in (0, 128, -1, 64.0, True, "64"):
        with pytest.raises(ValueError, match="readback_margin is an int in 1..127"):
            batch.embed_frames(frames, 20, 3, bits, steps=table, readback_margin=g)
        with pytest.raises(ValueError, match="readback_margin is an int in 1..127"):
            batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, steps=table, readback_margin=g)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_frames(frames, 20, 3, bits, readback_margin=64)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, readback_margin=64)
    for kw in (dict(readback=True), dict(readback_keyed=True)):
        with pytest.raises(ValueError, match="readback_stepped is a path of its own"):
            batch.embed_frames(frames, 20, 3, bits, steps=table, readback_margin=64, **kw)
        with pytest.raises(ValueError, match="readback_stepped is a path of its own"):
            batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, steps=table, readback_margin=64, **kw)


def test_pipeline_passes_the_gate_through(monkeypatch):
    """FramePipeline(readback_margin=g) refuses what embed_frames refuses, hands embed_device that one read-back keyword and a
    counts buffer of four uint64"""
    from svsdct import pipeline
    with pytest.raises(ValueError, match="needs steps"):
        pipeline.FramePipeline(8, 8, 1, 20, 3, readback_margin=64)
    with pytest.raises(ValueError, match="readback_margin is an int in 1..127"):
        pipeline.FramePipeline(8, 8, 1, 20, 3, steps=stl.uniform(20), readback_margin=128)
    seen, sizes = {}, []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    monkeypatch.setattr(pipeline.native, "ensure_device", lambda d: None)
    monkeypatch.setattr(pipeline.native, "load", lambda: Lib())
    monkeypatch.setattr(pipeline.native, "check", lambda rc, what: None)
    monkeypatch.setattr(pipeline, "_pinned", lambda n: (0, np.zeros(n, np.uint8)))
    monkeypatch.setattr(pipeline, "_device", lambda n: sizes.append(n) or type("P", (), {"value": 4096})())
    monkeypatch.setattr(pipeline.batch, "embed_device", lambda *a, **kw: seen.update(kw) or 0)
    pipe = pipeline.FramePipeline(8, 8, 1, 20, 3, depth=1, steps=steps_mod.uniform(20), readback_margin=64, dither_key=5)
    pipe.submit_embed(0, 1, 0, first_frame=2)
    assert seen["readback_margin"] == 64 and not {"readback", "readback_keyed", "readback_stepped"} & set(seen)
    assert seen["d_counts"] == 4096 and 32 in sizes and seen["first_frame"] == 2


def test_embed_repeated_frames_passes_the_gate_through(monkeypatch):
    seen = {}
    monkeypatch.setattr(batch, "embed_frames",
                        lambda frames, delta, n_ac, stream, **kw: seen.update(kw) or (frames, stream.size, batch.MarginCounts(1, 0, 2, 3)))
    out = batch.embed_repeated_frames(np.zeros((1, 8, 8), np.uint8), 1.0, 3, [1, 0], steps=stl.uniform(20), readback_margin=64)
    assert seen["readback_margin"] == 64 and out[1:] == (3, 2, batch.MarginCounts(1, 0, 2, 3))


def test_drop_in_reads_the_gate(monkeypatch, capsys):
    """SVS_READBACK_MARGIN=g needs SVS_STEPS, must be 1..127, and is refused with the other read-back switches"""
    import embed_process as emb
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY", "SVS_STEPS"):
        monkeypatch.delenv(name, raising=False)
    switches = ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR", "READBACK_KEYED")
    for other in switches + ("READBACK_STEPPED",):
        monkeypatch.setattr(emb, other, False)
    monkeypatch.setattr(emb, "READBACK_MARGIN", "64")
    assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
    out = capsys.readouterr().out
    assert "Error: SVS_READBACK_MARGIN memerlukan SVS_STEPS." in out and out.count("Error:") == 1
    monkeypatch.setenv("SVS_STEPS", "q75x2")
    for bad in ("0", "128", "x"):
        monkeypatch.setattr(emb, "READBACK_MARGIN", bad)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        assert "Error: SVS_READBACK_MARGIN harus bilangan bulat 1..127" in capsys.readouterr().out
    monkeypatch.setattr(emb, "READBACK_MARGIN", "64")
    for switch in switches:
        for other in switches:
            monkeypatch.setattr(emb, other, other == switch)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        out = capsys.readouterr().out
        assert "tidak dapat dipakai bersama" in out and "SVS_" + switch in out and out.count("Error:") == 1


# ---- (d) the experiment table ----------------------------------------------------------------------------------------------
def test_the_experiment_table():
    """README.md, "soft-margin pass": three 96 x 160 frames, one 2 400-bit copy per frame, 10 coefficients, reference rule, no
    dither, no order, the luminance requantisation model.  Asserted: on noise under matched(75, 2), row-major 1..10, the errors
    after Q = 75 with the pass at g = 64 are below half of those with the read-back alone; on the two letterbox rows they are 0.
    The other cells are measurements - the uniform-20 row gains nothing at Q = 75, where its lattice, not its margin, fails."""
    rows = rml.experiment_table()
    text = rml.format_experiment(rows)
    print("\n" + text)
    by = dict(rows)
    noise = by[rml.NOISE_ROW]["gates"]
    g, q = rml.ASSERTED_GATE, rml.ASSERTED_Q
    assert noise[0]["q"][q] > 0 and 2 * noise[g]["q"][q] < noise[0]["q"][q]
    for key in rml.LETTERBOX_ROWS:
        assert by[key]["gates"][g]["q"][q] == 0, key
    for key, row in rows:
        for gate, cell in row["gates"].items():
            assert cell["counts"][:2] == row["gates"][0]["counts"][:2], (key, gate)
            assert cell["direct"] <= row["gates"][0]["direct"], (key, gate)
    readme = [line.strip() for line in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md"))]
    lines = text.split("\n")
    at = readme.index(lines[0])
    assert readme[at:at + len(lines)] == lines, "README.md's soft-margin table is not the one computed here"
