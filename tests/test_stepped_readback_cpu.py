"""CPU tier of the stepped read-back (svs_stepped_embed_readback*, include/svsdct.h): the one-lane stepped forms of
csrc/svs_readback.hpp, built for the host (tests/hostemu/stepped_readback_emu.cpp),
  (a) equal the keyed forms at delta = D under a uniform table D, in bytes, counts and status;
  (b) accept only blocks that the independent NumPy extraction of the stepped format decodes, non-uniform tables included;
  (c) take the reciprocal make_qim takes: 1.0f / dk == inv_delta_f for every integer step;
  (d) the Python switches and the drop-in loop refuse what the issue says they refuse;
  (e) and the README's experiment table is the one computed here."""
import numpy as np
import pytest

import dither_lib as dl
import keyed_readback_lib as kl
import stepped_lib as stl
import stepped_readback_lib as srl
from readback_lib import content
from svsdct import batch, native
from svsdct import steps as steps_mod

H, W = 96, 160
T = 3
SELECTIONS = {"prefix10": kl.prefix(10), "zigzag10": kl.zigzag(10), "zigzag3@6": kl.zigzag(3, 6), "prefix63": kl.prefix(63)}
CLIPPING = ("letterbox", "bright", "flat0")


@pytest.fixture(scope="module", autouse=True)
def _emu(tmp_path_factory):
    srl.emu(tmp_path_factory.mktemp("stepped_readback_emu"))


def _bits(index):
    return dl.payload((H // 8) * (W // 8) * len(index) - 7)


# ---- (a) the uniform identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CLIPPING)
@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("tname", srl.UNIFORM)
def test_uniform_table_is_the_keyed_form(tname, sel, dither, kind):
    d, index = srl.UNIFORM[tname], SELECTIONS[sel]
    g = content(kind, H, W)
    bits = _bits(index)
    key = kl.DITHER_KEY if dither else None
    s0, used = dl.model_embed(g, d, bits, rule="reference", index=index, key=key, t=T)
    assert used == bits.size
    want, want_counts, want_status = kl.host_readback(s0, d, len(index), bits, index=index, dither_key=key, first_frame=T)
    got, counts, status = srl.host_readback(s0, stl.uniform(d), len(index), bits, index=index, dither_key=key, first_frame=T)
    print(f"{tname}, {sel}, dither {dither}, {kind}: keyed counts {want_counts}, stepped counts {counts}")
    # black areas always clip; whether a bright block loses a bit depends on the selection and the dither
    assert kind == "bright" or sum(want_counts) > 0, "the case must have failing blocks"
    assert counts == want_counts
    assert np.array_equal(status, want_status)
    assert np.array_equal(got, want)


def test_uniform_table_is_the_keyed_form_under_an_order_and_an_offset():
    """a batch of frames, a keyed order, a bit offset and a payload that ends inside a block"""
    d, index, off = 16, kl.zigzag(10), 45
    frames = srl.frames_of("letterbox", (2, 56, 136))
    n_bits = 2 * 7 * 17 * 10 - 13
    stream = dl.payload(off + n_bits + 50)
    s0, used = dl.model_batch_embed(frames, d, stream[off:off + n_bits], 10, "minmove", index, kl.DITHER_KEY, T, srl.ORDER_KEY)
    assert used == n_bits
    kw = dict(index=index, dither_key=kl.DITHER_KEY, block_key=srl.ORDER_KEY, first_frame=T, bit_offset=off, n_bits=n_bits)
    want, want_counts, want_status = kl.host_readback(s0, d, 10, stream, **kw)
    got, counts, status = srl.host_readback(s0, stl.uniform(d), 10, stream, **kw)
    assert want_counts[0] > 10
    assert counts == want_counts and np.array_equal(status, want_status) and np.array_equal(got, want)


# ---- (b) acceptance --------------------------------------------------------------------------------------------------------
ACCEPT_TABLES = {"m75x2": stl.matched(75, 2), "m95x2f16": stl.matched(95, 2, 16), "odd": stl.odd_steps(),
                 "u20": stl.uniform(20), "u16": stl.uniform(16), "u7": stl.uniform(7)}


@pytest.mark.parametrize("kind", CLIPPING)
@pytest.mark.parametrize("dither", (False, True), ids=("plain", "dither"))
@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("tname", ACCEPT_TABLES)
def test_every_accepted_block_decodes(tname, sel, dither, kind):
    """status 0 (reads back) and 1 (repaired): the NumPy extraction of stepped_lib reads every payload bit of the block; status 2
    keeps the plain stego's bytes; the counts are the statuses'"""
    table, index = ACCEPT_TABLES[tname], SELECTIONS[sel]
    n = len(index)
    g = content(kind, H, W)
    bits = _bits(index)
    key = kl.DITHER_KEY if dither else None
    rule = stl.RULES[(len(tname) + n + dither) % 3]
    s0, used = stl.model_embed(g, table, bits, n, rule, index, key, T)
    assert used == bits.size
    out, counts, status = srl.host_readback(s0, table, n, bits, index=index, dither_key=key, first_frame=T)
    nslot = -(-bits.size // n)
    assert (status[:nslot] != 3).all() and (status[nslot:] == 3).all()
    assert counts == (int((status == 1).sum()), int((status == 2).sum()))
    before = srl.wrong_slots(s0[None], table, bits, index, key, T)
    after = srl.wrong_slots(out[None], table, bits, index, key, T)
    st = status[:nslot]
    assert np.array_equal(before, st != 0)                       # the check is the receiver's verdict
    assert not after[st != 2].any()                              # accepted blocks decode
    assert np.array_equal(after[st == 2], before[st == 2])
    touched = (stl._to_blocks(out) != stl._to_blocks(s0)).any(axis=1)
    assert not touched[status != 1].any()                        # only repaired blocks change
    print(f"{tname}, {sel}, dither {dither}, {kind}, {rule}: {int(before.sum())} failing -> {counts}")


def test_the_delivery_setting_leaves_nothing_unrepaired():
    """the setting of the GPU tier's delivery test (matched(75, 2), zig-zag 1..10, dither, block key, minimum-move rule, one
    letterboxed 96 x 160 frame): the plain stepped stego has wrong bits, the pass repairs every failing block"""
    table, index, rule = srl.DELIVERY
    frame = kl.table_frame("letterbox")[None]
    bits = dl.payload(240 * 10 - 7)
    opts = (kl.DITHER_KEY, kl.TABLE_T, srl.ORDER_KEY)
    s0, used = srl.model_stego(frame, table, bits, index, rule, *opts)
    assert used == bits.size
    out, counts, _ = srl.host_readback(s0, table, 10, bits, index=index, dither_key=kl.DITHER_KEY, block_key=srl.ORDER_KEY,
                                       first_frame=kl.TABLE_T)
    print(f"counts {counts}; wrong bits without / with: {srl.bit_errors(s0, table, bits, index, *opts)} / "
          f"{srl.bit_errors(out, table, bits, index, *opts)}")
    assert counts[0] > 0 and counts[1] == 0
    assert srl.bit_errors(s0, table, bits, index, *opts) > 0 and srl.bit_errors(out, table, bits, index, *opts) == 0


# ---- (c) the reciprocal ----------------------------------------------------------------------------------------------------
def test_the_reciprocal_is_make_qims():
    own, qim = srl.reciprocals(4095)
    assert np.array_equal(own.view(np.uint32), qim.view(np.uint32))
    assert np.array_equal(own, np.float32(1.0) / np.arange(1, 4096, dtype=np.float32))


# ---- (d) refusals ----------------------------------------------------------------------------------------------------------
def test_python_switch_refusals():
    frames = np.zeros((1, 8, 8), np.uint8)
    bits = np.zeros(3, np.uint8)
    planes = native.Planes.contiguous(1, 8, 8)
    table = stl.uniform(20)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_frames(frames, 20, 3, bits, readback_stepped=True)
    with pytest.raises(ValueError, match="needs steps"):
        batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, readback_stepped=True)
    for kw in (dict(readback=True), dict(readback_keyed=True)):
        with pytest.raises(ValueError, match="readback_stepped is a path of its own"):
            batch.embed_frames(frames, 20, 3, bits, steps=table, readback_stepped=True, **kw)
        with pytest.raises(ValueError, match="readback_stepped is a path of its own"):
            batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, steps=table, readback_stepped=True, **kw)
        # the refusals that were there stay, word for word
        with pytest.raises(ValueError, match="per-coefficient steps have no read-back form"):
            batch.embed_frames(frames, 20, 3, bits, steps=table, **kw)
    with pytest.raises(ValueError, match="two paths"):
        batch.embed_device(64, 64, planes, 20, 3, 128, 0, 3, steps=table, readback_stepped=True, readback=True, readback_keyed=True)
    with pytest.raises(ValueError, match=r"delta\[1\]"):
        batch.embed_frames(frames, 20, 3, bits, steps=np.zeros(64, np.uint16), readback_stepped=True)


def test_pipeline_switch_refusals():
    from svsdct.pipeline import FramePipeline
    table = stl.uniform(20)
    with pytest.raises(ValueError, match="needs steps"):
        FramePipeline(8, 8, 1, 20, 3, readback_stepped=True)
    for kw in (dict(readback=True), dict(readback_keyed=True)):
        with pytest.raises(ValueError, match="readback_stepped is a path of its own"):
            FramePipeline(8, 8, 1, 20, 3, steps=table, readback_stepped=True, **kw)
        with pytest.raises(ValueError, match="read-back"):
            FramePipeline(8, 8, 1, 20, 3, steps=table, **kw)


def test_pipeline_passes_the_switch_through(monkeypatch):
    """FramePipeline(readback_stepped=True) hands embed_device that one read-back keyword, and the counts buffer"""
    from svsdct import pipeline
    seen = {}

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    monkeypatch.setattr(pipeline.native, "ensure_device", lambda d: None)
    monkeypatch.setattr(pipeline.native, "load", lambda: Lib())
    monkeypatch.setattr(pipeline.native, "check", lambda rc, what: None)
    monkeypatch.setattr(pipeline, "_pinned", lambda n: (0, np.zeros(n, np.uint8)))
    monkeypatch.setattr(pipeline, "_device", lambda n: type("P", (), {"value": 4096})())
    monkeypatch.setattr(pipeline.batch, "embed_device", lambda *a, **kw: seen.update(kw) or 0)
    pipe = pipeline.FramePipeline(8, 8, 1, 20, 3, depth=1, steps=steps_mod.uniform(20), readback_stepped=True, dither_key=5)
    pipe.submit_embed(0, 1, 0, first_frame=2)
    assert seen["readback_stepped"] is True and "readback" not in seen and "readback_keyed" not in seen
    assert seen["d_counts"] == 4096 and seen["first_frame"] == 2 and np.array_equal(seen["steps"], stl.uniform(20))


def test_embed_repeated_frames_passes_the_switch_through(monkeypatch):
    seen = {}
    monkeypatch.setattr(batch, "embed_frames",
                        lambda frames, delta, n_ac, stream, **kw: seen.update(kw) or (frames, stream.size, batch.ReadbackCounts(1, 0)))
    out = batch.embed_repeated_frames(np.zeros((1, 8, 8), np.uint8), 1.0, 3, [1, 0], steps=stl.uniform(20), readback_stepped=True)
    assert seen["readback_stepped"] is True and out[1:] == (3, 2, batch.ReadbackCounts(1, 0))


def test_drop_in_refusals(monkeypatch, capsys):
    """SVS_READBACK_STEPPED=1 needs SVS_STEPS, and is refused with every other read-back switch and SVS_KEEP_COLOUR; the
    refusals of SVS_STEPS with those switches stay"""
    import embed_process as emb
    for name in ("SVS_BLOCK_KEY", "SVS_COEFFS", "SVS_DITHER_KEY", "SVS_STEPS"):
        monkeypatch.delenv(name, raising=False)
    switches = ("KEEP_COLOUR", "READBACK", "READBACK_COLOUR", "READBACK_KEYED")
    for other in switches:
        monkeypatch.setattr(emb, other, False)
    monkeypatch.setattr(emb, "READBACK_STEPPED", True)
    assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
    out = capsys.readouterr().out
    assert "Error: SVS_READBACK_STEPPED=1 memerlukan SVS_STEPS." in out and out.count("Error:") == 1
    monkeypatch.setenv("SVS_STEPS", "q75x2")
    for stepped in (True, False):
        monkeypatch.setattr(emb, "READBACK_STEPPED", stepped)
        for switch in switches:
            for other in switches:
                monkeypatch.setattr(emb, other, other == switch)
            assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
            out = capsys.readouterr().out
            assert "tidak dapat dipakai bersama" in out and "SVS_" + switch in out and out.count("Error:") == 1
    # without SVS_STEPS the other switches do not excuse it either
    monkeypatch.delenv("SVS_STEPS")
    monkeypatch.setattr(emb, "READBACK_STEPPED", True)
    for switch in switches:
        for other in switches:
            monkeypatch.setattr(emb, other, other == switch)
        assert emb.embed_gambar_ke_video_final("in.mp4", "secret.png", "out", 20, 10, b"") == (False, None, None)
        assert "Error: SVS_READBACK_STEPPED" in capsys.readouterr().out


# ---- (e) the experiment table ----------------------------------------------------------------------------------------------
def test_the_experiment_table():
    """README.md, "stepped read-back": three letterboxed 96 x 160 frames, one 2 400-bit copy per frame, 10 coefficients.  The
    channel columns are measurements of the model, not promises: a repaired block is accepted because it decodes, not because it
    lies on a lattice point.  Asserted: the matched(75, 2), zig-zag 1..10, reference-rule row - the pass finds failing blocks,
    repairs every one, and the payload then reads back without an error; and for every row, that the direct column with the
    pass counts exactly the bits of the blocks left unrepaired (none where unrepaired is 0)."""
    rows = srl.experiment_table()
    text = srl.format_experiment(rows)
    print("\n" + text)
    by = dict(rows)
    r = by[srl.ASSERTED_ROW]
    assert r["failing"] > 0 and r["repaired"] == r["failing"] and r["unrepaired"] == 0
    assert r["direct"][0] > 0 and r["direct"][1] == 0
    assert np.isfinite(r["psnr"])
    for key, row in rows:
        assert row["repaired"] + row["unrepaired"] == row["failing"], key
        assert (row["direct"][1] == 0) == (row["unrepaired"] == 0), key
    import os
    readme = [line.strip() for line in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md"))]
    lines = text.split("\n")
    at = readme.index(lines[0])
    assert readme[at:at + len(lines)] == lines, "README.md's stepped read-back table is not the one computed here"
