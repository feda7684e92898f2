"""GPU tier of the guard checks under SVS_NEAREST and SVS_MINMOVE (CPU tier: test_guard_rules_cpu.py): on the frames of
tests/golden/guard_rules_corpus.npz - waves with 1, 8, 31, 32, 33, 64 (128) undecided blocks and one in every further wave,
boundary blocks with s* > 0 under the rule among them - the streaming kernels' rule bodies and their pooled replay make the
decisions of the host build of the bodies (tests/hostemu through minmove_lib.host_embed).

* product library, gray call with the flag in guarded, default and exact mode, and in place at the device-pointer level: the
  NumPy model's pixels;
* fused colour (B = G = R, the run-time QimRule::kind): the model's pixels in all three channels; keep-colour for one row1 and
  one row2 setting per rule;
* a keyed block order for one row1 and one row2 setting per rule, the frame's blocks permuted so that the undecided blocks
  sit in stream order where the layout put them (the KEYED instantiations' replays under a rule);
* experiments library, SVS_GUARD_SCALE = 1: the same bytes and the shim's replay count;
* SVS_GUARD_SCALE = 0.9 x max s*: the shim's bytes at that scale - not the model's, in the same blocks, same replay count -
  gray and colour."""
import functools
import os

import numpy as np
import pytest

import minmove_lib as ml
from kernel_matrix import FIRST_FRAME, KEY
from test_gpu_guard_sensitivity import counting, differing_blocks, in_place
from test_guard_rules_cpu import META, NAMES, rules_case
from test_keep_colour_cpu import gray_of
from testlib import REPO, experiments_library, using_library
from svsdct import batch, native, order

pytestmark = pytest.mark.gpu

W15 = (3735, 19235, 9798, 15)
# one row1 and one row2 setting per rule for the keep-colour and keyed-order runs
EXTRA = ("row1_one_block_per_lane__nearest", "row1_two_blocks_per_lane__minmove", "row2_n10__nearest", "row2_parked__minmove")


@pytest.fixture(scope="module")
def corpus():
    native.ensure_device(0)
    return np.load(os.path.join(REPO, "tests", "golden", "guard_rules_corpus.npz"))


def test_extra_settings_are_one_row1_and_one_row2_per_rule():
    got = sorted((META["settings"][k]["rule"], 1 if META["settings"][k]["n_ac"] <= 7 else 2) for k in EXTRA)
    assert got == [("minmove", 1), ("minmove", 2), ("nearest", 1), ("nearest", 2)]


@pytest.mark.parametrize("name", NAMES)
def test_rule_kernels_make_the_shims_guard_decisions(corpus, name, monkeypatch):
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    frame, bits = np.array(frame), np.array(bits)          # the shared case is read-only
    n, delta, x = m["n_ac"], m["delta"], m["test_scale"]
    flag = dict(minmove=m["rule"] == "minmove", nearest=m["rule"] == "nearest")
    host1, used, info1 = ml.host_embed(frame, delta, n, bits, **flag)
    assert used == bits.size and np.array_equal(host1[0], want) and info1["replayed"] == len(positions)
    host_x, _, info_x = ml.host_embed(frame, delta, n, bits, guard_scale=x, **flag)
    want_blocks = np.sort(positions[stars >= np.float32(x)])
    assert np.array_equal(differing_blocks(host_x[0], want), want_blocks) and want_blocks.size

    # product library: guarded, default and exact mode, in place
    for mode in ("guarded", None, "exact"):
        got, u = batch.embed_frames(frame[None], delta, n, bits, mode=mode, **flag)
        got = np.array(got)
        assert u == bits.size and np.array_equal(differing_blocks(got[0], want), []) and np.array_equal(got[0], want), (name, mode)
    with monkeypatch.context() as mp:
        mp.setattr(batch, "embed_device", functools.partial(batch.embed_device, **flag))
        assert np.array_equal(in_place(frame, delta, n, bits), want), name

    # fused colour path, B = G = R: gray is the plane itself with the default weights
    bgr = np.repeat(frame[None, ..., None], 3, axis=3)
    got_bgr, got_gray, u = batch.embed_bgr_frames(bgr, delta, n, bits, **flag)
    assert u == bits.size and np.array_equal(np.array(got_gray)[0], frame)
    assert np.array_equal(np.array(got_bgr)[0], np.repeat(want[..., None], 3, axis=2)), name

    exp = experiments_library()
    with using_library(exp):
        for scale, wanted, rep in (("1", want, info1["replayed"]), (repr(x), host_x[0], info_x["replayed"])):
            monkeypatch.setenv("SVS_GUARD_SCALE", scale)
            with counting(exp) as c:
                got, _ = batch.embed_frames(frame[None], delta, n, bits, mode="guarded", **flag)
            got = np.array(got)[0]
            assert np.array_equal(differing_blocks(got, want), differing_blocks(wanted, want)), (name, scale)
            assert np.array_equal(got, wanted), (name, scale)
            assert c.value == rep, (name, scale, c.value, rep)
            got_bgr, _, _ = batch.embed_bgr_frames(bgr, delta, n, bits, mode="guarded", **flag)
            assert np.array_equal(np.array(got_bgr)[0], np.repeat(wanted[..., None], 3, axis=2)), (name, scale, "bgr")
        monkeypatch.delenv("SVS_GUARD_SCALE")


@pytest.mark.parametrize("name", EXTRA)
def test_keep_colour_and_keyed_order_under_a_rule(corpus, name, monkeypatch):
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    frame, bits = np.array(frame), np.array(bits)          # the shared case is read-only
    n, delta = m["n_ac"], m["delta"]
    flag = dict(minmove=m["rule"] == "minmove", nearest=m["rule"] == "nearest")
    bgr = np.repeat(frame[None, ..., None], 3, axis=3)
    for mode in ("guarded", "exact"):
        kept = np.array(batch.embed_bgr_frames(bgr, delta, n, bits, mode=mode, keep_colour=True, **flag)[0])[0]
        assert np.array_equal(gray_of(kept, W15), want), (name, mode)
        same = want == frame
        assert np.array_equal(kept[same], bgr[0][same]), (name, mode)
    # keyed order: stream slot j of the call is block j of the corpus frame
    src = order.unpermute_blocks(frame[None], KEY, FIRST_FRAME)
    assert np.array_equal(order.permute_blocks(src, KEY, FIRST_FRAME)[0], frame) and not np.array_equal(src[0], frame)
    want_keyed = order.unpermute_blocks(want[None], KEY, FIRST_FRAME)
    for mode in ("guarded", None, "exact"):
        got, u = batch.embed_frames(src, delta, n, bits, mode=mode, block_key=KEY, first_frame=FIRST_FRAME, **flag)
        assert u == bits.size and np.array_equal(np.array(got), want_keyed), (name, mode)
    exp = experiments_library()
    with using_library(exp):
        monkeypatch.setenv("SVS_GUARD_SCALE", "1")
        with counting(exp) as c:
            got, _ = batch.embed_frames(src, delta, n, bits, mode="guarded", block_key=KEY, first_frame=FIRST_FRAME, **flag)
        assert np.array_equal(np.array(got), want_keyed) and c.value == len(positions), (name, c.value)
        monkeypatch.delenv("SVS_GUARD_SCALE")
