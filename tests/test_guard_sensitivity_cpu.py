"""The suite goes red when the streaming embed's guard (BETA, make_guard) or FAST extraction's tie margin (make_qim) is too
tight - CPU tier, on hostemu (the kernels' per-block arithmetic) and the oracle.

tests/golden/guard_corpus.npz holds, per kernel family, frames whose corpus blocks sit at the guard's boundary: for each, s*
is the largest guard scale at which the cheap path keeps the block and its pixels differ from the reference (t* the same
for extraction and the tie margin; tests/golden/make_guard_corpus.py).  At scale 1 every pixel and bit is the oracle's; at
0.9 x max s* exactly the blocks with s* above the scale differ.  The GPU tier (test_gpu_guard_sensitivity.py) checks that
the kernels make the same decisions."""
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import qim_dct_oracle as orc
from testlib import REPO, emu_embed, emu_extract, emu_scales, guard_corpus_case

GOLDEN = os.path.join(REPO, "tests", "golden")
META = json.load(open(os.path.join(GOLDEN, "guard_corpus.json")))
EMBED = sorted(META["embed"])
EXTRACT = sorted(META["extract"])


def _gen():
    spec = importlib.util.spec_from_file_location("make_guard_corpus", os.path.join(GOLDEN, "make_guard_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def corpus():
    return np.load(os.path.join(GOLDEN, "guard_corpus.npz"))


def embed_case(corpus, name):
    c = guard_corpus_case(corpus, META, name)
    return META["embed"][name], c["frame"], c["bits"], c["positions"], c["stars"]


def differing_blocks(a, b):
    h, w = a.shape[-2:]
    d = (a.reshape(-1, h // 8, 8, w // 8, 8) != b.reshape(-1, h // 8, 8, w // 8, 8)).any(axis=(2, 4))
    return np.flatnonzero(d.reshape(-1))


def test_corpus_covers_every_family():
    assert len(EMBED) == 9 and len(EXTRACT) == 5
    assert {m["delta"] for m in META["embed"].values()} >= {0.25, 4096.0}
    assert sorted(m["n_ac"] for m in META["extract"].values()) == [8, 10, 16, 36, 63]
    assert os.path.getsize(os.path.join(GOLDEN, "guard_corpus.npz")) < 250_000


@pytest.mark.parametrize("name", EMBED)
def test_embed_at_scale_one_is_the_oracle(corpus, name):
    m, frame, bits, positions, stars = embed_case(corpus, name)
    n, delta = m["n_ac"], m["delta"]
    ref, used = orc.batch_embed(frame[None], delta, bits, n)
    assert used == bits.size
    replayed = []
    got, _ = emu_embed(frame, delta, n, bits, exact=4, replayed=replayed)
    assert np.array_equal(got, ref)
    assert replayed[0] >= len(positions)             # every corpus block is undecided at scale 1
    assert np.array_equal(emu_extract(got, delta, n), orc.batch_extract_bits(ref, delta, n))


@pytest.mark.parametrize("name", EMBED)
def test_embed_below_max_s_star_differs_exactly_in_the_predicted_blocks(corpus, name):
    m, frame, bits, positions, stars = embed_case(corpus, name)
    n, delta, x = m["n_ac"], m["delta"], m["test_scale"]
    assert 0.89 * m["max_s_star"] < x < m["max_s_star"] == float(stars.max())
    ref, _ = orc.batch_embed(frame[None], delta, bits, n)
    with emu_scales(guard=x):
        got, _ = emu_embed(frame, delta, n, bits, exact=4)
    want = np.sort(positions[stars >= np.float32(x)])
    assert want.size >= 1
    assert np.array_equal(differing_blocks(got, ref), want)


@pytest.mark.parametrize("name", EMBED)
def test_stored_s_star_is_found_again(corpus, name):
    gen = _gen()
    m, frame, bits, positions, stars = embed_case(corpus, name)
    n = m["n_ac"]
    blocks = gen.frame_to_blocks(frame)
    per_block = bits.reshape(-1, n)
    for i in sorted({int(np.argmax(stars)), 0, len(stars) // 2, len(stars) - 1}):
        p = positions[i]
        assert gen.embed_star(blocks[p], per_block[p], n, m["delta"]) == float(stars[i]), (name, i)


_EMPIRICAL = {}


@pytest.mark.parametrize("name", EMBED)
def test_search_is_sharp(corpus, name):
    """each setting's max s* is at least half the largest err / BETA that tools/guard_bound.py measures by random sampling
    for the same row count and delta (the generator keeps searching until it gets there)."""
    m = META["embed"][name]
    key = (m["n_ac"], m["delta"])
    if key not in _EMPIRICAL:
        _EMPIRICAL[key] = _gen().empirical_err_over_beta(*key)
    assert _EMPIRICAL[key] == pytest.approx(m["empirical_max_err_over_beta"], rel=1e-9)
    assert m["max_s_star"] >= 0.5 * _EMPIRICAL[key], name


def extract_case(corpus, name):
    c = guard_corpus_case(corpus, META, name)
    return META["extract"][name], c["frame"], c["positions"], c["stars"]


@pytest.mark.parametrize("name", EXTRACT)
def test_extract_at_scale_one_is_the_oracle(corpus, name):
    m, frame, positions, stars = extract_case(corpus, name)
    redone = []
    got = emu_extract(frame, m["delta"], m["n_ac"], redone=redone)
    assert np.array_equal(got, orc.batch_extract_bits(frame[None], m["delta"], m["n_ac"]))
    assert redone[0] >= 1


@pytest.mark.parametrize("name", EXTRACT)
def test_extract_below_max_t_star_differs_exactly_in_the_predicted_blocks(corpus, name):
    m, frame, positions, stars = extract_case(corpus, name)
    n, x = m["n_ac"], m["test_scale"]
    assert 0.89 * m["max_t_star"] < x < m["max_t_star"] == float(stars.max())
    ref = orc.batch_extract_bits(frame[None], m["delta"], n).reshape(-1, n)
    with emu_scales(tie=x):
        got = emu_extract(frame, m["delta"], n).reshape(-1, n)
    want = np.sort(positions[stars >= np.float32(x)])
    assert want.size >= 1
    assert np.array_equal(np.flatnonzero((got != ref).any(1)), want)
    # the kernels take step two for a whole wave of 64 blocks when one is a candidate: the same bits at scale 1, and at x a
    # subset of the blocks above - still not empty, so the GPU tier sees the cut too
    assert np.array_equal(emu_extract(frame, m["delta"], n, wave=64), ref.reshape(-1))
    with emu_scales(tie=x):
        waved = emu_extract(frame, m["delta"], n, wave=64).reshape(-1, n)
    wrong = np.flatnonzero((waved != ref).any(1))
    assert wrong.size >= 1 and np.isin(wrong, want).all()


@pytest.mark.parametrize("name", EXTRACT)
def test_stored_t_star_is_found_again(corpus, name):
    gen = _gen()
    m, frame, positions, stars = extract_case(corpus, name)
    blocks = gen.frame_to_blocks(frame)
    for i in sorted({int(np.argmax(stars)), 0, len(stars) // 2, len(stars) - 1}):
        assert gen.extract_star(blocks[positions[i]], m["n_ac"], m["delta"]) == float(stars[i]), (name, i)
