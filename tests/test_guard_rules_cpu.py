"""SVS_NEAREST and SVS_MINMOVE on guard-boundary frames - CPU tier, on the host build of the streaming and exact bodies
(tests/hostemu through minmove_lib.host_embed: the library's route, rule word and RouteArgs::guard_scale) against the NumPy models of
nearest_lib / minmove_lib.

tests/golden/guard_rules_corpus.npz (tests/golden/make_guard_rules_corpus.py) holds one frame per kernel family and rule.  Its
undecided blocks fill waves with 1, 8, 31, 32, 33, 64 (128) entries and every further wave with one; among them sit the
boundary blocks, whose s* UNDER THE RULE is positive.  At scale 1 the shim gives the model's pixels and replays exactly the
listed blocks; at 0.9 x max s* it differs exactly in the blocks with s* at or above the scale.  The floors of max s* are half
the committed reference corpus's (guard_corpus.json) per kernel family.  A reference-rule block whose change vector under
SVS_NEAREST equals its reference change keeps its s* bit for bit: asserted for the whole reference corpus.  The GPU tier
(test_guard_rules_gpu.py) checks that the kernels make the same decisions."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import minmove_lib as ml
from testlib import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
META = json.load(open(os.path.join(GOLDEN, "guard_rules_corpus.json")))
REF_META = json.load(open(os.path.join(GOLDEN, "guard_corpus.json")))
NAMES = sorted(META["settings"])
MINMOVE = [k for k in NAMES if META["settings"][k]["rule"] == "minmove"]
# settings that stayed below their floor in the generator's run: name -> what it reached (none did)
BELOW_FLOOR = {}
# blocks of each committed reference setting whose SVS_NEAREST change vector is the reference's
CARRY_OVER = {"delta_max": 11, "delta_min": 66, "row1_double": 65, "row1_one_block_per_lane": 99, "row1_two_blocks_per_lane": 120,
              "row2_n10": 17, "row2_parked_double": 9, "row2_parked_f32": 18, "row2_worklist": 16}
TABLE = {"row1_two_blocks_per_lane": (3, 16.0, "pow2"), "row1_one_block_per_lane": (7, 20.0, "float32"),
         "row1_double": (5, 20.3, "double"), "row2_worklist": (9, 16.0, "pow2"), "row2_n10": (10, 20.0, "float32"),
         "row2_parked": (15, 20.3, "double")}


def _gen():
    if "make_guard_rules_corpus" in sys.modules:
        return sys.modules["make_guard_rules_corpus"]
    spec = importlib.util.spec_from_file_location("make_guard_rules_corpus", os.path.join(GOLDEN, "make_guard_rules_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["make_guard_rules_corpus"] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def corpus():
    return np.load(os.path.join(GOLDEN, "guard_rules_corpus.npz"))


_CASES = {}


def rules_case(corpus, name):
    """-> (setting's JSON entry, frame, bits, positions, stars, the model's stego) - the model runs once per setting"""
    if name not in _CASES:
        gen = _gen()
        m = META["settings"][name]
        c = gen.case(corpus, META, name)
        want = gen.model(c["frame"], m["delta"], m["n_ac"], c["bits"], m["rule"])
        for a in (c["frame"], c["bits"], want):
            a.setflags(write=False)
        _CASES[name] = (m, c["frame"], c["bits"], c["positions"], c["stars"], want)
    return _CASES[name]


def host(frame, m, bits, **kw):
    got, used, info = ml.host_embed(frame, m["delta"], m["n_ac"], bits, minmove=m["rule"] == "minmove",
                                    nearest=m["rule"] == "nearest", replay_map=True, **kw)
    assert used == bits.size
    return got[0], info


def differing_blocks(a, b):
    h, w = a.shape[-2:]
    d = (a.reshape(-1, h // 8, 8, w // 8, 8) != b.reshape(-1, h // 8, 8, w // 8, 8)).any(axis=(2, 4))
    return np.flatnonzero(d.reshape(-1))


def test_settings_are_the_table_and_the_files_are_small():
    s = META["settings"]
    assert len(NAMES) == 14
    for fam, (n, delta, qm) in TABLE.items():
        for rule in ("nearest", "minmove"):
            m = s[f"{fam}__{rule}"]
            assert (m["n_ac"], m["delta"], m["quantiser"], m["rule"]) == (n, delta, qm, rule)
    assert s["row1_one_block_per_lane__nearest"]["width"] // 8 % 2 == 1 and s["row1_two_blocks_per_lane__minmove"]["width"] % 16 == 0
    for name, src in (("row1_two_blocks_per_lane_d8__nearest", "row1_two_blocks_per_lane"), ("row2_n10_d8__nearest", "row2_n10")):
        assert (s[name]["n_ac"], s[name]["delta"]) == (REF_META["embed"][src]["n_ac"], REF_META["embed"][src]["delta"])
        assert s[name]["carried_over"] == CARRY_OVER[src]
    size = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("guard_rules_corpus.npz", "guard_rules_corpus.json"))
    assert size < os.path.getsize(os.path.join(GOLDEN, "guard_corpus.npz"))
    assert not META["quick"] and META["total_wall_time_s"] is not None
    for m in s.values():
        assert m["wall_time_s"] is not None and m["pools"] and m["boundary_blocks"] >= 1


@pytest.mark.parametrize("name", NAMES)
def test_scale_one_is_the_model_and_replays_the_listed_blocks(corpus, name):
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    got, info = host(frame, m, bits)
    assert np.array_equal(differing_blocks(got, want), []) and np.array_equal(got, want)
    assert info["path"] == 3 and (info["minmove"], info["nearest"]) == (m["rule"] == "minmove", m["rule"] == "nearest")
    assert np.array_equal(np.flatnonzero(info["replay_map"]), np.sort(positions)) and info["replayed"] == len(positions)
    exact, _ = host(frame, m, bits, pocketfft=True)
    assert np.array_equal(exact, want)
    # the layout: waves with 1, 8, 31, 32, 33, 64 (128) undecided blocks, then one per wave
    wave = m["wave"]
    per_wave = np.bincount(positions // wave, minlength=len(m["undecided_per_wave"])).tolist()
    lead = [1, 8, 31, 32, 33, 64] + ([128] if wave == 128 else [])
    assert per_wave == m["undecided_per_wave"] and per_wave[:len(lead)] == lead
    full_waves = frame.size // 64 // wave
    assert per_wave[len(lead):full_waves] == [1] * (full_waves - len(lead)) and full_waves >= len(lead) + 8
    assert m["undecided"] == len(positions) == sum(per_wave)


@pytest.mark.parametrize("name", NAMES)
def test_below_max_s_star_differs_exactly_in_the_predicted_blocks(corpus, name):
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    x = m["test_scale"]
    assert x is not None and 0.89 * m["max_s_star"] < x < m["max_s_star"] == float(stars.max())
    got, info = host(frame, m, bits, guard_scale=x)
    predicted = np.sort(positions[stars >= np.float32(x)])
    assert predicted.size >= 1
    assert np.array_equal(differing_blocks(got, want), predicted)
    assert info["replayed"] < len(positions)


@pytest.mark.parametrize("name", NAMES)
def test_stored_s_star_is_found_again(corpus, name):
    gen = _gen()
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    blocks = gen.frame_to_blocks(frame)
    per_block = bits.reshape(-1, m["n_ac"])
    starred = np.flatnonzero(stars > 0)
    assert len(starred) == m["boundary_blocks"]
    for i in sorted({int(np.argmax(stars)), *starred[::16].tolist(), int(np.flatnonzero(stars == 0)[0])}):
        p = positions[i]
        assert gen.rule_star(blocks[p], per_block[p], m["n_ac"], m["delta"], m["rule"]) == float(stars[i]), (name, i)


@pytest.mark.parametrize("name", sorted(CARRY_OVER))
def test_nearest_keeps_the_star_of_a_reference_block_with_the_same_change(name):
    """every block of the committed reference corpus whose change vector under SVS_NEAREST is its reference change: s* under
    SVS_NEAREST (the shim) is the stored star (hostemu, the reference rule) bit for bit"""
    gen = _gen()
    blocks, bits, stars, m = gen.reference_corpus_blocks(name)
    same = gen.nearest_change_is_reference_change(blocks, bits, m["n_ac"], m["delta"])
    assert int(same.sum()) == CARRY_OVER[name] >= 3
    for i in np.flatnonzero(same):
        got = gen.rule_star(blocks[i], bits[i], m["n_ac"], m["delta"], "nearest")
        assert np.float32(got) == stars[i] and got == float(stars[i]), (name, i, got, float(stars[i]))


@pytest.mark.parametrize("name", NAMES)
def test_filler_is_decided_at_scale_one_and_right_at_scale_zero(corpus, name):
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    got, info = host(frame, m, bits, guard_scale=0.0)
    assert np.isin(np.flatnonzero(info["replay_map"]), positions).all()      # a prediction ON an integer is undecided at any scale
    wrong = differing_blocks(got, want)
    assert np.isin(wrong, positions).all() and np.array_equal(wrong, np.sort(positions[stars > 0]))
    assert not bits.reshape(-1, m["n_ac"])[np.setdiff1d(np.arange(frame.size // 64), positions)].any()


@pytest.mark.parametrize("name", MINMOVE)
def test_minmove_settings_hold_coefficients_the_rule_leaves_alone(corpus, name):
    """at least a quarter of the undecided blocks hold a payload coefficient with a change of exactly 0"""
    m, frame, bits, positions, stars, want = rules_case(corpus, name)
    alone = _gen().left_alone(frame, bits, dict(delta=m["delta"], n_ac=m["n_ac"]))[positions]
    assert int(alone.sum()) == m["left_alone_blocks"] and 4 * m["left_alone_blocks"] >= len(positions)
    assert float(ml.band(m["delta"])[1:m["n_ac"] + 1].min()) > 0


@pytest.mark.parametrize("name", NAMES)
def test_max_s_star_reaches_half_the_reference_corpus(name):
    """the floor: half the committed max_s_star of the same kernel family in guard_corpus.json (the rules move a coefficient
    by at most delta where BETA's KD term assumes 1.5 delta: up to a third lower is expected, the rest is margin for the
    smaller search)"""
    m = META["settings"][name]
    assert m["floor"] == 0.5 * REF_META["embed"][m["floor_of"]]["max_s_star"]
    assert m["below_floor"] == (name in BELOW_FLOOR) == (m["max_s_star"] < m["floor"])
    if name in BELOW_FLOOR:
        pytest.xfail(BELOW_FLOOR[name])
    assert m["max_s_star"] >= m["floor"]


def test_generator_gives_the_same_bytes_whatever_the_worker_count(tmp_path):
    only = "row1_two_blocks_per_lane__minmove,row2_n10__nearest,row2_n10_d8__nearest"
    out = []
    for jobs in (1, 3):
        d = tmp_path / f"jobs{jobs}"
        subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_guard_rules_corpus.py"), "--quick", "--only", only,
                               "--jobs", str(jobs), "--out", str(d)], stdout=subprocess.DEVNULL)
        out.append([open(d / f, "rb").read() for f in ("guard_rules_corpus.npz", "guard_rules_corpus.json")])
    assert out[0] == out[1]
    assert sorted(json.loads(out[0][1])["settings"]) == sorted(only.split(","))
