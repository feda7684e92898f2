"""CPU tier: tools/ratelib.py, the harness of the feature rate scripts - the order in which `alternate` times its sides, the one
verdict rule, the loader of another build of the library, and the options and defaults of each of the ten scripts.  No GPU and
no torch: the timer is injected, and nothing here makes a session."""
import ctypes as C
import importlib
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import ratelib  # noqa: E402
from svsdct import native  # noqa: E402


def run_alternate(n_sides, reps, rotate=True):
    """(the sides in the order they were called, the result) with a timer that returns a running counter"""
    called = []

    def timer(fn):
        fn()
        return float(len(called))

    todo = {f"side {i}": (lambda i=i: called.append(i)) for i in range(n_sides)}
    return called, ratelib.alternate(todo, reps, rotate, timed=timer)


def test_alternate_rotates_the_starting_side():
    called, t = run_alternate(3, 4)
    assert [called.count(i) for i in range(3)] == [5, 5, 5]
    assert called[:3] == [0, 1, 2]                                  # the warm-ups come first, in the given order
    for r in range(4):
        assert called[3 + 3 * r:6 + 3 * r] == [(r + k) % 3 for k in range(3)]      # repetition r starts at side r % 3
    assert list(t) == ["side 0", "side 1", "side 2"] and all(len(v) == 4 for v in t.values())
    # the warm-ups are not among the times: side 0's are the counter after calls 4, 9 (behind sides 1, 2), 11 and 13
    assert t["side 0"] == [4.0, 9.0, 11.0, 13.0]


def test_alternate_fixed_order():
    called, t = run_alternate(3, 4, rotate=False)
    assert called == [0, 1, 2] * 5
    assert t["side 2"] == [6.0, 9.0, 12.0, 15.0]


def test_alternate_one_side_and_no_repetitions():
    called, t = run_alternate(1, 4)
    assert called == [0] * 5 and t == {"side 0": [2.0, 3.0, 4.0, 5.0]}
    called, t = run_alternate(3, 0)
    assert called == [0, 1, 2] and t == {"side 0": [], "side 1": [], "side 2": []}     # the warm-ups are still made


@pytest.mark.parametrize("this, inside, word", [
    ([1.0, 1.0, 1.0], True, "inside"),                 # the median on the baseline's min: the edges are inclusive
    ([3.0, 3.0, 3.0], True, "inside"),                 # and on its max
    ([0.5, 2.0, 9.0], True, "inside"),                 # the median counts, not the extremes
    ([3.0, 3.5, 3.5], False, "ABOVE (slower than)"),
    ([0.5, 0.5, 2.0], False, "BELOW (faster than)"),   # a faster build is not "inside"
])
def test_verdict(this, inside, word):
    assert ratelib.verdict([1.0, 2.0, 3.0], this) == (inside, f"    this build's median is {word} the baseline's spread")


def test_verdict_baseline_of_one_sample():
    assert ratelib.verdict([2.0], [2.0])[0]
    assert ratelib.verdict([2.0], [2.0, 2.001, 2.001]) == (False, "    this build's median is ABOVE (slower than) the baseline's spread")
    assert ratelib.verdict([2.0], [1.999])[1] == "    this build's median is BELOW (faster than) the baseline's spread"


def test_load_build_attaches_the_prototypes_a_library_has():
    lib = ratelib.load_build(native.LIB_PATH)
    for name in ("svs_embed_dev", "svs_soft_histogram_dev"):
        res, args = native.SIGNATURES[name]
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # a library with none of the symbols: nothing is attached and nothing raises
    emu = ratelib.load_build(os.path.join(REPO, "tests", "hostemu", "libsvs_hostemu.so"))
    assert not any(hasattr(emu, name) for name in native.SIGNATURES)
    assert isinstance(emu, C.CDLL)


# script -> (frames, reps, has --rounds, other defaults), as they were before the scripts shared a parser
DEFAULTS = {
    "readback_rates": (600, 10, True, {"configs": "8:3,20:10"}),
    "colour_readback_rates": (200, 7, True, {"configs": "8:3,20:10,7.5:20", "baseline_lib": None}),
    "keyed_readback_rates": (200, 7, True, {"delta": 20.0, "n_ac": 10, "baseline_lib": None}),
    "nearest_rates": (200, 5, False, {"configs": "8:3,8:10,20:10,8:20", "bgr_frames": 48, "bgr_configs": "20:10,8:3",
                                      "baseline_lib": None}),
    "minmove_rates": (200, 5, False, {"configs": "20:3,20:10,20:20", "bgr_frames": 48, "bgr_configs": "20:10",
                                      "baseline_lib": None}),
    "coeff_select_rates": (200, 5, False, {}),
    "dither_rates": (200, 5, False, {"baseline_lib": None}),
    "soft_extract_rates": (200, 5, False, {"baseline_lib": None}),
    "soft_vote_rates": (200, 5, False, {"baseline_lib": None}),
    "soft_histogram_rates": (200, 15, False, {"baseline_lib": None, "variant_lib": []}),
}


class Parsed(Exception):
    """carries the parsed options out of a script's main() before it touches a device"""


def stop_at_the_session(args):
    raise Parsed(args)


@pytest.mark.parametrize("script", sorted(DEFAULTS))
def test_script_options_and_defaults(script, monkeypatch):
    frames, reps, rounds, other = DEFAULTS[script]
    monkeypatch.setattr(ratelib, "Session", stop_at_the_session)
    main = importlib.import_module(script).main

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", [script + ".py", *argv])
        with pytest.raises(Parsed) as stopped:
            main()
        return stopped.value.args[0]

    required = ["--baseline-lib", "x.so"] if script == "coeff_select_rates" else []
    args = parse(*required)
    assert (args.frames, args.h, args.w, args.reps, args.fixed_order) == (frames, 2160, 3840, reps, False)
    assert args.out == os.path.join(REPO, "profiles", script + ".txt")
    for name, value in other.items():
        assert getattr(args, name) == value, name
    assert parse(*required, "--reps", "3", "--fixed-order", "--out", "o.txt").reps == 3
    if rounds:
        assert parse(*required, "--rounds", "3").reps == 3
    else:
        with pytest.raises(SystemExit):
            parse(*required, "--rounds", "3")
    if script == "coeff_select_rates":
        with pytest.raises(SystemExit):                 # its baseline is required
            parse()
