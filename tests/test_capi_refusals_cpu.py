"""The refusals of every svs_embed* / svs_extract* / svs_soft_* entry point, pinned against the build that wrote
tests/golden/capi_refusals.json (tests/golden/make_capi_refusals.py: the parent of the refactor to one options value per gray
call; the svs_soft_* symbols from the parent of the refactor to one description of a soft call's output): return code, the full svs_last_error() text and what the call left in its out parameters, for every argument a symbol
checks before its device work, alone and in pairs (precedence), and for the empty call.  No case reaches the device: the
library answers all of them without a GPU."""
import json
import os

import pytest

from capi_refusals_lib import cases_of, run_case
from svsdct import native
from testlib import REPO


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(REPO, "tests", "golden", "capi_refusals.json")) as f:
        return json.load(f)


def gray_and_colour_symbols():
    return sorted(s for s in native.SIGNATURES if s.startswith(("svs_embed", "svs_extract", "svs_soft")))


def test_every_embed_and_extract_symbol_is_in_the_table(table):
    assert sorted(table["symbols"]) == gray_and_colour_symbols() and len(table["symbols"]) == 34
    for sym, entry in table["symbols"].items():
        assert len(entry["parameters"]) == len(native.SIGNATURES[sym][1]), sym
        assert len(entry["pairs"]) >= 20, sym                                        # pairs: precedence
        assert any(c[1] == native.SVS_OK for c in entry["cases"]), sym               # the accepted empty call


def test_no_case_of_the_table_reaches_the_device(table):
    for sym in table["symbols"]:
        for name, args, rc, _, _ in cases_of(table, sym):
            assert rc in (native.SVS_OK, native.SVS_ERR_INVALID_ARG, native.SVS_ERR_CAPACITY), (sym, name)
            if rc == native.SVS_OK:
                planes = next(a["planes"] for a in args if isinstance(a, dict) and "planes" in a)
                assert planes[0] == 0, (sym, name)


def test_the_library_refuses_as_the_table_says(table):
    lib = native.load()
    wrong, n = [], 0
    for sym in table["symbols"]:
        for name, args, rc, message, outs in cases_of(table, sym):
            got = run_case(lib, sym, args)
            n += 1
            if got != (rc, message, outs):
                wrong.append((sym, name, got, (rc, message, outs)))
    assert n > 3000 and not wrong, f"{len(wrong)} of {n} cases differ; the first: {wrong[:3]}"
