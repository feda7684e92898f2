"""CPU tier: the kernel matrix (tests/kernel_matrix.py) is complete.  The kernel launch stubs of the product library, demangled,
are its inventory: every instantiation of the five dispatched families must be launched by at least one case of
KERNEL_CASES - as the library's own routing (csrc/svs_route.hpp via tests/hostemu) sends it - and every case must name only
instantiations the library has.  Every other kernel must be on HELPER_KERNELS with an existing test that launches it.
tests/test_kernel_matrix_gpu.py runs the cases against the oracle."""
import ast
import collections
import os

import pytest

import kernel_matrix as km
from testlib import REPO
from svsdct import native


@pytest.fixture(scope="module")
def inventory():
    if not os.path.exists(native.LIB_PATH):
        pytest.fail(f"{native.LIB_PATH} is missing: run `python __graft_entry__.py` first")
    return km.binary_inventory(native.LIB_PATH)


def dispatched(inventory):
    return {s for s in inventory if s.split("<")[0] in km.DISPATCHED_FAMILIES}


def test_inventory_reads_the_binary(inventory):
    """nm lists the stubs with their template arguments: each family has instantiations, the flags are spelled out"""
    families = collections.Counter(s.split("<")[0] for s in dispatched(inventory))
    assert set(families) == set(km.DISPATCHED_FAMILIES), families
    assert all("<" in s for s in dispatched(inventory))
    assert "embed_kernel<2, 1, 1, 0, true, svs::BlockOrderArgs>" in inventory
    assert "extract_bgr_kernel<8, 2, false>" in inventory


def test_cases_launch_exactly_the_dispatched_instantiations(inventory):
    want = dispatched(inventory)
    launched = collections.defaultdict(list)
    for case in km.KERNEL_CASES:
        syms = km.case_symbols(case)
        assert syms, f"{case.id} launches no kernel"
        for s in syms:
            launched[s].append(case.id)
    missing = sorted(want - set(launched))
    unknown = sorted(set(launched) - want)
    assert not missing, f"{len(missing)} of {len(want)} dispatched instantiations have no case: {missing}"
    assert not unknown, f"cases name instantiations the library does not have: {[(s, launched[s]) for s in unknown]}"
    print(f"{len(want)} dispatched instantiations, {len(km.KERNEL_CASES)} cases")


def test_every_other_kernel_has_a_test_that_launches_it(inventory):
    helpers = inventory - dispatched(inventory)
    assert helpers == set(km.HELPER_KERNELS), sorted(helpers ^ set(km.HELPER_KERNELS))
    for kernel, test_id in km.HELPER_KERNELS.items():
        path, name = test_id.split("::")
        tree = ast.parse(open(os.path.join(REPO, path)).read())
        assert name in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (kernel, test_id)


def test_case_ids_are_unique():
    ids = [c.id for c in km.KERNEL_CASES]
    assert len(ids) == len(set(ids)), [i for i, k in collections.Counter(ids).items() if k > 1]


def test_cases_cover_the_dimensions():
    """quantiser classes, both ends of every row range, n = 10, the clamped and empty routes, both block layouts, keyed
    cases, payloads that end inside a frame and (n > 1) inside a block, and FAST extraction only where the oracle applies"""
    gray = [c for c in km.KERNEL_CASES if c.entry == "gray"]
    ns = {c.n for c in gray}
    assert {1, 10, 0, 70} <= ns and any(n < 0 for n in ns)
    for r in range(2, 9):
        assert {8 * r - 8, 8 * r - 1} <= ns, r
    for entry in ("gray", "readback", "bgr"):
        qms = {km.plan_embed(c)["qm"] for c in km.KERNEL_CASES if c.entry == entry and km.plan_embed(c)["use"] > 0}
        assert qms == {km.QM_F32, km.QM_DOUBLE, km.QM_POW2}, entry
    paths = collections.Counter(km.plan_embed(c)["path"] for c in gray)
    assert set(paths) == {km.COPY, km.ROUND_TRIP, km.EXACT, km.STREAMING}
    assert {c.shape for c in km.KERNEL_CASES} == set(km.SHAPES)
    for name, (f, h, w) in km.SHAPES.items():
        per_lane = 2 if name == "even" else 1                                   # blocks per lane of embed_row1_kernel
        blocks = f * (h // 8) * (w // 8)
        assert blocks > per_lane * 256 and blocks % (64 * per_lane), name      # several workgroups, a partial last wave
    assert (km.SHAPES["even"][2] // 8) % 2 == 0 and (km.SHAPES["odd"][2] // 8) % 2 == 1
    assert km.BIT_OFFSET % 32
    for c in km.KERNEL_CASES:
        p = km.plan_embed(c)
        if c.entry != "bgr_extract" and p["use"] > 0:
            f = km.SHAPES[c.shape][0]
            n = km.clamp_n(c.n)
            assert km.capacity(c) * (f - 1) // f < p["use"] < km.capacity(c), c.id         # ends inside the last frame
            assert n == 1 or p["use"] % n, c.id                                              # and inside a block
        if c.entry in ("gray", "bgr_extract") and km.capacity(c) and km.plan_extract(c)["path"] == km.FAST:
            assert c.delta >= km.FAST_ORACLE_DELTA_MIN, c.id
