"""CPU tier of the one plan of a coded stream (svsdct/batch.py, _CodedPlan): its lengths against fec.coded_bits, rs.coded_bytes
and soft.tile, its workspace layout against coded_workspace_bytes, and the one capacity refusal - at every rate code, with and
without the outer code, for one copy, three and as many as fit, at the smallest payloads that cross a codeword (223 data bytes)
or a puncturing period and a byte (58, 59 bits).  Nothing here needs a GPU."""
import numpy as np
import pytest

from svsdct import batch, fec, rs, soft

SMALL = batch.capacity_bits(2, 16, 16, 10)         # 80 bits
LARGE = batch.capacity_bits(12, 96, 160, 10)       # for the payloads whose coded stream does not fit in 80
RATES = (2, 3, 23, 34, 56, 78)
PAYLOADS = {True: (8, 223 * 8, 224 * 8), False: (1, 58, 59)}


def _ceil8(bits):
    return (bits + 7) // 8


@pytest.mark.parametrize("outer", (False, True))
@pytest.mark.parametrize("rate", RATES)
def test_the_plan_holds_the_lengths_and_the_layout(rate, outer):
    assert (SMALL, LARGE) == (80, 28800)
    for n_info in PAYLOADS[outer]:
        k = n_info // 8 if outer else 0
        inner = 8 * rs.coded_bytes(k) if outer else n_info
        coded = fec.coded_bits(inner, rate)
        cap = SMALL if coded <= SMALL else LARGE
        for copies in (1, 3, None):
            plan = batch._CodedPlan.of(n_info, rate, copies, outer, cap)
            assert plan.work_bytes == batch.coded_workspace_bytes(n_info, rate, copies, outer, cap)
            assert (plan.capacity, plan.k, plan.inner, plan.coded) == (cap, k, inner, coded)
            assert plan.stream == soft.tile(np.zeros(coded, np.uint8), cap if copies is None else min(cap, copies * coded)).size
            # the stages in workspace order: the Reed-Solomon stream, the coded stream, the tiled stream
            stages = [(0, rs.coded_bytes(k))] * outer + [(plan.at_coded, _ceil8(coded))] + [(plan.at_stream, _ceil8(plan.stream))] * (copies != 1)
            if copies == 1:
                assert plan.at_stream == plan.at_coded                  # the coded stream is what is embedded
            end = 0
            for at, nbytes in stages:
                assert at % 4 == 0 and at >= end and nbytes > 0, (n_info, copies, stages)
                end = at + nbytes
            assert end <= plan.work_bytes < end + 4


@pytest.mark.parametrize("outer", (False, True))
@pytest.mark.parametrize("rate", RATES)
def test_one_step_above_the_capacity_is_refused_with_the_one_message(rate, outer):
    for cap in (SMALL, LARGE):
        most = rs.payload_bits(cap, rate) if outer else fec.info_bits(cap, rate)
        if most:
            assert batch._CodedPlan.of(most, rate, 1, outer, cap).coded <= cap
        n_info = most + (8 if outer else 1)
        coded = fec.coded_bits(8 * rs.coded_bytes(n_info // 8) if outer else n_info, rate)
        message = f"^{coded} coded bits exceed the capacity of {cap}: at rate code {rate} it holds {most} payload bits$"
        for copies in (1, 3, None):
            with pytest.raises(ValueError, match=message):
                batch._CodedPlan.of(n_info, rate, copies, outer, cap)
            with pytest.raises(ValueError, match=message):
                batch.coded_workspace_bytes(n_info, rate, copies, outer, cap)
    frames = np.zeros((2, 16, 16), np.uint8)
    n_info = (rs.payload_bits(SMALL, rate) + 8) if outer else fec.info_bits(SMALL, rate) + 1
    for call in (lambda: batch.embed_coded_frames(frames, 20, 10, np.zeros(n_info, np.uint8), rate=rate, outer=outer),
                 lambda: batch.extract_coded_frames(frames, 20, 10, n_info, rate=rate, outer=outer)):
        with pytest.raises(ValueError, match=f"exceed the capacity of {SMALL}"):
            call()


def test_the_host_path_refuses_before_it_encodes(monkeypatch):
    def encode(*args):
        raise AssertionError("the payload was encoded before the plan refused it")
    monkeypatch.setattr(fec, "encode", encode)
    monkeypatch.setattr(rs, "encode_array", encode)
    for outer, n_info in ((False, fec.info_bits(SMALL, 2) + 1), (True, 8)):
        with pytest.raises(ValueError, match="exceed the capacity"):
            batch.embed_coded_frames(np.zeros((2, 16, 16), np.uint8), 20, 10, np.zeros(n_info, np.uint8), rate=2, outer=outer)
