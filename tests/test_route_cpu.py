"""CPU tier: the routing of the C ABI (csrc/svs_route.hpp, compiled into tests/hostemu) - which kernel family an embed or
extract call runs, with which quantiser mode, coefficient rows, tile map and payload arguments.  The library and hostemu both
take their routing from that header; this pins its decision table across deltas, coefficient counts, payloads, flags, gray
and BGR, and the experiments library's SVS_GUARDED_OFF.  The GPU tier checks the kernels' results on the same paths."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from testlib import hostemu

COPY, ROUND_TRIP, EXACT, STREAMING = range(4)         # svs::EmbedPath
ZEROS, X_EXACT, FAST = range(3)                       # svs::ExtractPath
QM_F32, QM_DOUBLE, QM_POW2 = range(3)                 # svs::QuantMode
EIGHTH = 0xFFFFFFFF

NS = (0, 1, 7, 8, 10, 15, 16, 63)
DELTAS = (-1.0, 0.0, 2.0 ** -11, 0.2, 0.25, 8.0, 4096.0, 5000.0)
FLAGS = ((False, False), (True, False), (False, True), (True, True))   # (SVS_EXACT_POCKETFFT, SVS_EXACT_GUARDED)
TOTAL = 12                                            # blocks of the batch
PAYLOADS = (0, 5, 10 ** 9)                            # empty, a few bits, more than the capacity


def plan_embed(delta, n, n_bits, bit_offset, pocketfft, guarded, bgr, off):
    out = (ctypes.c_int64 * 10)()
    hostemu().emu_plan_embed(ctypes.c_double(delta), n, ctypes.c_uint64(TOTAL), ctypes.c_uint64(n_bits),
                             ctypes.c_uint64(bit_offset), int(pocketfft), int(guarded), int(bgr), int(off), out)
    return dict(zip(("path", "rows", "qm", "xcd_chunk", "n_ac", "two_blocks", "use", "bit_offset", "n_bits", "n_words"), out))


def plan_extract(delta, n, pocketfft, guarded, bgr, off):
    out = (ctypes.c_int64 * 4)()
    hostemu().emu_plan_extract(ctypes.c_double(delta), n, ctypes.c_uint64(TOTAL), int(pocketfft), int(guarded), int(bgr), int(off),
                               out)
    return dict(zip(("path", "rows", "qm", "xcd_chunk"), out))


def qm_of(delta):
    """svs::make_qim's quantiser mode"""
    if float(np.float32(delta)) != delta:
        return QM_DOUBLE
    m, e = math.frexp(delta)
    return QM_POW2 if m == 0.5 and -100 < e < 100 else QM_F32


def expected_embed(delta, n, n_bits, bit_offset, pocketfft, guarded, bgr, off):
    """the decision table of svs_embed_dev / svs_embed_bgr_dev as the parent of svs_route.hpp wrote them out"""
    use = min(n_bits, TOTAL * n) if delta > 0 and n > 0 else 0
    rows = n // 8 + 1
    streaming = use > 0 and 0.25 <= delta <= 4096 and not pocketfft and rows <= 2 and not (off and not bgr)
    if use > 0:
        words = ((bit_offset + use + 7) // 8 + 3) // 4
        if streaming:   # embed_row1_kernel / embed_kernel<2>; BGR: embed_bgr_kernel<rows, QM, false>
            return dict(path=STREAMING, rows=rows, qm=qm_of(delta), n_ac=n, two_blocks=int(not bgr and rows == 1), use=use,
                        bit_offset=bit_offset, n_bits=use, n_words=words)
        # embed_exact_kernel<QM, 1 | 2 | 8>; BGR: embed_bgr_kernel<8, QM, true>
        return dict(path=EXACT, rows=rows if rows <= 2 and not bgr else 8, qm=qm_of(delta), n_ac=n, two_blocks=0, use=use,
                    bit_offset=bit_offset, n_bits=use, n_words=words)
    # nothing to embed: gray - the QM_F32 instantiations, bit offset 0; BGR - make_qim(1.0)'s (QM_POW2), the call's bit offset
    qm = QM_POW2 if bgr else QM_F32
    if n_bits == 0:     # embed_row1_kernel<QM_F32, 1 | 2> copy; BGR: embed_bgr_kernel<1, QM_POW2, false> convert
        return dict(path=COPY, rows=1, qm=qm, n_ac=1, two_blocks=int(not bgr and rows == 1), use=0,
                    bit_offset=bit_offset if bgr else 0, n_bits=0, n_words=0)
    # embed_exact_kernel<QM_F32, 8>; BGR: embed_bgr_kernel<8, QM_POW2, true> - every block round-tripped, one pass bit
    return dict(path=ROUND_TRIP, rows=8, qm=qm, n_ac=0, two_blocks=0, use=0, bit_offset=bit_offset if bgr else 0, n_bits=1,
                n_words=0)


def expected_extract(delta, n, pocketfft, guarded, bgr, off):
    """the decision table of svs_extract_dev / svs_extract_bgr_dev as the parent of svs_route.hpp wrote them out"""
    if not delta > 0:
        return dict(path=ZEROS)
    rows = n // 8 + 1
    qm = QM_POW2 if qm_of(delta) == QM_POW2 else QM_F32
    chunk = 32 if rows == 1 else (0 if rows == 2 and not bgr else EIGHTH)
    if bgr:             # no flags
        exact = False
    elif guarded:       # GUARDED: FAST inside the guard's delta range (unless SVS_GUARDED_OFF), pocketfft-identical outside
        exact = not (0.25 <= delta <= 4096 and not off)
    else:
        exact = pocketfft
    exact = exact or rows == 1 or float(np.float32(delta)) < 2.0 ** -10
    return dict(path=X_EXACT if exact else FAST, rows=rows, qm=qm, xcd_chunk=chunk)


@pytest.mark.parametrize("bgr", (False, True), ids=("gray", "bgr"))
def test_embed_routing(bgr):
    import bench
    for n, delta, n_bits, bit_offset, (pocketfft, guarded), off in itertools.product(NS, DELTAS, PAYLOADS, (0, 37), FLAGS,
                                                                                      (False, True)):
        case = (n, delta, n_bits, bit_offset, pocketfft, guarded, bgr, off)
        got = plan_embed(delta, n, n_bits, bit_offset, pocketfft, guarded, bgr, off)
        want = expected_embed(delta, n, n_bits, bit_offset, pocketfft, guarded, bgr, off)
        assert got["xcd_chunk"] == EIGHTH, case
        assert {k: got[k] for k in want} == want, case
        # bench.py's roofline label names the kernel svs_embed_dev launches for a payload that can be embedded
        if not bgr and not off and want["use"] > 0 and not (pocketfft and guarded):
            label = bench.embed_kernel_label("exact" if pocketfft else ("guarded" if guarded else "fast"), n, delta)
            prefix = {EXACT: "embed_exact_kernel", STREAMING: "embed_row1_kernel" if got["rows"] == 1 else "embed_kernel<2>"}
            assert label.startswith(prefix[got["path"]]), (case, label)


@pytest.mark.parametrize("bgr", (False, True), ids=("gray", "bgr"))
def test_extract_routing(bgr):
    # n = 0 is never planned: a call without coefficients returns before it (no bits to extract)
    for n, delta, (pocketfft, guarded), off in itertools.product(NS[1:], DELTAS, FLAGS, (False, True)):
        if bgr and (pocketfft or guarded):
            continue    # the BGR extract call has no flags
        case = (n, delta, pocketfft, guarded, bgr, off)
        got = plan_extract(delta, n, pocketfft, guarded, bgr, off)
        want = expected_extract(delta, n, pocketfft, guarded, bgr, off)
        assert {k: got[k] for k in want} == want, case


def test_paths_the_kernels_serve():
    """spot checks: the benchmark's n = 3 at delta 8 streams through the one-row kernel, two blocks per lane allowed; the GUI's
    n = 10 through the two-row kernel; SVS_GUARDED_OFF sends the gray call, and only the gray call, to the exact kernel"""
    assert plan_embed(8.0, 3, 100, 0, False, True, False, False)["path"] == STREAMING
    assert plan_embed(8.0, 3, 100, 0, False, True, False, False)["two_blocks"] == 1
    assert plan_embed(8.0, 10, 100, 0, False, False, False, False)["rows"] == 2
    assert plan_embed(8.0, 3, 100, 0, False, True, False, True)["path"] == EXACT
    assert plan_embed(8.0, 3, 100, 0, False, True, True, True)["path"] == STREAMING
    assert plan_extract(8.0, 10, False, True, False, False)["path"] == FAST
    assert plan_extract(8.0, 10, False, True, False, True)["path"] == X_EXACT
    assert plan_extract(8.0, 10, False, False, True, True)["path"] == FAST
