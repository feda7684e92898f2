"""The kernel matrix: one table of calls (KERNEL_CASES) that, between them, launch every kernel instantiation the product library
dispatches - the five families of csrc/svs_capi.hip (launch_embed, launch_readback, launch_embed_bgr, launch_extract,
launch_extract_bgr).  tests/test_kernel_matrix_gpu.py runs each case against the oracle; tests/test_kernel_matrix_cpu.py maps
each case to the symbols it launches (case_symbols) and checks that the map covers exactly the instantiations in the binary.

The route of a case (path, quantiser mode, rows, two blocks per lane) is the library's own: csrc/svs_route.hpp through
tests/hostemu.  case_symbols adds only what the launchers add on top of the plan: the KEYED, read-back and KEEP
instantiations, the n = 10 one and rows_allow_two_blocks."""
import ctypes
import re
import subprocess
from typing import NamedTuple

from testlib import hostemu

COPY, ROUND_TRIP, EXACT, STREAMING = range(4)         # svs::EmbedPath
ZEROS, X_EXACT, FAST = range(3)                       # svs::ExtractPath
QM_F32, QM_DOUBLE, QM_POW2 = range(3)                 # svs::QuantMode

# (frames, height, width).  even: 34 blocks per row, 16-byte pitches - embed_row1_kernel<QM, 2> - 612 blocks: three
# workgroups of one block per lane, two of two, the last wave partial either way.  odd: 25 blocks per row - <QM, 1> - 375 blocks.
SHAPES = {"even": (3, 48, 272), "odd": (3, 40, 200)}
BIT_OFFSET = 37                                       # not a multiple of 32
KEY, FIRST_FRAME = 0x0123456789ABCDEF, 5
FAST_ORACLE_DELTA_MIN = 0.25                          # FAST extraction is compared with the oracle from here up


class Case(NamedTuple):
    """entry: "gray" (svs_embed*_dev into a second buffer, then svs_extract* of its stego and of the cover, same mode and key),
    "readback" (svs_embed_readback_dev), "bgr" (svs_embed_bgr) or "bgr_extract" (svs_extract_bgr, no flags).
    payload: "bits" - bits [BIT_OFFSET, BIT_OFFSET + budget) of a stream, the budget ending inside the last frame and, for
    n > 1, inside a block (40 bits where nothing can be embedded); "empty" - no payload."""
    entry: str
    mode: str
    delta: float
    n: int
    shape: str = "odd"
    keyed: bool = False
    keep: bool = False
    payload: str = "bits"

    @property
    def id(self):
        return (f"{self.entry}-{self.mode}-d{self.delta:g}-n{self.n}-{self.shape}" + ("-keyed" if self.keyed else "") +
                ("-keep" if self.keep else "") + ("-empty" if self.payload == "empty" else ""))


def _cases():
    c = []
    alt = ("fast", "guarded")
    # streaming gray embed, one coefficient row (n = 1 and 7): embed_row1_kernel<QM, 1 | 2, KEYED>, 8 = QM_POW2, 20 = QM_F32,
    # 7.3 = QM_DOUBLE; extract_exact_kernel<1, QM, 1, KEYED>
    for i, delta in enumerate((8, 20, 7.3)):
        for j, shape in enumerate(("even", "odd")):
            for k, keyed in enumerate((False, True)):
                c.append(Case("gray", alt[(i + j + k) % 2], delta, (1, 7)[(j + k) % 2], shape, keyed))
    # streaming gray embed, two rows: embed_kernel<2, QM, 1, 0 | 10, KEYED>; FAST extract_kernel<2, QM, 1, 0 | 10, KEYED>
    for i, delta in enumerate((8, 20, 7.3)):
        c += [Case("gray", alt[i % 2], delta, 8, "even"), Case("gray", alt[(i + 1) % 2], delta, 15, "odd", True),
              Case("gray", alt[(i + 1) % 2], delta, 10, "odd"), Case("gray", alt[i % 2], delta, 10, "even", True)]
    # pocketfft mode, rows 1..8 (n = 8r - 8 | 8r - 1, and 1): embed_exact_kernel<QM, 1 | 2 | 8, KEYED>,
    # extract_exact_kernel<r, QM, 1, KEYED>; 4 = QM_POW2, 7.5 = QM_F32
    for r in range(1, 9):
        for i, delta in enumerate((4, 7.5)):
            for keyed in (False, True):
                n = (max(1, 8 * r - 8), 8 * r - 1)[(r + i + keyed) % 2]
                c.append(Case("gray", "exact", delta, n, ("even", "odd")[(r + i) % 2], keyed))
    # QM_DOUBLE steps outside the streaming kernels' range run the exact kernels in every mode: embed_exact_kernel<1, U, KEYED>
    # (5000.3: FAST extraction with n >= 8; 0.1: guarded - pocketfft-identical extraction below the guard's range)
    for keyed in (False, True):
        c += [Case("gray", "fast", 5000.3, 7, "even", keyed), Case("gray", "guarded", 0.1, 8, "odd", keyed),
              Case("gray", "fast", 5000.3, 63, "odd", keyed), Case("gray", "guarded", 0.1, 15, "even", keyed)]
    # FAST extraction with rows 3..8 (n >= 16: the embed is the exact kernel): extract_kernel<r, QM, 1, 0, KEYED>
    for r in range(3, 9):
        for i, delta in enumerate((8, 20)):
            for keyed in (False, True):
                n = (8 * r - 8, 8 * r - 1)[(r + i + keyed) % 2]
                c.append(Case("gray", alt[(r + keyed) % 2], delta, n, ("odd", "even")[(r + i) % 2], keyed))
    # routing edges: n > 63 clamps to 63; n = 0, n < 0 and delta <= 0 with a payload round-trip every block
    # (embed_exact_kernel<0, 8>; nothing or ZEROS to extract); an empty payload is a copy (embed_row1_kernel<0, 1 | 2>), keyed too
    c += [Case("gray", "guarded", 20, 70, "even"), Case("gray", "fast", 8, 70, "odd", True),
          Case("gray", "guarded", 8, 0, "odd"), Case("gray", "exact", 20, -3, "even"), Case("gray", "fast", 0.0, 10, "even"),
          Case("gray", "guarded", -1.0, 3, "odd", True),
          Case("gray", "fast", 8, 3, "even", payload="empty"), Case("gray", "guarded", 7.3, 10, "odd", True, payload="empty")]
    # read-back: readback_kernel<1 | 2 | 8, QM, KEYED> after the embed of each row class and quantiser mode
    for delta, n, mode in ((8, 3, "guarded"), (16, 10, "fast"), (8, 20, "guarded"),
                           (20, 7, "fast"), (7.5, 15, "exact"), (20, 63, "guarded"),
                           (7.3, 5, "guarded"), (0.1, 12, "fast"), (7.3, 40, "exact")):
        for keyed in (False, True):
            c.append(Case("readback", mode, delta, n, ("odd", "even")[keyed], keyed))
    # fused colour embed: embed_bgr_kernel<1 | 2, QM, false, KEEP> (streaming) and <8, QM, true, KEEP> (exact, round trip);
    # the copy of an empty payload runs <1, QM_POW2, false, KEEP>
    for i, delta in enumerate((8, 20, 7.3)):
        for keep in (False, True):
            c += [Case("bgr", alt[(i + keep) % 2], delta, (1, 7)[keep], ("even", "odd")[keep], keep=keep),
                  Case("bgr", alt[(i + keep + 1) % 2], delta, (10, 15)[keep], ("odd", "even")[keep], keep=keep),
                  Case("bgr", ("exact", "fast")[keep], delta, (3, 20)[keep], "odd", keep=keep)]
    for keep in (False, True):
        c += [Case("bgr", "fast", 8, 3, "even", keep=keep, payload="empty"), Case("bgr", "guarded", 0.0, 10, "odd", keep=keep)]
    # fused colour extraction: FAST extract_bgr_kernel<2..8, QM, true>; pocketfft-identical <1, QM, false> and, below 2^-10,
    # <2..8, QM, false> (2^-11 = QM_POW2; 0.0007 is no power of two: the QM_F32 instantiation)
    for r in range(2, 9):
        for i, delta in enumerate((8, 20)):
            c.append(Case("bgr_extract", "fast", delta, (8 * r - 8, 8 * r - 1)[(r + i) % 2], ("even", "odd")[(r + i) % 2]))
        for i, delta in enumerate((2.0 ** -11, 0.0007)):
            c.append(Case("bgr_extract", "fast", delta, (8 * r - 1, 8 * r - 8)[(r + i) % 2], ("odd", "even")[(r + i) % 2]))
    c += [Case("bgr_extract", "fast", 8, 1, "even"), Case("bgr_extract", "fast", 7.3, 7, "odd")]
    return c


KERNEL_CASES = _cases()

# Kernels outside the five dispatched families, each with an existing test that launches it
HELPER_KERNELS = {
    "ascii_to_packed_kernel": "tests/test_gpu_parity.py::test_string_payload_entry_points_equal_the_packed_ones",
    "packed_to_ascii_kernel": "tests/test_gpu_parity.py::test_string_payload_entry_points_equal_the_packed_ones",
    "fill_synthetic_kernel": "tests/test_helper_kernels_gpu.py::test_fill_synthetic_frames_counters_and_padding",
    "fill_bits_kernel": "tests/test_helper_kernels_gpu.py::test_fill_bits_counters_past_2_to_the_32",
    "frame_sse_kernel": "tests/test_helper_kernels_gpu.py::test_frame_sse_many_frames_and_pitched",
    "bit_errors_kernel": "tests/test_helper_kernels_gpu.py::test_bit_errors_lengths_and_tail_masks",
    "frame_minmax_kernel": "tests/test_helper_kernels_gpu.py::test_ssim_and_data_range_at_tile_band_and_row_group_edges",
    "frame_range_finish_kernel": "tests/test_helper_kernels_gpu.py::test_ssim_and_data_range_at_tile_band_and_row_group_edges",
    "ssim_partial_kernel": "tests/test_helper_kernels_gpu.py::test_ssim_and_data_range_at_tile_band_and_row_group_edges",
    "ssim_finish_kernel": "tests/test_helper_kernels_gpu.py::test_ssim_and_data_range_at_tile_band_and_row_group_edges",
    "bgr_to_gray_kernel": "tests/test_helper_kernels_gpu.py::test_colour_conversions_pitched_with_sentinels",
    "gray_to_bgr_kernel": "tests/test_helper_kernels_gpu.py::test_colour_conversions_pitched_with_sentinels",
}
DISPATCHED_FAMILIES = ("embed_row1_kernel", "embed_kernel", "embed_exact_kernel", "readback_kernel", "embed_bgr_kernel",
                       "extract_kernel", "extract_exact_kernel", "extract_bgr_kernel")

_KERNEL_NAME = re.compile(r"svs::(?:__device_stub__)?(\w+_kernel)(<[^()]*>)?")


def kernel_name(text):
    """'family<args>' (or 'name' for a plain kernel) of a demangled symbol or trace name, None if it names no svs kernel"""
    m = _KERNEL_NAME.search(text)
    return m.group(1) + (m.group(2) or "") if m else None


def binary_inventory(lib_path):
    """the kernel launch stubs of a library, demangled (`nm -C`) -> set of 'family<args>' / 'name'"""
    out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    return {kernel_name(line) for line in out.splitlines() if "__device_stub__" in line}


# ---- the route of a case ----------------------------------------------------------------------------------------------
def clamp_n(n):
    return min(max(int(n), 0), 63)


def capacity(case):
    f, h, w = SHAPES[case.shape]
    return f * (h // 8) * (w // 8) * clamp_n(case.n)


def budget(case):
    """payload bits the call offers"""
    if case.payload == "empty":
        return 0
    cap = capacity(case)
    if cap == 0 or not case.delta > 0:
        return 40
    f = SHAPES[case.shape][0]
    nb = cap - (cap // f) // 3 - 1                    # inside the last frame
    return nb - 1 if clamp_n(case.n) > 1 and nb % clamp_n(case.n) == 0 else nb


def _flags(mode):
    return int(mode == "exact"), int(mode == "guarded")        # SVS_EXACT_POCKETFFT, SVS_EXACT_GUARDED


def plan_embed(case):
    f, h, w = SHAPES[case.shape]
    out = (ctypes.c_int64 * 10)()
    bgr = case.entry == "bgr"
    hostemu().emu_plan_embed(ctypes.c_double(case.delta), int(case.n), ctypes.c_uint64(f * (h // 8) * (w // 8)),
                             ctypes.c_uint64(budget(case)), ctypes.c_uint64(BIT_OFFSET), *_flags(case.mode), int(bgr), 0, out)
    return dict(zip(("path", "rows", "qm", "xcd_chunk", "n_ac", "two_blocks", "use", "bit_offset", "n_bits", "n_words"), out))


def plan_extract(case):
    f, h, w = SHAPES[case.shape]
    out = (ctypes.c_int64 * 4)()
    bgr = case.entry == "bgr_extract"
    pocketfft, guarded = (0, 0) if bgr else _flags(case.mode)
    hostemu().emu_plan_extract(ctypes.c_double(case.delta), int(case.n), ctypes.c_uint64(f * (h // 8) * (w // 8)), pocketfft,
                               guarded, int(bgr), 0, out)
    return dict(zip(("path", "rows", "qm", "xcd_chunk"), out))


def rows_allow_two_blocks(case):
    """csrc/svs_capi.hip's rule for contiguous planes in separate device allocations (256-byte aligned)"""
    f, h, w = SHAPES[case.shape]
    return (w // 8) % 2 == 0 and w % 16 == 0 and (h * w) % 16 == 0


def _b(v):
    return "true" if v else "false"


def _keyed(keyed):
    return "true, svs::BlockOrderArgs" if keyed else "false"


def case_symbols(case):
    """the kernel instantiations one case launches, as 'family<template args>' (the demangled names of the binary)"""
    syms = []
    if case.entry in ("gray", "readback"):
        p = plan_embed(case)
        keyed = case.keyed and p["path"] in (EXACT, STREAMING)
        qm, rows = p["qm"], p["rows"]
        if p["path"] in (EXACT, ROUND_TRIP):
            syms.append(f"embed_exact_kernel<{qm}, {rows}, {_keyed(keyed)}>")
        elif rows == 2:
            syms.append(f"embed_kernel<2, {qm}, 1, 0, true, svs::BlockOrderArgs>" if keyed else
                        f"embed_kernel<2, {qm}, 1, {10 if p['n_ac'] == 10 else 0}, false>")
        else:
            bpl = 2 if p["two_blocks"] and rows_allow_two_blocks(case) else 1
            syms.append(f"embed_row1_kernel<{qm}, {bpl}, {_keyed(keyed)}>")
        if case.entry == "readback" and p["use"] > 0:
            syms.append(f"readback_kernel<{rows}, {qm}, {_keyed(keyed)}>")
    if case.entry == "bgr":
        p = plan_embed(case)
        exact = p["path"] in (EXACT, ROUND_TRIP)
        syms.append(f"embed_bgr_kernel<{8 if exact else p['rows']}, {p['qm']}, {_b(exact)}, {_b(case.keep)}>")
    if case.entry in ("gray", "bgr_extract") and capacity(case) > 0:
        p = plan_extract(case)
        qm, rows = p["qm"], p["rows"]
        if case.entry == "bgr_extract":
            if p["path"] != ZEROS:
                syms.append(f"extract_bgr_kernel<{rows}, {qm}, {_b(p['path'] == FAST)}>")
        elif p["path"] == X_EXACT:
            syms.append(f"extract_exact_kernel<{rows}, {qm}, 1, {_keyed(case.keyed)}>")
        elif p["path"] == FAST:
            if case.keyed:
                syms.append(f"extract_kernel<{rows}, {qm}, 1, 0, true, svs::BlockOrderArgs>")
            else:
                syms.append(f"extract_kernel<{rows}, {qm}, 1, {10 if clamp_n(case.n) == 10 else 0}, false>")
    return syms
