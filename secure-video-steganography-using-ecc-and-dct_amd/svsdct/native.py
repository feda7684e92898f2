"""ctypes binding of libsvsdct.so - the C ABI declared in include/svsdct.h.

There is deliberately no fallback: if the shared library has not been built (or cannot be
loaded) importing the symbols raises `SvsNativeError` with the build command.  The product path
never computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SVSDCT_LIB", os.path.join(_PKG_DIR, "lib", "libsvsdct.so"))

SVS_OK = 0
SVS_ERR_INVALID_ARG = -1
SVS_ERR_HIP = -2
SVS_ERR_NO_DEVICE = -3
SVS_ERR_CAPACITY = -4
SVS_EXACT_POCKETFFT = 1      # flags bit: pocketfft-identical arithmetic (include/svsdct.h)
SVS_EXACT_GUARDED = 2        # flags bit: the same bit-identical result through the guarded kernel where it applies
SVS_KEEP_COLOUR = 0x100      # flags bit, fused colour embed only: stego pixels keep the cover's colour (include/svsdct.h)
SVS_READBACK = 0x200         # flags bit, gray embed only: read every payload block back, repair the ones that fail (include/svsdct.h)
SVS_NEAREST = 0x800          # flags bit, every embed call: a wrong parity moves to the nearer lattice point (include/svsdct.h)
SVS_MINMOVE = 0x1000         # flags bit, every embed call: a coefficient moves only as far as its decision cell asks (include/svsdct.h)
ABI_VERSION = 4


class SvsNativeError(RuntimeError):
    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class Planes(C.Structure):
    """struct svs_planes"""
    _fields_ = [("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("reserved", C.c_int32), ("row_pitch", C.c_int64), ("frame_pitch", C.c_int64)]

    @classmethod
    def contiguous(cls, n_frames: int, height: int, width: int) -> "Planes":
        return cls(n_frames, height, width, 0, width, height * width)


class ReadbackCounts(C.Structure):
    """struct svs_readback_counts: blocks repaired / left unrepaired by an SVS_READBACK call"""
    _fields_ = [("repaired", C.c_uint64), ("unrepaired", C.c_uint64)]


class MarginCounts(C.Structure):
    """struct svs_margin_counts: the read-back's two counts and the margin pass's (svs_stepped_embed_readback_margin*)"""
    _fields_ = [("repaired", C.c_uint64), ("unrepaired", C.c_uint64), ("strengthened", C.c_uint64), ("weak", C.c_uint64)]


class BlockOrder(C.Structure):
    """struct svs_block_order: the keyed block order of the ordered entry points (include/svsdct.h, svsdct/order.py)"""
    _fields_ = [("key", C.c_uint64), ("first_frame", C.c_uint32), ("reserved", C.c_uint32)]


class Coeffs(C.Structure):
    """struct svs_coeffs: the payload coefficient selection of the select entry points (include/svsdct.h, svsdct/coeffs.py)"""
    _fields_ = [("count", C.c_uint8), ("index", C.c_uint8 * 63)]


class Dither(C.Structure):
    """struct svs_dither: the keyed dither of the dithered entry points (include/svsdct.h, svsdct/dither.py)"""
    _fields_ = [("key", C.c_uint64), ("first_frame", C.c_uint32), ("reserved", C.c_uint32)]


class Steps(C.Structure):
    """struct svs_steps: the 64 quantiser steps of the requantisation channel (include/svsdct.h, svsdct/channel.py)"""
    _fields_ = [("step", C.c_uint16 * 64)]


class QimSteps(C.Structure):
    """struct svs_qim_steps: the per-coefficient QIM steps of the stepped entry points (include/svsdct.h, svsdct/steps.py)"""
    _fields_ = [("delta", C.c_uint16 * 64)]


class Matrix(C.Structure):
    """struct svs_matrix: k bits a block and the flip search of the matrix entry points (include/svsdct.h, svsdct/matrix.py)"""
    _fields_ = [("k", C.c_uint32), ("search", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SVS_SCAN_ROW_MAJOR = 0
SVS_SCAN_ZIGZAG = 1

_u8p = C.c_void_p   # device or host byte pointers are passed as integers / c_void_p
_u64p = C.POINTER(C.c_uint64)
_PL = C.POINTER(Planes)
_BO = C.POINTER(BlockOrder)
_CO = C.POINTER(Coeffs)
_DI = C.POINTER(Dither)
_ST = C.POINTER(Steps)
_QS = C.POINTER(QimSteps)
_MX = C.POINTER(Matrix)

# name -> (restype, argtypes); every symbol include/svsdct.h declares
SIGNATURES = {
    "svs_abi_version": (C.c_int, []),
    "svs_last_error": (C.c_char_p, []),
    "svs_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "svs_init": (C.c_int, [C.c_int]),
    "svs_device_arch": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "svs_shutdown": (C.c_int, []),
    "svs_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "svs_free": (C.c_int, [C.c_void_p]),
    "svs_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "svs_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "svs_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "svs_stream_synchronize": (C.c_int, [C.c_void_p]),
    "svs_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "svs_stream_destroy": (C.c_int, [C.c_void_p]),
    "svs_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "svs_host_free": (C.c_int, [C.c_void_p]),
    "svs_capacity_bits": (C.c_uint64, [_PL, C.c_int]),
    "svs_packed_bytes": (C.c_uint64, [C.c_uint64]),
    "svs_embed_dev": (C.c_int, [_u8p, _u8p, _PL, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.c_void_p]),
    "svs_embed": (C.c_int, [_u8p, _u8p, _PL, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]),
    "svs_embed_str": (C.c_int, [_u8p, _u8p, _u8p, _PL, C.c_double, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_extract_str": (C.c_int, [_u8p, _PL, C.c_double, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_embed_ordered_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                         _u64p, C.c_void_p]),
    "svs_extract_ordered_dev": (C.c_int, [_u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p,
                                           C.c_void_p]),
    "svs_embed_ordered": (C.c_int, [_u8p, _u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                     _u64p]),
    "svs_extract_ordered": (C.c_int, [_u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_coeffs_scan": (C.c_int, [_CO, C.c_int, C.c_int, C.c_int]),
    "svs_embed_select_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, C.c_double, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p,
                                        C.c_void_p]),
    "svs_extract_select_dev": (C.c_int, [_u8p, _PL, _BO, _CO, C.c_double, _u8p, C.c_uint64, C.c_uint32, _u64p, C.c_void_p]),
    "svs_embed_select": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, C.c_double, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]),
    "svs_extract_select": (C.c_int, [_u8p, _PL, _BO, _CO, C.c_double, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_embed_dithered_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                          C.c_uint32, _u64p, C.c_void_p]),
    "svs_extract_dithered_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p,
                                            C.c_void_p]),
    "svs_embed_dithered": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                      C.c_uint32, _u64p]),
    "svs_extract_dithered": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_soft_extract_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p,
                                        C.c_void_p]),
    "svs_soft_extract": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_soft_vote_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                     _u64p, C.c_void_p]),
    "svs_soft_vote": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                 _u64p]),
    "svs_soft_histogram_dev": (C.c_int, [_u8p, _PL, _CO, _DI, C.c_double, C.c_int, C.c_void_p, C.c_uint32, _u64p, C.c_void_p]),
    "svs_soft_histogram": (C.c_int, [_u8p, _PL, _CO, _DI, C.c_double, C.c_int, C.c_void_p, C.c_uint32, _u64p]),
    "svs_quality_steps": (C.c_int, [_ST, C.c_int]),
    "svs_requantise_dev": (C.c_int, [_u8p, _u8p, _PL, _ST, C.c_uint32, C.c_void_p]),
    "svs_requantise": (C.c_int, [_u8p, _u8p, _PL, _ST, C.c_uint32]),
    "svs_matched_steps": (C.c_int, [_QS, _ST, C.c_int, C.c_int]),
    "svs_stepped_embed_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                         _u64p, C.c_void_p]),
    "svs_stepped_embed": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]),
    "svs_stepped_extract_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p, C.c_void_p]),
    "svs_stepped_extract": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_stepped_soft_extract_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p,
                                                C.c_void_p]),
    "svs_stepped_soft_extract": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_stepped_soft_vote_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                             _u64p, C.c_void_p]),
    "svs_stepped_soft_vote": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                         _u64p]),
    "svs_stepped_soft_histogram_dev": (C.c_int, [_u8p, _PL, _CO, _DI, _QS, C.c_int, C.c_void_p, C.c_uint32, _u64p, C.c_void_p]),
    "svs_stepped_soft_histogram": (C.c_int, [_u8p, _PL, _CO, _DI, _QS, C.c_int, C.c_void_p, C.c_uint32, _u64p]),
    "svs_matrix_capacity_bits": (C.c_uint64, [_PL, _MX]),
    "svs_matrix_embed_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, _MX, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                        _u64p, C.c_void_p]),
    "svs_matrix_embed": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, _MX, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                    _u64p]),
    "svs_matrix_extract_dev": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, _MX, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p,
                                          C.c_void_p]),
    "svs_matrix_extract": (C.c_int, [_u8p, _PL, _BO, _CO, _DI, _QS, _MX, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_embed_readback_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                          _u64p, C.c_void_p, C.c_void_p]),
    "svs_embed_readback": (C.c_int, [_u8p, _u8p, _PL, _BO, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32,
                                      _u64p, C.POINTER(ReadbackCounts)]),
    "svs_embed_dithered_readback_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64,
                                                   C.c_uint64, C.c_uint32, _u64p, C.c_void_p, C.c_void_p]),
    "svs_embed_dithered_readback": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                               C.c_uint32, _u64p, C.POINTER(ReadbackCounts)]),
    "svs_stepped_embed_readback_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                                  C.c_uint32, _u64p, C.c_void_p, C.c_void_p]),
    "svs_stepped_embed_readback": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                              C.c_uint32, _u64p, C.POINTER(ReadbackCounts)]),
    "svs_stepped_embed_readback_margin_dev": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                                         C.c_uint32, C.c_uint32, _u64p, C.c_void_p, C.c_void_p]),
    "svs_stepped_embed_readback_margin": (C.c_int, [_u8p, _u8p, _PL, _BO, _CO, _DI, _QS, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                                     C.c_uint32, C.c_uint32, _u64p, C.POINTER(MarginCounts)]),
    "svs_extract_dev": (C.c_int, [_u8p, _PL, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p, C.c_void_p]),
    "svs_extract": (C.c_int, [_u8p, _PL, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint32, _u64p]),
    "svs_bgr_to_gray_dev": (C.c_int, [_u8p, C.c_int64, C.c_int64, _u8p, _PL, C.c_void_p, C.c_void_p]),
    "svs_gray_to_bgr_dev": (C.c_int, [_u8p, _PL, _u8p, C.c_int64, C.c_int64, C.c_void_p]),
    "svs_embed_bgr_dev": (C.c_int, [_u8p, C.c_int64, C.c_int64, _u8p, C.c_int64, C.c_int64, _u8p, _PL, C.c_void_p,
                                     C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.c_void_p]),
    "svs_extract_bgr_dev": (C.c_int, [_u8p, C.c_int64, C.c_int64, _PL, C.c_void_p, C.c_double, C.c_int, _u8p,
                                       C.c_uint64, _u64p, C.c_void_p]),
    "svs_embed_bgr": (C.c_int, [_u8p, _u8p, _u8p, _PL, C.c_void_p, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                 C.c_uint32, _u64p]),
    "svs_extract_bgr": (C.c_int, [_u8p, _PL, C.c_void_p, C.c_double, C.c_int, _u8p, C.c_uint64, _u64p]),
    "svs_embed_bgr_readback_dev": (C.c_int, [_u8p, C.c_int64, C.c_int64, _u8p, C.c_int64, C.c_int64, _u8p, _PL, C.c_void_p,
                                              C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, C.c_void_p,
                                              C.c_void_p]),
    "svs_embed_bgr_readback": (C.c_int, [_u8p, _u8p, _u8p, _PL, C.c_void_p, C.c_double, C.c_int, _u8p, C.c_uint64, C.c_uint64,
                                          C.c_uint32, _u64p, C.POINTER(ReadbackCounts)]),
    "svs_fill_synthetic_dev": (C.c_int, [_u8p, _PL, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "svs_fill_bits_dev": (C.c_int, [_u8p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]),
    "svs_frame_sse_dev": (C.c_int, [_u8p, _u8p, _PL, C.c_void_p, C.c_void_p]),
    "svs_ssim_workspace_bytes": (C.c_uint64, [_PL]),
    "svs_frame_ssim_dev": (C.c_int, [_u8p, _u8p, _PL, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "svs_bit_errors_dev": (C.c_int, [_u8p, _u8p, C.c_uint64, C.c_void_p, C.c_void_p]),
}

def load_library(path: str, signatures: dict, abi_symbol: str, version: int) -> C.CDLL:
    """The one loader of the package's shared libraries: the library at `path` with the prototype of every name in `signatures`
    attached and its ABI version (`abi_symbol`, svs_rs_abi_version: libsvsrs.so) checked against `version`; SVS_SKIP_ABI_CHECK
    in the environment lets a mismatch through (A/B runs against old builds).  Loading does not touch the GPU."""
    stem = abi_symbol[: -len("_abi_version")].replace("_", "")
    so = "lib" + ("svsdct" if stem == "svs" else stem) + ".so"
    if not os.path.exists(path):
        raise SvsNativeError(f"{so} not found at {path}; build it with `python __graft_entry__.py` "
                             f"(or `make -C <package>/csrc`). There is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as exc:  # missing ROCm runtime etc.
        raise SvsNativeError(f"cannot load {path}: {exc}") from exc
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise SvsNativeError(f"{path} does not export {name}; rebuild it") from exc
        fn.restype, fn.argtypes = res, args
    got = getattr(lib, abi_symbol)()
    if got != version and not os.environ.get("SVS_SKIP_ABI_CHECK"):
        raise SvsNativeError(f"ABI version mismatch: {path} reports {got}, the binding expects {version}; rebuild {so}")
    return lib


def bind(module: dict, prefix: str):
    """(load, check) of the binding module whose globals() are `module` and whose symbols start with `prefix` (svs_fec:
    svs_fec_abi_version, svs_fec_last_error).  load() loads the module's LIB_PATH once, with its SIGNATURES and ABI_VERSION, and
    keeps the library in the module's `_lib`, which a caller may assign to route the calls elsewhere; all four are read at the
    call.  check(rc, what) raises SvsNativeError with the library's last error unless rc is SVS_OK."""
    module.setdefault("_lib", None)

    def load() -> C.CDLL:
        if module["_lib"] is None:
            module["_lib"] = load_library(module["LIB_PATH"], module["SIGNATURES"], prefix + "_abi_version", module["ABI_VERSION"])
        return module["_lib"]

    def check(rc: int, what: str) -> None:
        if rc != SVS_OK:
            msg = getattr(load(), prefix + "_last_error")().decode("utf-8", "replace")
            raise SvsNativeError(f"{what} failed ({rc}): {msg}", rc)

    load.__doc__ = "Load the library once and attach prototypes.  Loading does not touch the GPU."
    return load, check


load, check = bind(globals(), "svs")


_current = threading.local()      # hipSetDevice is per host thread: remember what THIS thread last selected


def ensure_device(device: int = 0) -> None:
    """Make `device` the calling thread's HIP device (svs_init = hipSetDevice + a usability check) unless this thread
    selected it already; raises when no GPU is usable.  A process that alternates devices, or a new thread, is
    switched explicitly instead of silently running on whatever device was current."""
    if getattr(_current, "device", None) == device:
        return
    check(load().svs_init(device), f"svs_init({device})")
    _current.device = device


def release_thread_context() -> None:
    """Give back the calling thread's staging context of the host-pointer entry points (svs_shutdown: two streams and the
    device buffers the thread's calls grew); the next such call builds a new one.  The frame pipelines call it when they
    close, so a worker thread that has processed a clip does not keep HBM for the rest of the process."""
    if _lib is not None:
        _lib.svs_shutdown()


def device_arch(device: int = 0) -> str:
    buf = C.create_string_buffer(128)
    check(load().svs_device_arch(device, buf, len(buf)), "svs_device_arch")
    return buf.value.decode()
