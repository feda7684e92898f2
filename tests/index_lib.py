"""Helpers of the index-arithmetic tests.

CPU half: the functions of csrc/svs_index.hpp and the payload readers of csrc/svs_block.hpp as tests/hostemu exports them
(tests/test_index_arithmetic_cpu.py).  GPU half: SparseFrames - a device allocation that spans pitched frames gigabytes
apart of which only the frames' rows are ever uploaded or downloaded, with sentinel windows where a truncated offset would
land (tests/test_index_arithmetic_gpu.py)."""
import ctypes as C

import numpy as np

from testlib import hostemu

K_EIGHTH = 0xFFFFFFFF          # svs::kEighth
WG = 256                       # SVS_WG: blocks per workgroup with one block per lane

_bound = False


def emu():
    global _bound
    lib = hostemu()
    if not _bound:
        lib.emu_make_div.argtypes = [C.c_uint32, C.c_void_p]
        lib.emu_fast_div.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        lib.emu_tile_of.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        lib.emu_tile_of_one.restype = C.c_uint32
        lib.emu_tile_of_one.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.emu_block_offset.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        lib.emu_stream_first.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32,
                                         C.c_void_p, C.c_void_p]
        lib.emu_payload_window.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
        lib.emu_payload_qword.restype = C.c_uint64
        lib.emu_payload_qword.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64]
        lib.emu_window32.restype = C.c_uint32
        lib.emu_window32.argtypes = [C.c_uint64, C.c_uint32]
        _bound = True
    return lib


def make_div(d):
    """-> (mul, shift, div) of svs::make_div(d)"""
    out = np.zeros(3, np.uint32)
    emu().emu_make_div(int(d), out.ctypes.data)
    return tuple(int(v) for v in out)


def fast_div(ns, d):
    ns = np.ascontiguousarray(ns, np.uint32)
    out = np.empty_like(ns)
    emu().emu_fast_div(ns.ctypes.data, ns.size, int(d), out.ctypes.data)
    return out


def tile_map(grid, chunk):
    """tile_of(i, grid, chunk) for every workgroup i < grid"""
    out = np.empty(grid, np.uint32)
    emu().emu_tile_of(int(grid), int(chunk), out.ctypes.data)
    return out


def block_offsets(gblocks, wb, bpf, row_pitch, frame_pitch, bgr=False):
    gblocks = np.ascontiguousarray(gblocks, np.uint32)
    out = np.empty(gblocks.size, np.int64)
    emu().emu_block_offset(gblocks.ctypes.data, gblocks.size, int(wb), int(bpf), int(row_pitch), int(frame_pitch), int(bgr),
                           out.ctypes.data)
    return out


def stream_firsts(gblocks, n, bpf, key=None, first_frame=0, want_second=False):
    gblocks = np.ascontiguousarray(gblocks, np.uint32)
    first, second = np.empty(gblocks.size, np.uint64), np.empty(gblocks.size, np.uint64)
    emu().emu_stream_first(gblocks.ctypes.data, gblocks.size, int(n), int(bpf), int(key is not None), int(key or 0),
                           int(first_frame), first.ctypes.data, second.ctypes.data if want_second else None)
    return (first, second) if want_second else first


_sparse = None


def sparse_payload():
    """uint8 view of a 16 GiB anonymous mapping that reserves no memory (pages appear when written, untouched ones read as
    zero): a payload buffer of up to 2^32 - 1 dwords of which a test writes a few windows.  A reader that truncates a word
    index then reads other bytes of the mapping - a mismatch, not a fault.  None where such a mapping is refused (the
    readers are then shown the window alone, through a biased pointer)."""
    global _sparse
    if _sparse is None:
        import mmap
        try:
            m = mmap.mmap(-1, (1 << 34) + 4096, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0))
            _sparse = np.frombuffer(m, np.uint8)
        except (OSError, ValueError, OverflowError):
            _sparse = False
    return _sparse if _sparse is not False else None


def payload_window(window_words, word_base, n_words, s):
    """svs::payload_window at stream bit s of a buffer of n_words dwords whose dwords [word_base, word_base + len) are
    window_words (little-endian dwords of the packed bytes) -> the 64 stream bits as one integer, MSB first"""
    w = np.ascontiguousarray(window_words, np.uint32)
    out = np.zeros(2, np.uint32)
    emu().emu_payload_window(w.ctypes.data, int(word_base), int(n_words), int(s), out.ctypes.data)
    return (int(out[0]) << 32) | int(out[1])


def payload_qword(window_words, word_base, n_words, s):
    w = np.ascontiguousarray(window_words, np.uint32)
    return int(emu().emu_payload_qword(w.ctypes.data, int(word_base), int(n_words), int(s)))


# ---- GPU half ---------------------------------------------------------------------------------------------------------
class DevBuf:
    """a device allocation freed by close() (or on exit of a `with`), not whenever the collector gets to it"""

    def __init__(self, nbytes):
        from svsdct import native
        self.native, self.lib = native, native.load()
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        native.check(self.lib.svs_malloc(C.byref(self.ptr), self.nbytes), f"svs_malloc({self.nbytes})")

    @property
    def addr(self):
        return self.ptr.value

    def memset(self, value, offset=0, nbytes=None):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        assert 0 <= offset and offset + nbytes <= self.nbytes
        self.native.check(self.lib.svs_memset(C.c_void_p(self.addr + offset), int(value), int(nbytes), None), "svs_memset")

    def put(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        self.native.check(self.lib.svs_memcpy_h2d(C.c_void_p(self.addr + offset), arr.ctypes.data, arr.nbytes, None), "h2d")
        self.sync()

    def get(self, offset=0, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        assert 0 <= offset and offset + nbytes <= self.nbytes
        out = np.empty(int(nbytes), np.uint8)
        self.native.check(self.lib.svs_memcpy_d2h(out.ctypes.data, C.c_void_p(self.addr + offset), out.nbytes, None), "d2h")
        self.sync()
        return out.view(dtype)

    def sync(self):
        self.native.check(self.lib.svs_stream_synchronize(None), "sync")

    def close(self):
        if self.ptr:
            self.sync()
            self.lib.svs_free(self.ptr)
            self.ptr = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()


SENTINEL, SENTINEL_BYTES = 0x5A, 4096


class SparseFrames(DevBuf):
    """Pitched frames in ONE allocation that covers their whole span: a truncated offset lands inside it and shows as a
    mismatch, not as a fault.  Only the frames' rows travel.  px = bytes per pixel (1 gray, 3 interleaved BGR).  `fill`:
    the byte the span is set to before anything is uploaded.  For every frame (or, with one frame, every 8-row band) whose
    offset o is >= 2^31, a 4 KiB sentinel window is set at o mod 2^32 and at o mod 2^31 - where a 32-bit or a sign-extended
    31-bit offset would land - unless that window meets a frame's rows; check_sentinels() asserts they are untouched."""

    def __init__(self, f, h, w, row_pitch, frame_pitch, px=1, fill=0xC3):
        self.f, self.h, self.w, self.px = f, h, w, px
        self.row_pitch, self.frame_pitch = int(row_pitch), int(frame_pitch)
        self.row_bytes = w * px
        super().__init__((f - 1) * self.frame_pitch + (h - 1) * self.row_pitch + self.row_bytes + 64)
        self.memset(fill)
        self.fill = fill
        self.sentinels = []
        starts = [k * self.frame_pitch + r * self.row_pitch for k in range(f) for r in range(0, h, 8)]
        for o in starts:
            if o < (1 << 31):
                continue
            for at in {o % (1 << 32), o % (1 << 31)}:
                at -= at % 8
                if at + SENTINEL_BYTES <= self.nbytes and not self._meets_rows(at, at + SENTINEL_BYTES) and at not in self.sentinels:
                    self.memset(SENTINEL, at, SENTINEL_BYTES)
                    self.sentinels.append(at)
        self.sync()

    def _meets_rows(self, lo, hi):
        for k in range(self.f):
            for r in range(self.h):
                o = k * self.frame_pitch + r * self.row_pitch
                if o < hi and lo < o + self.row_bytes:
                    return True
        return False

    def upload(self, frames):
        """frames: uint8 [f, h, w] (gray) or [f, h, w, 3]"""
        frames = np.ascontiguousarray(frames).reshape(self.f, self.h, self.row_bytes)
        for k in range(self.f):
            self._rows(k, frames[k])
        self.sync()

    def _rows(self, k, rows):
        for r in range(self.h):
            row = np.ascontiguousarray(rows[r])
            self.native.check(self.lib.svs_memcpy_h2d(C.c_void_p(self.addr + k * self.frame_pitch + r * self.row_pitch),
                                                      row.ctypes.data, row.nbytes, None), "h2d")

    def download(self):
        """-> uint8 [f, h, w * px]: the frames' rows"""
        out = np.empty((self.f, self.h, self.row_bytes), np.uint8)
        for k in range(self.f):
            for r in range(self.h):
                self.native.check(self.lib.svs_memcpy_d2h(out[k, r].ctypes.data,
                                                          C.c_void_p(self.addr + k * self.frame_pitch + r * self.row_pitch),
                                                          self.row_bytes, None), "d2h")
        self.sync()
        return out

    def padding_after_rows(self, nbytes=64):
        """the bytes right after every frame's first and last row are still the fill (where no row or sentinel sits)"""
        ok = True
        for k in range(self.f):
            for r in (0, self.h - 1):
                at = k * self.frame_pitch + r * self.row_pitch + self.row_bytes
                n = min(nbytes, self.row_pitch - self.row_bytes) if r < self.h - 1 else nbytes
                if n > 0 and not self._meets_rows(at, at + n) and \
                        not any(s < at + n and at < s + SENTINEL_BYTES for s in self.sentinels):
                    ok = ok and bool((self.get(at, n) == self.fill).all())
        return ok

    def check_sentinels(self):
        assert self.sentinels, "no sentinel window was placed: the geometry reaches no offset past 2^31"
        for at in self.sentinels:
            got = self.get(at, SENTINEL_BYTES)
            assert (got == SENTINEL).all(), f"sentinel window at byte {at} was written ({int((got != SENTINEL).sum())} bytes)"
