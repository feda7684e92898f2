"""The device buffers of one staged call: what a function that takes NumPy arrays puts around the *_device call it wraps.

    with Staged(device) as dev:
        d_in, d_out = dev.upload(values), dev.alloc(out_bytes)
        ... enqueue on the null stream ...
        out = dev.download(d_out, out_bytes)
        dev.synchronise()                                    # `out` holds the bytes from here on

Everything goes through libsvsdct.so's svs_malloc / svs_memcpy_* / svs_memset on the null stream; the buffers are freed when the
block ends.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native


class Staged:
    def __init__(self, device: int = 0):
        self.lib, self.ptrs, self.held = native.load(), [], []
        native.ensure_device(device)

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        native.check(self.lib.svs_malloc(C.byref(p), max(int(nbytes), 4)), "svs_malloc")
        self.ptrs.append(p)
        return p.value

    def upload(self, host: np.ndarray, d_to: int | None = None) -> int:
        """a C-contiguous array -> a buffer of its size (d_to: into that one instead); the scope holds the array until it ends"""
        d_to = self.alloc(host.nbytes) if d_to is None else d_to
        self.held.append(host)
        if host.nbytes:
            native.check(self.lib.svs_memcpy_h2d(d_to, host.ctypes.data, host.nbytes, None), "svs_memcpy_h2d")
        return d_to

    def zero(self, d_at: int, nbytes: int) -> None:
        native.check(self.lib.svs_memset(d_at, 0, int(nbytes), None), "svs_memset")

    def download(self, d_from: int, into) -> np.ndarray:
        """into: a C-contiguous array to fill, or a number of bytes -> a new uint8 array; valid behind synchronise()"""
        out = into if isinstance(into, np.ndarray) else np.empty(int(into), np.uint8)
        if out.nbytes:
            native.check(self.lib.svs_memcpy_d2h(out.ctypes.data, d_from, out.nbytes, None), "svs_memcpy_d2h")
        return out

    def synchronise(self) -> None:
        native.check(self.lib.svs_stream_synchronize(None), "svs_stream_synchronize")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.svs_free(p)
        return False
