// svs_abi.hpp - what the host side of every library's C ABI shares: the last-error string behind svs_*_last_error, fail(), the
// check behind a kernel launch and the overlap test of two buffers.  Include it behind the library's public header (the SVS_ERR_*
// codes are that header's).  Several of the libraries are loaded into one process, so EVERYTHING HERE HAS INTERNAL LINKAGE (see the
// note at the top of csrc/svs_rs_decode.hpp): each translation unit, and so each library, owns an error string of its own.
// fail() and the string compile with a plain C++ compiler; launched() is there under hipcc only.
#pragma once

#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

bool overlap(const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

#if defined(__HIPCC__)
// behind a kernel launch of the call `what`
int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SVS_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    return SVS_OK;
}
#endif

}  // namespace
