// keep_colour_shim.cpp - TEST INFRASTRUCTURE ONLY: the host build of csrc/svs_colour.hpp (the keep-colour rule the
// gfx950 kernel applies), for tests/test_keep_colour_cpu.py.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I<csrc> keep_colour_shim.cpp -o <tmp>/libkc.so
#include <cstdint>

#include "svs_colour.hpp"

namespace {

// violations[0..3]: gray(out) != t, out != c + d although nothing clips, d == 0 but out != c, a channel moved against d
void check_one(uint32_t c, uint32_t t, const uint32_t *w, uint64_t *v) {
    const uint32_t c0 = c & 0xffu, c1 = (c >> 8) & 0xffu, c2 = (c >> 16) & 0xffu;
    uint32_t b = c0, g = c1, r = c2;
    svs::keep_colour_pixel(b, g, r, t, w[0], w[1], w[2], w[3]);
    const int d = (int)t - (int)svs::colour_gray(c0, c1, c2, w[0], w[1], w[2], w[3]);
    v[0] += svs::colour_gray(b, g, r, w[0], w[1], w[2], w[3]) != t;
    const int lo = (int)(c0 < c1 ? (c0 < c2 ? c0 : c2) : (c1 < c2 ? c1 : c2));
    const int hi = (int)(c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2));
    if (lo + d >= 0 && hi + d <= 255)
        v[1] += (int)b != (int)c0 + d || (int)g != (int)c1 + d || (int)r != (int)c2 + d;
    if (d == 0) v[2] += b != c0 || g != c1 || r != c2;
    const int mv[3] = {(int)b - (int)c0, (int)g - (int)c1, (int)r - (int)c2};
    for (int k = 0; k < 3; ++k) v[3] += (d > 0 && mv[k] < 0) || (d < 0 && mv[k] > 0) || (d == 0 && mv[k] != 0);
}

}  // namespace

extern "C" {

// bgr / out: n pixels of 3 bytes; t: n target grays; w: {wb, wg, wr, shift}
void kc_apply(const uint8_t *bgr, const uint8_t *t, uint8_t *out, uint64_t n, const uint32_t *w) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
        svs::keep_colour_pixel(b, g, r, t[i], w[0], w[1], w[2], w[3]);
        out[3 * i] = (uint8_t)b; out[3 * i + 1] = (uint8_t)g; out[3 * i + 2] = (uint8_t)r;
    }
}

// every colour (c = B | G << 8 | R << 16, first .. first + count - 1) x every t with |t - gray(c)| <= radius
// (radius >= 255: every t); returns the number of (c, t) pairs checked, violations in v[4]
uint64_t kc_check(uint32_t first, uint32_t count, uint32_t stride, int radius, const uint32_t *w, uint64_t *v) {
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t c = (first + i * stride) & 0xffffffu;
        const int g0 = (int)svs::colour_gray(c & 0xffu, (c >> 8) & 0xffu, (c >> 16) & 0xffu, w[0], w[1], w[2], w[3]);
        const int lo = g0 - radius < 0 ? 0 : g0 - radius, hi = g0 + radius > 255 ? 255 : g0 + radius;
        for (int t = lo; t <= hi; ++t, ++pairs) check_one(c, (uint32_t)t, w, v);
    }
    return pairs;
}

}
