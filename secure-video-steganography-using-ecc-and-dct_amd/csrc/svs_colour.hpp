// svs_colour.hpp - the keep-colour stego pixel (SVS_KEEP_COLOUR, include/svsdct.h).
//
// The reference writes every payload frame as cvtColor(stego_gray, COLOR_GRAY2BGR) (embed_process.py:126); its receiver
// only ever looks at cvtColor(frame, COLOR_BGR2GRAY) (config_and_setup.py:111-112).  So any BGR pixel whose fixed-point
// gray is the stego gray carries the reference's bits.  With weights wb + wg + wr = 2^s, adding the same d to B, G and R
// adds exactly d to the gray: w.(c + d) = w.c + d 2^s.  This header picks, for a cover pixel c and a target gray t, the
// pixel closest to "c shifted by t - gray(c)" whose gray is exactly t:
//   1. P = clamp(c + d, 0, 255) per channel, d = t - gray(c).  Done if gray(P) == t (always, when nothing clipped).
//   2. Otherwise visit the channels of positive weight in decreasing weight order (ties: B, G, R), stopping as soon as
//      gray(P) == t, and move each toward t by the smallest amount that reaches t, limited by its range [0, 255].
// Every weight is <= 2^s, so a unit step moves the gray by at most 1 and never jumps past t; all positive-weight
// channels at 255 (0) give gray 255 (0), so the walk always ends on t; step 1 leaves gray(P) between gray(c) and t, so
// every channel moves only in the direction of d.  d == 0 gives P == c.
//
// Plain integer arithmetic on values < 2^24: the host (tests) and the gfx950 kernel (svs_device.hpp, clipped pixels
// only) compute the same bytes.
#pragma once
#include <stdint.h>

#include "svs_block.hpp"

namespace svs {

SVS_HD uint32_t colour_gray(uint32_t b, uint32_t g, uint32_t r, uint32_t wb, uint32_t wg, uint32_t wr, uint32_t shift) {
    return (b * wb + g * wg + r * wr + (1u << (shift - 1))) >> shift;
}

SVS_HD uint32_t clamp_u8(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// (b, g, r): the cover pixel on entry, the keep-colour pixel on return; t: the stego gray (0..255)
SVS_HD void keep_colour_pixel(uint32_t &b, uint32_t &g, uint32_t &r, uint32_t t, uint32_t wb, uint32_t wg, uint32_t wr,
                              uint32_t shift) {
    const int d = (int)t - (int)colour_gray(b, g, r, wb, wg, wr, shift);
    uint32_t p[3] = {clamp_u8((int)b + d), clamp_u8((int)g + d), clamp_u8((int)r + d)};
    uint32_t w[3] = {wb, wg, wr}, ch[3] = {0u, 1u, 2u};
    const uint32_t one = 1u << shift, half = one >> 1;
    if (((w[0] * p[0] + w[1] * p[1] + w[2] * p[2] + half) >> shift) != t) {
        // sort the channels by decreasing weight (stable: B, G, R among equals) - a three-element network
#define SVS_KC_SWAP(i, j)                                                                                            \
    if (w[i] < w[j]) {                                                                                               \
        const uint32_t tw = w[i], tp = p[i], tc = ch[i];                                                             \
        w[i] = w[j]; p[i] = p[j]; ch[i] = ch[j];                                                                     \
        w[j] = tw; p[j] = tp; ch[j] = tc;                                                                            \
    }
        SVS_KC_SWAP(1, 2) SVS_KC_SWAP(0, 1) SVS_KC_SWAP(1, 2)
#undef SVS_KC_SWAP
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 3; ++k) {
            if (w[k] == 0u) continue;
            const uint32_t acc = w[0] * p[0] + w[1] * p[1] + w[2] * p[2];
            const uint32_t y = (acc + half) >> shift;
            if (y < t) {          // smallest m with acc + m w_k + half >= t 2^s
                const uint32_t need = (t * one - half - acc + w[k] - 1u) / w[k], room = 255u - p[k];
                p[k] += need < room ? need : room;
            } else if (y > t) {   // smallest m with acc - m w_k + half < (t + 1) 2^s
                const uint32_t need = (acc + half + 1u - (t + 1u) * one + w[k] - 1u) / w[k];
                p[k] -= need < p[k] ? need : p[k];
            }
        }
    }
    // back to B, G, R
    b = ch[0] == 0u ? p[0] : ch[1] == 0u ? p[1] : p[2];
    g = ch[0] == 1u ? p[0] : ch[1] == 1u ? p[1] : p[2];
    r = ch[0] == 2u ? p[0] : ch[1] == 2u ? p[1] : p[2];
}

}  // namespace svs
