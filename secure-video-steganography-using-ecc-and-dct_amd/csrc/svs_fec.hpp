// svs_fec.hpp - the per-step arithmetic of the convolutional code and its windowed Viterbi decoder (include/svsfec.h, "THE
// FORMAT"), in a form that compiles for the device (csrc/svs_fec.hip) and for the host (svs_fec_encode; tests/hostemu/fec_emu.cpp
// drives the same functions state by state).  Integers only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SVS_FEC_HD __host__ __device__ inline
#else
#define SVS_FEC_HD inline
#endif

namespace svsfec {

constexpr int kStates = 64;
constexpr int kSegment = 512;                      // SVS_FEC_SEGMENT
constexpr int kOverlap = 64;                       // SVS_FEC_OVERLAP
constexpr int kTail = 6;                           // SVS_FEC_TAIL
constexpr int kWindow = kSegment + 2 * kOverlap;   // the longest window: 640 steps
constexpr int kWeightMax = 32767;
constexpr int32_t kStartOff = -(1 << 30);          // the start metric of a state the encoder cannot be in
static_assert((int64_t)(kWindow + 1) * 3 * kWeightMax < (1ll << 30), "a window's metrics must stay inside int32");

// generators in octal 133, 171, 165; reg = (x << 6) | s.  Each has bit 0 set: the branches of p0 and p0 + 1 send opposite bits
SVS_FEC_HD uint32_t generator(int j) { return j == 0 ? 0133u : j == 1 ? 0171u : 0165u; }

SVS_FEC_HD uint32_t parity7(uint32_t v) {
    v ^= v >> 4;
    v ^= v >> 2;
    v ^= v >> 1;
    return v & 1u;
}

// out_j of the step that leaves state s with input x
SVS_FEC_HD uint32_t output_bit(uint32_t s, uint32_t x, int j) { return parity7(((x << 6) | s) & generator(j)); }
SVS_FEC_HD uint32_t next_state(uint32_t s, uint32_t x) { return ((x << 6) | s) >> 1; }

// the new state ns: its first predecessor, and the sign (2 out_j - 1) of coded bit j on the branch from it
SVS_FEC_HD uint32_t pred0(uint32_t ns) { return 2u * (ns & 31u); }
SVS_FEC_HD int branch_sign(uint32_t ns, int j) { return 2 * (int)output_bit(pred0(ns), ns >> 5, j) - 1; }

// weights
SVS_FEC_HD int32_t weight_of(uint8_t soft) { return (2 * (int32_t)(soft >> 7) - 1) * (2 * (int32_t)(soft & 127u) + 1); }
SVS_FEC_HD int32_t weight_of(int32_t v) { return v < -kWeightMax ? -kWeightMax : v > kWeightMax ? kWeightMax : v; }

// the window [ws, we) of the segment that starts at step a = 512 k, of n steps in all
SVS_FEC_HD uint64_t segment_end(uint64_t a, uint64_t n) { return a + kSegment < n ? a + kSegment : n; }
SVS_FEC_HD uint64_t window_start(uint64_t a) { return a >= (uint64_t)kOverlap ? a - kOverlap : 0; }
SVS_FEC_HD uint64_t window_end(uint64_t a, uint64_t n) {
    const uint64_t b = segment_end(a, n);
    return b + kOverlap < n ? b + kOverlap : n;
}
SVS_FEC_HD int32_t start_metric(uint64_t ws, uint32_t s) { return ws == 0 && s != 0 ? kStartOff : 0; }

// the branch metric of p0 from a state's signs and the step's weights
template <int RATE>
SVS_FEC_HD int32_t branch_metric(const int *sign, const int32_t *w) {
    int32_t bm = sign[0] * w[0] + sign[1] * w[1];
    if (RATE == 3) bm += sign[2] * w[2];
    return bm;
}

// add, compare, select: m0, m1 the metrics of p0 and p0 + 1 before the step -> the new metric; *d = 1 when p1 won
SVS_FEC_HD int32_t acs(int32_t m0, int32_t m1, int32_t bm, uint32_t *d) {
    const int32_t c0 = m0 + bm, c1 = m1 - bm;
    *d = c1 > c0 ? 1u : 0u;
    return *d ? c1 : c0;
}

// one step of the traceback: `word` holds d(t, .) of the 64 states -> the decoded bit of step t; *s becomes the predecessor
SVS_FEC_HD uint32_t trace_step(uint64_t word, uint32_t *s) {
    const uint32_t bit = *s >> 5;
    *s = 2u * (*s & 31u) + (uint32_t)((word >> *s) & 1u);
    return bit;
}

}  // namespace svsfec
