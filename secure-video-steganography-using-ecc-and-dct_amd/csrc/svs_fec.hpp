// svs_fec.hpp - the per-step arithmetic of the convolutional code and its windowed Viterbi decoder (include/svsfec.h, "THE
// FORMAT"), in a form that compiles for the device (csrc/svs_fec.hip) and for the host (svs_fec_encode; tests/hostemu/fec_emu.cpp
// drives the same functions state by state).  Integers only.
#pragma once

#include <stdint.h>

#include <type_traits>

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

// ---- punctured codes ("Punctured codes" in the header): the rate-2 code with some coded bits not sent ----------------------
// period P, K kept bits a period; bit 2 i + j of `pattern` is set when out_j of step i of a period is sent.  period = 0: `code`
// is no punctured code
struct Puncture {
    int period, kept;
    uint32_t pattern;
};
SVS_FEC_HD constexpr Puncture puncture(int code) {
    return code == 23   ? Puncture{2, 3, 0x7u}         // out_0 1 1            out_1 1 0
           : code == 34 ? Puncture{3, 4, 0x27u}        //       1 1 0                1 0 1
           : code == 56 ? Puncture{5, 6, 0x267u}       //       1 1 0 1 0            1 0 1 0 1
           : code == 78 ? Puncture{7, 8, 0x2657u}      //       1 1 1 1 0 1 0        1 0 0 0 1 0 1
                        : Puncture{0, 0, 0u};
}
constexpr int kMotherRate = 2;

SVS_FEC_HD uint32_t punct_kept(const Puncture &pc, int i, int j) { return (pc.pattern >> (2 * i + j)) & 1u; }
// the kept bits of a period before out_j of its step i; j = 0: pre[i]
SVS_FEC_HD int punct_before(const Puncture &pc, int i, int j = 0) {
    return __builtin_popcount(pc.pattern & ((1u << (2 * i + j)) - 1u));
}
// S(t): the sent bits before step t.  64-bit: t reaches 2^40 + 6
SVS_FEC_HD uint64_t sent_before(const Puncture &pc, uint64_t t) {
    return t / (uint64_t)pc.period * (uint64_t)pc.kept + (uint64_t)punct_before(pc, (int)(t % (uint64_t)pc.period));
}
// the largest n with S(n) <= capacity.  S is strictly increasing (every step keeps a bit); period < kept, so n <= capacity
SVS_FEC_HD uint64_t steps_that_fit(const Puncture &pc, uint64_t capacity) {
    const int left = (int)(capacity % (uint64_t)pc.kept);
    int i = pc.period - 1;
    while (punct_before(pc, i) > left) --i;             // pre[0] = 0 ends it
    return capacity / (uint64_t)pc.kept * (uint64_t)pc.period + (uint64_t)i;
}

// Where a window finds its mother bits.  A window that starts at step ws = wq P + phase reads the run of sent values from
// S(ws) on; its step ws + k is step r of period wq + q, with phase + k = q P + r, and small numbers do from there.
struct PunctStep {
    int q, r;
};
SVS_FEC_HD PunctStep punct_step(const Puncture &pc, int u) { return PunctStep{u / pc.period, u % pc.period}; }
SVS_FEC_HD PunctStep punct_advance(const Puncture &pc, PunctStep s, int steps) {
    s.q += steps / pc.period;
    s.r += steps % pc.period;
    if (s.r >= pc.period) {
        s.r -= pc.period;
        ++s.q;
    }
    return s;
}
// the place of out_j of that step in the window's run (0 = the value at S(ws)), -1 when it is not sent
SVS_FEC_HD int sent_place(const Puncture &pc, int phase, PunctStep s, int j) {
    if (!punct_kept(pc, s.r, j)) return -1;
    return s.q * pc.kept + punct_before(pc, s.r, j) - punct_before(pc, phase);
}

// ---- the host side's rules about a rate code: 2, 3 or a punctured code -------------------------------------------------------
inline bool punctured(int rate) { return puncture(rate).period != 0; }
inline bool rate_ok(int rate) { return rate == 2 || rate == 3 || punctured(rate); }
constexpr const char *kRates = "none of 2, 3, 23, 34, 56, 78";

// the values a stream of n steps holds: rate * n, or S(n) of a punctured code
inline uint64_t stream_bits(uint64_t n, int rate) { return punctured(rate) ? sent_before(puncture(rate), n) : (uint64_t)rate * n; }

// f(std::integral_constant<int, rate>) of a rate that rate_ok() let through: the one place a runtime rate picks an instantiation
template <typename F>
inline void with_rate(int rate, F &&f) {
    switch (rate) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 23: f(std::integral_constant<int, 23>{}); break;
        case 34: f(std::integral_constant<int, 34>{}); break;
        case 56: f(std::integral_constant<int, 56>{}); break;
        default: f(std::integral_constant<int, 78>{}); break;
    }
}

}  // namespace svsfec
