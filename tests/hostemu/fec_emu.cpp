// fec_emu.cpp - test-only host build of csrc/svs_fec.hpp: the decoder of include/svsfec.h as the kernel of csrc/svs_fec.hip
// walks it - one segment at a time, 64 states a step, a decision word a step, the traceback over the words - with every
// per-step value coming from the header's functions.  tests/fec_lib.py compiles it with g++ into a shared library; with
// -DFEC_EMU_MAIN it is a stand-alone program (its own main) that tests/test_fec_cpu.py builds with
// -fsanitize=address,undefined and runs once.
#include "svs_fec.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace svsfec;

template <int RATE, typename In>
void decode_segment(const In *in, uint64_t n_info, uint64_t seg, uint8_t *out, uint64_t out_bytes) {
    const uint64_t n = n_info + kTail, a = seg * kSegment;
    const uint64_t ws = window_start(a), we = window_end(a, n);
    const int len = (int)(we - ws);
    std::vector<int16_t> w((size_t)RATE * len);
    std::vector<uint64_t> dec((size_t)len);
    for (int i = 0; i < RATE * len; ++i) w[i] = (int16_t)weight_of(in[(uint64_t)RATE * ws + i]);

    int32_t m[kStates], next[kStates];
    int sign[kStates][3];
    for (int s = 0; s < kStates; ++s) {
        m[s] = start_metric(ws, (uint32_t)s);
        for (int j = 0; j < 3; ++j) sign[s][j] = branch_sign((uint32_t)s, j);
    }
    for (int t = 0; t < len; ++t) {
        const int32_t ww[3] = {w[RATE * t], w[RATE * t + 1], RATE == 3 ? w[RATE * t + 2] : 0};
        uint64_t word = 0;
        for (int s = 0; s < kStates; ++s) {
            uint32_t d;
            next[s] = acs(m[pred0(s)], m[pred0(s) + 1], branch_metric<RATE>(sign[s], ww), &d);
            word |= (uint64_t)d << s;
        }
        memcpy(m, next, sizeof m);
        dec[t] = word;
    }
    uint32_t s = 0;
    if (we != n)
        for (int k = 1; k < kStates; ++k)
            if (m[k] > m[s]) s = (uint32_t)k;          // the lowest-numbered state with the largest metric
    uint8_t bytes[kSegment / 8] = {0};
    for (int t = len - 1; t >= (int)(a - ws); --t) {
        const uint32_t bit = trace_step(dec[t], &s);
        const int at = t - (int)(a - ws);              // the step's place in the segment
        if (at < kSegment && ws + t < n_info) bytes[at >> 3] |= (uint8_t)(bit << (7 - (at & 7)));
    }
    for (int i = 0; i < kSegment / 8; ++i)
        if (seg * (kSegment / 8) + i < out_bytes) out[seg * (kSegment / 8) + i] = bytes[i];
}

template <typename In>
int decode(const In *in, uint64_t n_info, int rate, uint8_t *out) {
    if (rate != 2 && rate != 3) return -1;
    const uint64_t out_bytes = (n_info + 7) / 8, n_segments = (n_info + kSegment - 1) / kSegment;
    for (uint64_t seg = 0; seg < n_segments; ++seg) {
        if (rate == 2) decode_segment<2, In>(in, n_info, seg, out, out_bytes);
        else decode_segment<3, In>(in, n_info, seg, out, out_bytes);
    }
    return 0;
}

}  // namespace

extern "C" {
int fec_emu_decode_soft(const uint8_t *soft, uint64_t n_info, int rate, uint8_t *out) { return decode(soft, n_info, rate, out); }
int fec_emu_decode_weights(const int32_t *weights, uint64_t n_info, int rate, uint8_t *out) { return decode(weights, n_info, rate, out); }
}

#if defined(FEC_EMU_MAIN)
// the stand-alone program: encodes with the header's step, decodes clean and noisy streams of both kinds in buffers of exactly
// the size a call may touch (a sanitizer sees one byte too many), and checks the clean round trips
static uint32_t lcg(uint32_t *x) { return *x = *x * 1664525u + 1013904223u; }

int main() {
    const uint64_t lengths[] = {1, 2, 58, 59, 506, 507, 570, 571, 1018, 1019, 2045, 5000};
    uint32_t seed = 12345u;
    int runs = 0;
    for (uint64_t n_info : lengths)
        for (int rate = 2; rate <= 3; ++rate) {
            const uint64_t n = n_info + kTail, nc = rate * n;
            std::vector<uint8_t> info(n_info), soft(nc), out((n_info + 7) / 8), noisy(out.size());
            std::vector<int32_t> wide(nc);
            uint32_t s = 0;
            for (uint64_t t = 0; t < n; ++t) {
                const uint32_t x = t < n_info ? (info[t] = (lcg(&seed) >> 16) & 1u) : 0u;
                for (int j = 0; j < rate; ++j) {
                    const uint32_t c = output_bit(s, x, j), r = lcg(&seed) >> 8;
                    soft[rate * t + j] = (uint8_t)((c << 7) | (r & 127u));
                    wide[rate * t + j] = (r % 7 == 0) ? (c ? INT32_MAX : INT32_MIN) : (int32_t)((c ? 1 : -1) * (int32_t)(1 + r % 100000u));
                }
                s = next_state(s, x);
            }
            if (s != 0) return printf("the tail does not end in state 0\n"), 1;
            for (int kind = 0; kind < 3; ++kind) {
                memset(out.data(), 0xEE, out.size());
                if (kind == 2)                              // noise: flips at the lowest confidence, zeros
                    for (uint64_t i = 0; i < nc; i += 11) soft[i] = (uint8_t)((soft[i] & 0x80u) ^ 0x80u);
                const int rc = kind == 1 ? fec_emu_decode_weights(wide.data(), n_info, rate, out.data())
                                         : fec_emu_decode_soft(soft.data(), n_info, rate, out.data());
                if (rc != 0) return printf("decode refused\n"), 1;
                uint64_t wrong = 0;
                for (uint64_t t = 0; t < n_info; ++t) wrong += ((out[t >> 3] >> (7 - (t & 7))) & 1u) != info[t];
                if (n_info & 7 && (out.back() & (0xFFu >> (n_info & 7)))) return printf("pad bits set\n"), 1;
                if (kind < 2 && wrong) return printf("n_info %llu rate %d kind %d: %llu wrong\n", (unsigned long long)n_info, rate, kind, (unsigned long long)wrong), 1;
                ++runs;
            }
        }
    printf("fec emu ok: %d decodes\n", runs);
    return 0;
}
#endif
